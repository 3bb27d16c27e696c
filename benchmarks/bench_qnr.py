"""D_lambda, D_s and QNR: the band-pair UQI kernel and the pan-degrade kernel vs the dispatch they replace (same
tensors, same process).

``spectral_distortion_index``, ``spatial_distortion_index`` and ``quality_with_no_reference`` (``pan_lr=None``, window 7)
through ``csrc/image/band_uqi.hip`` against the same calls with ``TM_AMD_BAND_UQI=0``, which restores the earlier
dispatch: every band pair gathered in front of the UQI window kernel, the pan degradation as a torch box filter +
bilinear resize.  The switch is read at call time, so the two paths alternate in timed windows of device events after a
warm-up of both; one JSON line per case: median ms of both (and the spread of the per-round values), their ratio and
both paths' values.  After all timings, one line per case with the device activities (kernels and copies) of one call
on either path (``torch.profiler``, in a pass of its own).

Usage: ``python benchmarks/bench_qnr.py [--out profiles/qnr_bench.jsonl]``
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F  # noqa: N812

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchmetrics_amd.functional.image import quality_with_no_reference  # noqa: E402
from torchmetrics_amd.functional.image import spatial_distortion_index  # noqa: E402
from torchmetrics_amd.functional.image import spectral_distortion_index  # noqa: E402

ROUNDS = 5
WINDOW_MS = 100.0  # per path and round: >= 500 ms of timed work per path
SWITCH = "TM_AMD_BAND_UQI"
METRICS = {
    "d_lambda": lambda p, ms, pan: spectral_distortion_index(p, ms),
    "d_s": lambda p, ms, pan: spatial_distortion_index(p, ms, pan, window_size=7),
    "qnr": lambda p, ms, pan: quality_with_no_reference(p, ms, pan, window_size=7),
}


def window_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def alternate(fns):
    """Per-call ms of every fn in each of ROUNDS alternating windows, after a warm-up."""
    reps = []
    for fn in fns:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps.append(max(1, int(WINDOW_MS / max(window_ms(fn, 1), 1e-3))))
    times = [[] for _ in fns]
    for _ in range(ROUNDS):
        for i, fn in enumerate(fns):
            times[i].append(window_ms(fn, reps[i]))
    return times


def tensors(shape, r, dtype, dev, gen):
    """Correlated bands in [0, 1], ``ms`` a noisy r-fold decimation of ``preds``, ``pan`` of the size of ``preds``."""
    b, c, h, w = shape
    base = torch.rand(b, 1, h, w, device=dev, generator=gen)
    mix = torch.linspace(0.2, 0.8, c, device=dev).view(1, c, 1, 1)
    preds = mix * base + (1 - mix) * torch.rand(shape, device=dev, generator=gen)
    ms = F.avg_pool2d(preds, r) + 0.05 * torch.rand(b, c, h // r, w // r, device=dev, generator=gen)
    pan = (base + 0.1 * torch.rand(shape, device=dev, generator=gen)).clamp(0, 1)
    return preds.to(dtype), ms.to(dtype), pan.to(dtype)


def paths(metric, args):
    def path(setting):
        def call():
            os.environ[SWITCH] = setting
            return metric(*args)
        return call
    return path("1"), path("0")


def kernels_per_call(fn):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_qnr needs a ROCm GPU"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    cases = []
    # the two flagship shapes for all three metrics; D_lambda alone at 2 and 3 bands (one and three pairs), where
    # the band-pair kernel saves the least
    plan = [(shape, dtype, tuple(METRICS)) for shape in ((4, 8, 1024, 1024), (16, 4, 512, 512))
            for dtype in (torch.float32, torch.bfloat16)]
    plan += [((16, c, 512, 512), torch.float32, ("d_lambda",)) for c in (2, 3)]
    for shape, dtype, names in plan:
        data = tensors(shape, 4, dtype, dev, gen)
        for name in names:
            fused, parent = paths(METRICS[name], data)
            label = f"{name} {'x'.join(map(str, shape))} ratio 4 {str(dtype)[6:]}"
            row = {"case": label, "fused_value": float(fused()), "parent_value": float(parent())}
            fused_t, parent_t = alternate([fused, parent])
            fused_ms, parent_ms = statistics.median(fused_t), statistics.median(parent_t)
            row.update(fused_ms=round(fused_ms, 4), parent_ms=round(parent_ms, 4),
                       speedup=round(parent_ms / fused_ms, 2),
                       fused_ms_minmax=[round(min(fused_t), 4), round(max(fused_t), 4)],
                       parent_ms_minmax=[round(min(parent_t), 4), round(max(parent_t), 4)])
            emit(row)
            if shape[0] == 4:  # the launch counts do not depend on the image size
                cases.append((label, fused, parent))
    for label, fused, parent in cases:
        emit({"case": label, "fused_kernels": kernels_per_call(fused), "parent_kernels": kernels_per_call(parent)})
    os.environ[SWITCH] = "1"


if __name__ == "__main__":
    main()
