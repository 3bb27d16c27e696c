"""SSIM window kernels vs the pad / grouped-convolution formulation they replace (same tensors, same process).

Volumes: ``structural_similarity_index_measure`` on 5-D inputs (``csrc/image/ssim3d.hip``) against ``_ssim_update_conv``
called directly, which is what every 5-D call ran before the volume kernel existed.  One 2-D row
(``csrc/image/ssim.hip``) gives the family a record.  The two paths alternate in timed windows of device events; one
JSON line per case: median ms of both, their ratio, achieved bytes/s of the fused path over the bytes the algorithm
must read (both inputs once), and the largest difference between the two paths' per-image values.

Usage: ``python benchmarks/bench_ssim3d.py [--out profiles/ssim3d_bench.jsonl]``
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchmetrics_amd.functional.image import ssim as S  # noqa: E402

ROUNDS = 5
WINDOW_MS = 100.0  # per path and round: >= 500 ms of timed work per path


def window_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def alternate(fns):
    """Median per-call ms of every fn, timed in alternating windows after a warm-up."""
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
    return [statistics.median(t) for t in times]


def case(shape, dtype, dev, gen):
    t = torch.rand(shape, device=dev, generator=gen)
    p = (t + 0.1 * torch.randn(shape, device=dev, generator=gen)).clamp(0, 1).to(dtype)
    t = t.to(dtype)
    nd = len(shape) - 2
    ks, sg = nd * [11], nd * [1.5]

    def fused():
        return S.structural_similarity_index_measure(p, t, data_range=1.0, reduction="none")

    def conv():
        pc, tc, c1, c2 = S._data_range_consts(p, t, 1.0, 0.01, 0.03)
        return S._ssim_update_conv(pc, tc, True, ks, sg, ks, c1, c2, False, False)

    row = {"case": f"ssim{nd}d {'x'.join(map(str, shape))} {str(dtype)[6:]} window 11"}
    try:
        diff = float((fused().double() - conv().double()).abs().max())
        fused_ms, conv_ms = alternate([fused, conv])
        row.update(fused_ms=round(fused_ms, 4), conv_ms=round(conv_ms, 4), speedup=round(conv_ms / fused_ms, 2),
                   max_abs_diff=diff)
    except RuntimeError as err:  # the convolution formulation may be unavailable for a dtype; the kernel is still timed
        (fused_ms,) = alternate([fused])
        row.update(fused_ms=round(fused_ms, 4), conv_ms=None, conv_error=str(err).splitlines()[0][:120])
    row["fused_GBps"] = round(2 * p.numel() * p.element_size() / fused_ms / 1e6, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ssim3d needs a ROCm GPU"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    cases = [((2, 1, 128, 128, 128), torch.float32), ((2, 1, 128, 128, 128), torch.bfloat16),
             ((1, 1, 160, 192, 160), torch.float32), ((1, 1, 160, 192, 160), torch.bfloat16),
             ((16, 3, 512, 512), torch.float32)]
    for shape, dtype in cases:
        line = json.dumps(case(shape, dtype, dev, gen))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
