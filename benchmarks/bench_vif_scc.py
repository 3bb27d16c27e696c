"""VIF and SCC: the fused prefilter-and-window kernels vs the dispatch they replace (same tensors, same process).

``visual_information_fidelity`` and ``spatial_correlation_coefficient`` through ``csrc/image/window_prefilter.hip``
against the same calls with ``TM_AMD_WINDOW_PREFILTER=0``, which restores the earlier dispatch: vendor convolutions
around the SSIM window kernel for fp32, the torch composition in the 16-bit type for bf16.  The switch is read at call
time, so the two paths alternate in timed windows of device events after a warm-up of both; one JSON line per case:
median ms of both (and the spread of the per-round values), their ratio, and both paths' values.

Usage: ``python benchmarks/bench_vif_scc.py [--out profiles/vif_scc_bench.jsonl]``
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchmetrics_amd.functional.image import spatial_correlation_coefficient  # noqa: E402
from torchmetrics_amd.functional.image import visual_information_fidelity  # noqa: E402

ROUNDS = 5
WINDOW_MS = 100.0  # per path and round: >= 500 ms of timed work per path
SWITCH = "TM_AMD_WINDOW_PREFILTER"


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


def case(name, metric, shape, dtype, dev, gen):
    t = torch.rand(shape, device=dev, generator=gen)
    p = (t + 0.1 * torch.randn(shape, device=dev, generator=gen)).clamp(0, 1).to(dtype)
    t = t.to(dtype)

    def path(setting):
        def call():
            os.environ[SWITCH] = setting
            return metric(p, t)
        return call

    fused, parent = path("1"), path("0")
    row = {"case": f"{name} {'x'.join(map(str, shape))} {str(dtype)[6:]}",
           "fused_value": float(fused()), "parent_value": float(parent())}
    fused_t, parent_t = alternate([fused, parent])
    os.environ[SWITCH] = "1"
    fused_ms, parent_ms = statistics.median(fused_t), statistics.median(parent_t)
    row.update(fused_ms=round(fused_ms, 4), parent_ms=round(parent_ms, 4), speedup=round(parent_ms / fused_ms, 2),
               fused_ms_minmax=[round(min(fused_t), 4), round(max(fused_t), 4)],
               parent_ms_minmax=[round(min(parent_t), 4), round(max(parent_t), 4)])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vif_scc needs a ROCm GPU"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    shape = (16, 3, 512, 512)
    cases = [("vif", visual_information_fidelity, torch.float32), ("vif", visual_information_fidelity, torch.bfloat16),
             ("scc window 8", lambda p, t: spatial_correlation_coefficient(p, t, window_size=8), torch.float32)]
    for name, metric, dtype in cases:
        line = json.dumps(case(name, metric, shape, dtype, dev, gen))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
