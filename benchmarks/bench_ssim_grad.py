"""Forward + backward of ``1 - ssim`` and ``1 - ms_ssim`` as training losses: the fused kernel pair
(``csrc/image/ssim.hip`` forward, ``csrc/image/ssim_grad.hip`` backward) vs the pad / grouped-convolution formulation
under torch autograd, which is what every call that required a gradient ran before the backward kernel existed.

Same tensors, same process; the two paths alternate in timed windows of device events after a warm-up.  One JSON line
per case: median ms of a whole step (forward, ``backward()``) on both paths, their ratio, and the largest difference
between the two paths' gradients relative to the largest gradient.

Usage: ``python benchmarks/bench_ssim_grad.py [--out profiles/ssim_grad_bench.jsonl]``
"""
import argparse
import json
import os
import statistics
import sys
from unittest import mock

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


def case(metric, shape, dtype, both, dev, gen):
    t = torch.rand(shape, device=dev, generator=gen)
    p = (t + 0.1 * torch.randn(shape, device=dev, generator=gen)).clamp(0, 1).to(dtype).requires_grad_()
    t = t.to(dtype).requires_grad_(both)
    loss = S.structural_similarity_index_measure if metric == "ssim" else \
        S.multiscale_structural_similarity_index_measure

    def step():
        p.grad = t.grad = None
        (1 - loss(p, t, data_range=1.0)).backward()
        return p.grad, t.grad

    def fused():
        return step()

    def conv():  # the same public call with the differentiable kernels switched off: the convolution path
        with mock.patch.object(S, "_fused_grad_ok", lambda *a: False):
            return step()

    row = {"case": f"1 - {metric} fwd+bwd {'x'.join(map(str, shape))} {str(dtype)[6:]} grad "
                   f"{'preds+target' if both else 'preds'}"}
    try:
        gf, gc = fused()[0].double(), conv()[0].double()
        row["max_rel_grad_diff"] = float((gf - gc).abs().max() / gc.abs().max())
        fused_ms, conv_ms = alternate([fused, conv])
        row.update(fused_ms=round(fused_ms, 4), conv_ms=round(conv_ms, 4), speedup=round(conv_ms / fused_ms, 2))
    except RuntimeError as err:  # no convolution for this dtype: the kernels are still timed
        (fused_ms,) = alternate([fused])
        row.update(fused_ms=round(fused_ms, 4), conv_ms=None, conv_error=str(err).splitlines()[0][:120])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ssim_grad needs a ROCm GPU"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    for metric in ("ssim", "ms_ssim"):
        for dtype in (torch.float32, torch.bfloat16):
            for both in (False, True):
                line = json.dumps(case(metric, (16, 3, 512, 512), dtype, both, dev, gen))
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
