"""Forward + backward of ``1 - ssim`` and ``1 - ms_ssim`` on volumes as training losses: the fused kernels
(``csrc/image/ssim3d.hip`` forward, ``csrc/image/ssim3d_grad.hip`` backward) vs the pad / grouped-``conv3d``
formulation under torch autograd, which is what every 5-D call that required a gradient ran before the backward
kernels existed.

Same tensors, same process; the two paths alternate in timed windows of device events after a warm-up.  One JSON line
per case: median ms of a whole step (forward, ``backward()``) on both paths, their ratio, and the largest difference
between the two paths' gradients relative to the largest gradient.  MS-SSIM runs three scales (five do not fit an 11^3
window into 128^3).

Usage: ``python benchmarks/bench_ssim3d_grad.py [--out profiles/ssim3d_grad_bench.jsonl]``
"""
import argparse
import json
import os
import sys
from unittest import mock

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bench_ssim_grad import alternate  # noqa: E402
from torchmetrics_amd.functional.image import ssim as S  # noqa: E402

SHAPES = ((2, 1, 128, 128, 128), (1, 1, 160, 192, 160))
BETAS = (0.0448, 0.2856, 0.3001)


def case(metric, shape, dtype, both, dev, gen):
    t = torch.rand(shape, device=dev, generator=gen)
    p = (t + 0.1 * torch.randn(shape, device=dev, generator=gen)).clamp(0, 1).to(dtype).requires_grad_()
    t = t.to(dtype).requires_grad_(both)

    def step():
        p.grad = t.grad = None
        if metric == "ssim":
            val = S.structural_similarity_index_measure(p, t, data_range=1.0)
        else:
            val = S.multiscale_structural_similarity_index_measure(p, t, data_range=1.0, betas=BETAS)
        (1 - val).backward()
        return p.grad, t.grad

    def fused():
        return step()

    def conv():  # the same public call with the differentiable kernels switched off: the convolution path
        with mock.patch.object(S, "_fused3d_grad_ok", lambda *a: False):
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
    assert torch.cuda.is_available(), "bench_ssim3d_grad needs a ROCm GPU"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    for metric in ("ssim", "ms_ssim"):
        for shape in SHAPES:
            for dtype in (torch.float32, torch.bfloat16):
                for both in (False, True):
                    line = json.dumps(case(metric, shape, dtype, both, dev, gen))
                    print(line, flush=True)
                    if args.out:
                        with open(args.out, "a") as f:
                            f.write(line + "\n")


if __name__ == "__main__":
    main()
