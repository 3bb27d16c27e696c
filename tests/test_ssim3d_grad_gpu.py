"""Differentiable 3-D SSIM / MS-SSIM on the fused backward kernels (``csrc/image/ssim3d_grad.hip``) vs torch autograd
through a plain separable fp64 window filter on the CPU (``unfold`` times the taps, axis by axis, no convolution), on
the rounded 16-bit values upcast to fp64 where the inputs are fp16 / bf16.

Gradients of a mean scale with 1 / n, so every comparison is ``max|diff| / max|oracle grad|`` over the tensor.
"""
import functools

import pytest
import torch

import torchmetrics_amd.functional as F
from torchmetrics_amd import image as I
from torchmetrics_amd import ops
from torchmetrics_amd.functional.image.helper import _window_1d

pytestmark = pytest.mark.gpu
EPS16 = {torch.float16: torch.finfo(torch.float16).eps, torch.bfloat16: torch.finfo(torch.bfloat16).eps}


def _taps(sigma, gaussian=True, ks=11):
    out = []
    for s in sigma:
        k = int(3.5 * s + 0.5) * 2 + 1 if gaussian else ks
        g = torch.exp(-0.5 * ((torch.arange(k, dtype=torch.float64) - (k - 1) / 2) / s) ** 2) if gaussian else \
            torch.ones(k, dtype=torch.float64)
        out.append(g / g.sum())
    return out


def _oracle(x, y, taps, c1, c2):
    """Per-volume (sum SSIM, sum CS) over the valid windows of fp64 ``[P, D, H, W]`` tensors, ``[P, 2]``."""
    def m(a):
        for axis, w in zip((1, 2, 3), taps):
            a = (a.unfold(axis, w.numel(), 1) * w).sum(-1)
        return a

    mx, my, exx, eyy, exy = m(x), m(y), m(x * x), m(y * y), m(x * y)
    sxx, syy, sxy = torch.clamp(exx - mx**2, min=0), torch.clamp(eyy - my**2, min=0), exy - mx * my
    up, lo = 2 * sxy + c2, sxx + syy + c2
    ssim = ((2 * mx * my + c1) * up) / ((mx**2 + my**2 + c1) * lo)
    return torch.stack([ssim.sum((1, 2, 3)), (up / lo).sum((1, 2, 3))], -1)


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(shape, generator=g)
    p = (t + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1).to(dtype)
    return p, t.to(dtype), 0.5 + torch.rand(*shape[:-3], 2, generator=g, dtype=torch.float64)


def _err(ours, ref, dtype=torch.float32):
    ref = ref.to(dtype).double() if dtype in EPS16 else ref  # 16-bit: the oracle gradient rounded to the dtype
    return float((ours.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def _bound(dtype, conv=None):
    """fp32: ten times ``conv``, the convolution formulation's own fp32 autograd error against this oracle, and no
    less than 2e-5.  ``conv`` was measured on the CPU for every fp32 case and stands beside it below.  fp64: 1e-10.
    16-bit: one eps of the dtype (the output rounding plus the fp32 accumulation slack)."""
    return {torch.float32: 10 * max(conv or 0.0, 2e-6), torch.float64: 1e-10}.get(dtype) or EPS16[dtype]


RAGGED = (2, 29, 21, 77)  # windows 19 x 11 x 67, voxel tiles 3 x 2: ragged second tile on both axes of both launches


@pytest.mark.parametrize(("shape", "sigma", "gaussian", "chunk", "dtype", "conv"), [  # conv: larger of its gx / gy errors
    ((1, 11, 11, 11), (1.5, 1.5, 1.5), True, 0, torch.float32, 3.89e-5),  # volume == window: one tap per voxel, flush
    (RAGGED, (1.5, 1.5, 1.5), True, 0, torch.float32, 5.95e-6),
    (RAGGED, (1.5, 1.5, 1.5), True, 1, torch.float32, 5.95e-6),  # one slice per block
    (RAGGED, (1.5, 1.5, 1.5), True, 7, torch.float32, 5.95e-6),  # chunk < kd, dividing neither 19 nor 29
    ((2, 13, 20, 70), (0.5, 1.0, 1.5), True, 4, torch.float32, 4.26e-6),  # taps 5, 9, 11: axis / tap order; KD != 11
    (RAGGED, (1.5, 1.5, 1.5), False, 0, torch.float32, 5.62e-6),  # uniform 11^3
    ((2, 12, 19, 75), (1.5, 1.5, 1.5), True, 5, torch.float64, None),  # window depth 2 < chunk
    ((2, 12, 19, 75), (1.5, 1.5, 1.5), True, 5, torch.float16, None),  # odd width: 16-bit loads and stores
    ((2, 12, 19, 75), (1.5, 1.5, 1.5), True, 5, torch.bfloat16, None),
])
def test_ssim3d_backward_vs_window_oracle(shape, sigma, gaussian, chunk, dtype, conv):
    x, y, g = _inputs(shape, dtype)
    taps = _taps(sigma, gaussian)
    x64, y64 = (v.to(torch.float64, copy=True).requires_grad_() for v in (x, y))
    c12 = torch.tensor([1e-4, 9e-4, 0.0], dtype=torch.float64, requires_grad=True)
    (_oracle(x64, y64, taps, c12[0], c12[1]) * g).sum().backward()
    gx, gy, gc = ops.ssim3d_backward(x.cuda(), y.cuda(), *taps, c12.detach(), g, True, True, chunk)
    assert gx.dtype == dtype and gy.dtype == dtype and gx.shape == x.shape and gy.shape == y.shape
    assert gc.dtype == (torch.float64 if dtype == torch.float64 else torch.float32)
    assert gc.shape[0] == shape[0] and gc.shape[2] == 2
    dc = gc.sum((0, 1)).cpu().double()
    errs = {"gx": _err(gx, x64.grad, dtype), "gy": _err(gy, y64.grad, dtype),
            "dc1": float(abs(dc[0] - c12.grad[0]) / abs(c12.grad[0])),
            "dc2": float(abs(dc[1] - c12.grad[1]) / abs(c12.grad[1]))}
    print(errs)
    assert max(errs.values()) <= _bound(dtype, conv), errs
    if shape == RAGGED and gaussian and chunk == 0:
        gx3, gy3, gc3 = ops.ssim3d_backward(x.cuda(), y.cuda(), *taps, c12.detach(), g, False, False, chunk)
        assert gy3 is None and gc3 is None and torch.equal(gx3, gx)  # grad_x alone: the 3-map variant, same values
        again = ops.ssim3d_backward(x.cuda(), y.cuda(), *taps, c12.detach(), g, True, True, chunk)
        assert all(torch.equal(a, b) for a, b in zip(again, (gx, gy, gc)))  # fixed order, no atomics


def _public_oracle(p, t, data_range, wsim, wcs):
    """Weighted sum of the per-volume SSIM and CS means of fp64 ``[B, C, D, H, W]`` inputs, differentiable."""
    dr = torch.maximum(p.max() - p.min(), t.max() - t.min()) if data_range is None else data_range
    sums = _oracle(p.flatten(0, 1), t.flatten(0, 1), _taps((1.5, 1.5, 1.5)), (0.01 * dr) ** 2, (0.03 * dr) ** 2)
    n = p.shape[1] * (p.shape[2] - 10) * (p.shape[3] - 10) * (p.shape[4] - 10)
    means = sums.reshape(p.shape[0], p.shape[1], 2).sum(1) / n
    return (means[:, 0] * wsim).sum() + (means[:, 1] * wcs).sum()


def _ms_oracle(p, t, betas):
    taps, vals = _taps((0.5, 0.5, 0.5)), []
    for _ in betas:
        s = _oracle(p[:, 0], t[:, 0], taps, 1e-4, 9e-4)[0] / ((p.shape[-3] - 4) * (p.shape[-2] - 4) * (p.shape[-1] - 4))
        vals.append(torch.relu(s))
        p, t = torch.nn.functional.avg_pool3d(p, 2), torch.nn.functional.avg_pool3d(t, 2)
    vals = [v[1] for v in vals[:-1]] + [vals[-1][0]]
    return torch.prod(torch.stack(vals) ** torch.tensor(betas, dtype=torch.float64))


@pytest.mark.parametrize(("case", "conv"), [  # conv: the convolution path's error on the same call, CPU fp32
    ("range_1", 7.08e-6), ("range_none", 7.08e-6), ("target_grad", 6.46e-6), ("class", 6.00e-6),
    ("ms_ssim", 1.23e-4),  # 5-tap sigma 0.5 windows down to 12^3, relu and pow between the scales
])
def test_ssim3d_grad_public_path_reaches_backward_kernels(monkeypatch, case, conv):
    calls, real = [], ops.ssim3d_backward
    monkeypatch.setattr(ops, "ssim3d_backward", lambda *a, **k: calls.append(1) or real(*a, **k))
    shape = (1, 1, 48, 48, 48) if case == "ms_ssim" else (2, 2, 29, 21, 77)
    p, t, w = _inputs(shape, seed=3)
    w = w[:, 0]  # [B, 2]: a weight per volume on its SSIM and on its CS
    p64, t64 = p.double().requires_grad_(), t.double().requires_grad_()
    pg, tg = p.cuda().requires_grad_(case != "target_grad"), t.cuda().requires_grad_(case == "target_grad")
    if case == "ms_ssim":
        betas = (0.0448, 0.2856, 0.3001)
        _ms_oracle(p64, t64, betas).backward()
        F.multiscale_structural_similarity_index_measure(pg, tg, kernel_size=5, sigma=0.5, betas=betas,
                                                         data_range=1.0).backward()
    elif case == "class":
        _public_oracle(p64, t64, 1.0, torch.full((2,), 0.5, dtype=torch.float64), 0.0).backward()
        I.StructuralSimilarityIndexMeasure(data_range=1.0).cuda()(pg, tg).backward()
    else:
        dr = None if case == "range_none" else 1.0
        _public_oracle(p64, t64, dr, w[:, 0], w[:, 1]).backward()
        sim, cs = F.structural_similarity_index_measure(pg, tg, data_range=dr, reduction="none",
                                                        return_contrast_sensitivity=True)
        (sim * w[:, 0].cuda() + cs * w[:, 1].cuda()).sum().backward()
    if case == "target_grad":  # the target alone requires a gradient
        assert pg.grad is None
        errs = {"target": _err(tg.grad, t64.grad)}
    else:
        errs = {"preds": _err(pg.grad, p64.grad)}
    print(errs)
    assert max(errs.values()) <= _bound(torch.float32, conv), errs
    assert len(calls) == (3 if case == "ms_ssim" else 1)


def test_ssim3d_without_grad_keeps_forward_kernel(monkeypatch):
    p, t, _ = _inputs((2, 2, 29, 21, 77), seed=3)
    p, t = p.cuda(), t.cuda()
    taps = _window_1d([11, 11, 11], [1.5, 1.5, 1.5], True, p.dtype, p.device)  # the public path's own taps, constants
    c12 = torch.tensor([(0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2, 0.0])
    part = ops.ssim3d_partials(p.reshape(4, 29, 21, 77), t.reshape(4, 29, 21, 77), *taps, c12)
    monkeypatch.setattr(ops, "ssim3d_sums_grad", None)  # any call would raise
    monkeypatch.setattr(ops, "ssim3d_backward", None)
    sim, cs = F.structural_similarity_index_measure(p, t, data_range=1.0, reduction="none",
                                                    return_contrast_sensitivity=True)
    ref = part.sum(1).reshape(2, 2, 2).sum(1) / (2 * 19 * 11 * 67)
    assert torch.equal(sim, ref[:, 0]) and torch.equal(cs, ref[:, 1])
