"""3-D SSIM / MS-SSIM on the fused volume kernel (``csrc/image/ssim3d.hip``) vs an explicit fp64 window oracle.

The oracle evaluates every valid ``(kd, kh, kw)`` window with ``sliding_window_view`` and the outer-product weights
(no convolution), on the rounded 16-bit values upcast to fp64 where the inputs are fp16 / bf16.
"""
import functools
import math

import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import sliding_window_view

import torchmetrics_amd.functional as F
from torchmetrics_amd import image as I
from torchmetrics_amd import ops
from tests.helpers import assert_close, run_class_test

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
ATOL = 2e-5  # the 2-D SSIM tests' bound; the fp32 conv3d formulation is within 2e-6 of the oracle at these shapes


def _taps(sigma, gaussian=True, ks=11):
    out = []
    for s in sigma:
        k = int(3.5 * s + 0.5) * 2 + 1 if gaussian else ks
        g = np.exp(-0.5 * ((np.arange(k) - (k - 1) / 2) / s) ** 2) if gaussian else np.ones(k)
        out.append(g / g.sum())
    return out


def _oracle(p, t, taps, data_range=1.0):
    """(SSIM, CS) means over the valid windows of every ``[D, H, W]`` plane of fp64 ``[P, D, H, W]`` arrays."""
    dr = max(p.max() - p.min(), t.max() - t.min()) if data_range is None else data_range
    c1, c2 = (0.01 * dr) ** 2, (0.03 * dr) ** 2
    w3 = np.einsum("i,j,k->ijk", *taps)
    m = lambda a: np.einsum("pdhwijk,ijk->pdhw", sliding_window_view(a, w3.shape, axis=(1, 2, 3)), w3)  # noqa: E731
    mx, my, exx, eyy, exy = m(p), m(t), m(p * p), m(t * t), m(p * t)
    sxx, syy, sxy = np.maximum(exx - mx**2, 0), np.maximum(eyy - my**2, 0), exy - mx * my
    up, lo = 2 * sxy + c2, sxx + syy + c2
    ssim = ((2 * mx * my + c1) * up) / ((mx**2 + my**2 + c1) * lo)
    return np.stack([ssim.mean((1, 2, 3)), (up / lo).mean((1, 2, 3))], -1)


@functools.lru_cache(maxsize=None)
def _case(shape, sigma=(1.5, 1.5, 1.5), gaussian=True, dtype=torch.float32, data_range=1.0):
    """Seeded volumes in ``dtype``, the fp64 taps and the oracle's per-plane (SSIM, CS) means, computed once."""
    g = torch.Generator().manual_seed(0)
    t = torch.rand(shape, generator=g)
    p = (t + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1).to(dtype)
    t = t.to(dtype)
    taps = _taps(sigma, gaussian)
    return p, t, [torch.from_numpy(w) for w in taps], _oracle(p.double().numpy(), t.double().numpy(), taps, data_range)


RAGGED = (4, 29, 21, 77)  # output 19 x 11 x 67: ragged second tile on both in-plane axes, several planes


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize(("shape", "sigma", "gaussian", "chunk", "dtype"), [
    ((1, 11, 11, 11), (1.5, 1.5, 1.5), True, 0, torch.float32),  # volume == window: the ring completes exactly once
    (RAGGED, (1.5, 1.5, 1.5), True, 0, torch.float32),
    (RAGGED, (1.5, 1.5, 1.5), True, 1, torch.float32),  # one output slice per block
    (RAGGED, (1.5, 1.5, 1.5), True, 7, torch.float32),  # chunk < kd, not dividing 19
    ((2, 13, 20, 70), (0.5, 1.0, 1.5), True, 4, torch.float32),  # taps 5, 9, 11: any axis / tap mix-up, KD != 11
    ((2, 29, 21, 77), (1.5, 1.5, 1.5), False, 0, torch.float32),  # uniform 11^3
    ((2, 12, 19, 75), (1.5, 1.5, 1.5), True, 5, torch.float64),  # output depth 2 < chunk; fp64 accumulation
    ((2, 12, 19, 75), (1.5, 1.5, 1.5), True, 5, torch.float16),  # 16-bit loads at odd W
    ((2, 12, 19, 75), (1.5, 1.5, 1.5), True, 5, torch.bfloat16),
])
def test_ssim3d_partials_vs_window_oracle(device, shape, sigma, gaussian, chunk, dtype):
    p, t, taps, ref = _case(shape, sigma, gaussian, dtype)
    c12 = torch.tensor([1e-4, 9e-4, 0.0], dtype=torch.float64)
    part = ops.ssim3d_partials(p.to(device), t.to(device), *taps, c12, chunk)
    assert part.shape[0] == shape[0] and part.shape[2] == 2
    assert part.dtype == (torch.float64 if dtype == torch.float64 else torch.float32)
    n = math.prod(s - w.numel() + 1 for s, w in zip(shape[1:], taps))
    print("max |diff|", np.abs(part.sum(1).cpu().double().numpy() / n - ref).max())
    assert_close(part.sum(1) / n, ref, atol=ATOL)


def _count_calls(monkeypatch):
    calls, real = [], ops.ssim3d_partials
    monkeypatch.setattr(ops, "ssim3d_partials", lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize(("api", "data_range"), [("functional", 1.0), ("class", 1.0), ("functional", None)])
def test_ssim3d_public_path_reaches_kernel(monkeypatch, api, data_range):
    p, t, _, ref = _case(RAGGED, data_range=data_range)
    p, t, ref = p.reshape(2, 2, 29, 21, 77), t.reshape(2, 2, 29, 21, 77), ref.reshape(2, 2, 2).mean(1)
    calls = _count_calls(monkeypatch)
    if api == "functional":
        sim, cs = F.structural_similarity_index_measure(p.cuda(), t.cuda(), data_range=data_range, reduction="none",
                                                        return_contrast_sensitivity=True)
        assert_close(sim, ref[:, 0], atol=ATOL)
        assert_close(cs, ref[:, 1], atol=ATOL)
    else:
        run_class_test(p[None], t[None], I.StructuralSimilarityIndexMeasure, lambda a, b: ref[:, 0].mean(),
                       {"data_range": data_range}, atol=ATOL, device="cuda")
    assert calls


@pytest.mark.gpu
def test_ms_ssim3d_vs_window_oracle(monkeypatch):
    g = torch.Generator().manual_seed(3)
    t = torch.rand(1, 1, 48, 48, 48, generator=g)
    p = (t + 0.05 * torch.randn(t.shape, generator=g)).clamp(0, 1)
    betas, taps = (0.0448, 0.2856, 0.3001), _taps((0.5, 0.5, 0.5))
    pp, tt, css = p.double(), t.double(), []
    for _ in betas:
        s, c = _oracle(pp[:, 0].numpy(), tt[:, 0].numpy(), taps)[0]
        css.append(max(c, 0.0))
        pp, tt = torch.nn.functional.avg_pool3d(pp, 2), torch.nn.functional.avg_pool3d(tt, 2)
    css[-1] = max(s, 0.0)
    calls = _count_calls(monkeypatch)
    val = F.multiscale_structural_similarity_index_measure(p.cuda(), t.cuda(), kernel_size=5, sigma=0.5, betas=betas,
                                                           data_range=1.0)
    assert_close(val, np.prod(np.array(css) ** np.array(betas)), atol=ATOL)
    assert len(calls) == len(betas)


@pytest.mark.gpu
@pytest.mark.parametrize("why", ["depth_window_13", "requires_grad"])
def test_ssim3d_fallback_keeps_conv_path(monkeypatch, why):
    sigma = 1.8 if why == "depth_window_13" else 1.5
    p, t, _, ref = _case(RAGGED, (sigma,) * 3)
    p, t = p.reshape(2, 2, 29, 21, 77).cuda(), t.reshape(2, 2, 29, 21, 77).cuda()
    calls = _count_calls(monkeypatch)
    sim = F.structural_similarity_index_measure(p.requires_grad_(why == "requires_grad"), t, sigma=sigma,
                                                data_range=1.0, reduction="none")
    assert_close(sim, ref.reshape(2, 2, 2).mean(1)[:, 0], atol=ATOL)
    assert not calls
