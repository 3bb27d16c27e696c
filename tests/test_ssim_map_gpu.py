"""SSIM full-image maps and UQI maps on the fused map kernels (``csrc/image/ssim_map.hip``) vs an explicit fp64 window
oracle: ``np.pad(mode="reflect")`` by the half windows, ``sliding_window_view`` and the outer-product weights (no
convolution), on the rounded 16-bit values upcast to fp64 where the inputs are fp16 / bf16.

Per-pixel bound: ten times ``conv``, the pad / grouped-convolution formulation's own worst per-pixel error against this
oracle on the same case (measured on the CPU in fp32, it stands beside each case below), and no less than 2e-5; 16-bit
maps add half an ulp of the dtype at 1.0 for the one rounding at the store.  Scores keep the SSIM tests' 2e-5.
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
from torchmetrics_amd.functional.image import ssim as S

pytestmark = pytest.mark.gpu
ATOL = 2e-5
HALF_ULP = {torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}
F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
UQI_EPS = float(torch.finfo(torch.float32).eps)


def _bound(dtype, conv):
    return max(10 * conv, ATOL) + HALF_ULP.get(dtype, 0.0)


def _oracle(p, t, taps, c12, uqi, reflect):
    """fp64 ``[P, *spatial]`` arrays -> (map, per-plane mean over the windows that lie fully inside the input)."""
    half = [w.size // 2 for w in taps]
    if reflect:
        p, t = (np.pad(a, [(0, 0)] + [(h, h) for h in half], mode="reflect") for a in (p, t))
    wn, sub = functools.reduce(np.multiply.outer, taps), "ijk"[:len(taps)]
    m = lambda a: np.einsum(f"...{sub},{sub}->...",  # noqa: E731
                            sliding_window_view(a, wn.shape, axis=tuple(range(1, a.ndim))), wn)
    mx, my, exx, eyy, exy = m(p), m(t), m(p * p), m(t * t), m(p * t)
    sxx, syy, sxy = np.maximum(exx - mx**2, 0), np.maximum(eyy - my**2, 0), exy - mx * my
    c1, c2, eps = c12
    if uqi:
        full = (2 * mx * my * 2 * sxy) / ((mx**2 + my**2) * (sxx + syy) + eps)
    else:
        full = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx**2 + my**2 + c1) * (sxx + syy + c2))
    inner = full[(slice(None), *(slice(h, -h if h else None) for h in half))] if reflect else full
    return full, inner.reshape(len(full), -1).mean(1)


@functools.lru_cache(maxsize=None)
def _case(shape, sigma, gaussian=True, dtype=F32, c12=(1e-4, 9e-4, 0.0), uqi=False, reflect=True):
    """Seeded planes in ``dtype``, the fp64 taps and the oracle's (map, per-plane score), computed once."""
    g = torch.Generator().manual_seed(0)
    t = torch.rand(shape, generator=g)
    p = (t + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1).to(dtype)
    t = t.to(dtype)
    taps = []
    for s in sigma:
        k = int(3.5 * s + 0.5) * 2 + 1 if gaussian else 11
        w = np.exp(-0.5 * ((np.arange(k) - (k - 1) / 2) / s) ** 2) if gaussian else np.ones(k)
        taps.append(w / w.sum())
    full, score = _oracle(p.double().numpy(), t.double().numpy(), taps, c12, uqi, reflect)
    return p, t, [torch.from_numpy(w) for w in taps], full, score


def _check(name, full, part, ref_full, ref_score, n, dtype, conv):
    err = float(np.abs(full.double().cpu().numpy() - ref_full).max())
    score = part[..., 0].sum(1).double().cpu().numpy() / n
    print(f"{name}: map max |diff| {err:.3g} (bound {_bound(dtype, conv):.3g}), "
          f"score max |diff| {np.abs(score - ref_score).max():.3g}")
    assert full.dtype == dtype and tuple(full.shape) == ref_full.shape
    assert err <= _bound(dtype, conv)
    np.testing.assert_allclose(score, ref_score, atol=ATOL, rtol=0)


@pytest.mark.parametrize(("shape", "sigma", "gaussian", "dtype", "uqi", "reflect", "conv"), [
    ((1, 11, 11), (1.5, 1.5), True, F32, False, True, 2.70e-6),  # image == window: every halo reflects on both sides
    ((4, 29, 77), (1.5, 1.5), True, F32, False, True, 4.97e-6),  # ragged tiles on both axes, several planes
    ((2, 20, 70), (1.0, 1.5), True, F32, False, True, 4.69e-6),  # taps 9 x 11: any axis mix-up
    ((2, 29, 77), (1.5, 1.5), False, F32, False, True, 3.46e-6),  # uniform 11 x 11
    ((2, 19, 75), (1.5, 1.5), True, F64, False, True, 0.0),
    ((2, 19, 75), (1.5, 1.5), True, F16, False, True, 0.0),  # odd width: 16-bit vector loads and stores
    ((2, 19, 75), (1.5, 1.5), True, BF16, False, True, 0.0),
    ((4, 29, 77), (1.5, 1.5), True, F32, True, False, 4.21e-6),  # UQI, valid windows only
    ((1, 40, 70), (4.5, 4.5), True, F32, False, True, 8.52e-6),  # window 33: the limit, LDS above the default 64 KB
    ((1, 40, 70), (4.5, 4.5), True, F64, False, True, 0.0),  # fp64 over window 23: the 4-row tile
])
def test_ssim2d_map_vs_window_oracle(shape, sigma, gaussian, dtype, uqi, reflect, conv):
    c12 = (0.0, 0.0, UQI_EPS) if uqi else (1e-4, 9e-4, 0.0)
    p, t, taps, ref_full, ref_score = _case(shape, sigma, gaussian, dtype, c12, uqi, reflect)
    full, part = ops.ssim2d_map(p.cuda(), t.cuda(), *taps, torch.tensor(c12, dtype=torch.float64),
                                ops.UQI_MODE if uqi else ops.SSIM_MODE, reflect)
    n = math.prod(s - w.numel() + 1 for s, w in zip(shape[1:], taps))
    _check("ssim2d_map", full, part, ref_full, ref_score, n, dtype, conv)


VOL = (2, 29, 21, 77)  # ragged tiles on both in-plane axes, depth not a multiple of any chunk below


@pytest.mark.parametrize(("shape", "sigma", "gaussian", "chunk", "dtype", "conv"), [
    ((1, 11, 11, 11), (1.5, 1.5, 1.5), True, 0, F32, 1.12e-5),  # volume == window: every halo reflects on both sides
    (VOL, (1.5, 1.5, 1.5), True, 0, F32, 1.75e-5),
    (VOL, (1.5, 1.5, 1.5), True, 1, F32, 1.75e-5),  # one output slice per block
    (VOL, (1.5, 1.5, 1.5), True, 7, F32, 1.75e-5),  # chunk < kd, not dividing 29
    ((2, 13, 20, 70), (0.5, 1.0, 1.5), True, 4, F32, 1.18e-5),  # taps 5, 9, 11: any axis / tap mix-up, KD != 11
    (VOL, (1.5, 1.5, 1.5), False, 0, F32, 1.66e-5),  # uniform 11^3
    ((2, 12, 19, 75), (1.5, 1.5, 1.5), True, 5, F64, 0.0),
    ((2, 12, 19, 75), (1.5, 1.5, 1.5), True, 5, F16, 0.0),  # 16-bit loads and stores at odd W
    ((2, 12, 19, 75), (1.5, 1.5, 1.5), True, 5, BF16, 0.0),
])
def test_ssim3d_map_vs_window_oracle(shape, sigma, gaussian, chunk, dtype, conv):
    p, t, taps, ref_full, ref_score = _case(shape, sigma, gaussian, dtype)
    args = (p.cuda(), t.cuda(), *taps, torch.tensor([1e-4, 9e-4, 0.0], dtype=torch.float64), chunk)
    full, part = ops.ssim3d_map(*args)
    n = math.prod(s - w.numel() + 1 for s, w in zip(shape[1:], taps))
    _check(f"ssim3d_map chunk {chunk}", full, part, ref_full, ref_score, n, dtype, conv)
    again = ops.ssim3d_map(*args)
    assert torch.equal(again[0], full) and torch.equal(again[1], part)


def _count_calls(monkeypatch):
    calls = {}
    for mod, name in ((ops, "ssim2d_map"), (ops, "ssim3d_map"), (S, "_ssim_update_conv")):
        real = getattr(mod, name)
        monkeypatch.setattr(mod, name, lambda *a, _n=name, _r=real, **k: calls.update({_n: 1}) or _r(*a, **k))
    return calls


@pytest.mark.parametrize("data_range", [1.0, None])
@pytest.mark.parametrize("api", ["functional", "class"])
@pytest.mark.parametrize(("shape", "conv"), [((4, 29, 77), 4.97e-6), (VOL, 1.75e-5)])
def test_ssim_full_image_public_path_reaches_kernel(monkeypatch, shape, conv, api, data_range):
    p, t = _case(shape, (1.5,) * (len(shape) - 1))[:2]
    dr = 1.0 if data_range else float(max(p.max() - p.min(), t.max() - t.min()))
    ref_full, ref_score = _case(shape, (1.5,) * (len(shape) - 1), c12=((0.01 * dr) ** 2, (0.03 * dr) ** 2, 0.0))[3:]
    bc = (shape[0] // 2, 2, *shape[1:])
    p, t = p.reshape(bc).cuda(), t.reshape(bc).cuda()
    calls = _count_calls(monkeypatch)
    if api == "functional":
        sim, full = F.structural_similarity_index_measure(p, t, data_range=data_range, reduction="none",
                                                          return_full_image=True)
    else:
        metric = I.StructuralSimilarityIndexMeasure(data_range=data_range, reduction="none",
                                                    return_full_image=True).to("cuda")
        metric.update(p, t)
        sim, full = metric.compute()
    assert list(calls) == ["ssim2d_map" if len(shape) == 3 else "ssim3d_map"]
    assert full.shape == p.shape and full.dtype == p.dtype and sim.dtype == p.dtype
    err = float(np.abs(full.double().cpu().numpy() - ref_full.reshape(bc)).max())
    print(f"public {len(bc)}-D {api} data_range={data_range}: map max |diff| {err:.3g}")
    assert err <= _bound(F32, conv)
    np.testing.assert_allclose(sim.double().cpu().numpy(), ref_score.reshape(bc[:2]).mean(1), atol=ATOL, rtol=0)


def test_uqi_map_public_path_reaches_kernel(monkeypatch):
    p, t, _, ref_full, _ = _case((4, 29, 77), (1.5, 1.5), c12=(0.0, 0.0, UQI_EPS), uqi=True, reflect=False)
    p, t = p.reshape(2, 2, 29, 77), t.reshape(2, 2, 29, 77)
    calls = _count_calls(monkeypatch)
    full = F.universal_image_quality_index(p.cuda(), t.cuda(), reduction="none")
    assert list(calls) == ["ssim2d_map"]
    assert full.shape == S._uqi_map(p, t, (11, 11), (1.5, 1.5), UQI_EPS).shape and full.dtype == p.dtype
    assert float(np.abs(full.double().cpu().numpy() - ref_full.reshape(full.shape)).max()) <= _bound(F32, 4.21e-6)


@pytest.mark.parametrize(("why", "conv"), [("requires_grad", 4.97e-6), ("window_37", 1.18e-5)])
def test_ssim_full_image_fallback_keeps_conv_path(monkeypatch, why, conv):
    shape, sigma = ((4, 29, 77), 1.5) if why == "requires_grad" else ((2, 40, 70), 5.0)
    p, t, _, ref_full, ref_score = _case(shape, (sigma, sigma))
    bc = (shape[0] // 2, 2, *shape[1:])
    p, t = p.reshape(bc).cuda().requires_grad_(why == "requires_grad"), t.reshape(bc).cuda()
    calls = _count_calls(monkeypatch)
    sim, full = F.structural_similarity_index_measure(p, t, sigma=sigma, data_range=1.0, reduction="none",
                                                      return_full_image=True)
    assert list(calls) == ["_ssim_update_conv"]
    assert float(np.abs(full.detach().double().cpu().numpy() - ref_full.reshape(bc)).max()) <= _bound(F32, conv)
    np.testing.assert_allclose(sim.detach().double().cpu().numpy(), ref_score.reshape(bc[:2]).mean(1), atol=ATOL,
                               rtol=0)
    if why == "requires_grad":
        full.sum().backward()
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
