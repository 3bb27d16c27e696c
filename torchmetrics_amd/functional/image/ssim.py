"""SSIM, MS-SSIM and UQI (reference ``F/image/ssim.py:26-528``, ``F/image/uqi.py``).

The per-image scores run through the fused HIP window kernels on ROCm (``csrc/image/ssim.hip`` for 2-D images,
``csrc/image/ssim3d.hip`` for 3-D volumes): they evaluate the valid windows straight from the unpadded inputs (the
reference's reflect-pad + crop yields exactly those windows).  2-D SSIM / MS-SSIM of ROCm inputs that require a
gradient (``1 - ssim`` as a training loss) stay on that kernel and take their backward from its transposed twin,
``csrc/image/ssim_grad.hip``, for windows up to 15; 3-D volumes that require one likewise keep the volume kernel and
take their backward from the two launches of ``csrc/image/ssim3d_grad.hip`` (in-plane windows up to 15, depth windows
up to 11).  ``return_full_image`` maps of ROCm images and volumes, and ``reduction='none'`` UQI maps, come from the
map kernels of ``csrc/image/ssim_map.hip``, which mirror the borders while they stage a tile and give the per-image
score from the same launch.  The explicit pad / grouped-convolution formulation below is kept for what the kernels do
not cover: depth windows over 11, in-plane windows over 33 (over 15 with a gradient), maps that require a gradient, and
autograd on the CPU and of UQI.
"""
import math
from typing import List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F  # noqa: N812
from torch import Tensor
from typing_extensions import Literal

from torchmetrics_amd import ops
from torchmetrics_amd.functional.image.helper import (
    _gaussian_kernel_2d,
    _gaussian_kernel_3d,
    _reflection_pad_3d,
    _window_1d,
)
from torchmetrics_amd.utilities.checks import _check_same_shape
from torchmetrics_amd.utilities.distributed import reduce

_Reduction = Literal["elementwise_mean", "sum", "none", None]


def _ssim_check_inputs(preds: Tensor, target: Tensor) -> Tuple[Tensor, Tensor]:
    if preds.dtype != target.dtype:
        target = target.to(preds.dtype)
    _check_same_shape(preds, target)
    if len(preds.shape) not in (4, 5):
        raise ValueError(
            "Expected `preds` and `target` to have BxCxHxW or BxCxDxHxW shape."
            f" Got preds: {preds.shape} and target: {target.shape}."
        )
    return preds, target


def _normalise_args(preds: Tensor, kernel_size, sigma) -> Tuple[List[int], List[float]]:
    nd = preds.ndim - 2
    ks = list(kernel_size) if isinstance(kernel_size, Sequence) else nd * [kernel_size]
    sg = list(sigma) if isinstance(sigma, Sequence) else nd * [sigma]
    if len(ks) != nd or len(ks) not in (2, 3):
        raise ValueError(
            f"`kernel_size` has dimension {len(ks)}, but expected to be two less that target dimensionality,"
            f" which is: {preds.ndim}"
        )
    if len(sg) != nd or len(sg) not in (2, 3):
        raise ValueError(
            f"`kernel_size` has dimension {len(ks)}, but expected to be two less that target dimensionality,"
            f" which is: {preds.ndim}"
        )
    if any(x % 2 == 0 or x <= 0 for x in ks):
        raise ValueError(f"Expected `kernel_size` to have odd positive number. Got {ks}.")
    if any(y <= 0 for y in sg):
        raise ValueError(f"Expected `sigma` to have positive number. Got {sg}.")
    return ks, sg


def _data_range_consts(preds: Tensor, target: Tensor, data_range, k1: float, k2: float):
    """Clamp for a (min, max) range and return (preds, target, c1, c2) -- c1/c2 may be device scalars (no sync)."""
    if data_range is None:
        dr = torch.maximum(preds.max() - preds.min(), target.max() - target.min())
    elif isinstance(data_range, tuple):
        preds = torch.clamp(preds, min=data_range[0], max=data_range[1])
        target = torch.clamp(target, min=data_range[0], max=data_range[1])
        dr = data_range[1] - data_range[0]
    else:
        dr = data_range
    return preds, target, (k1 * dr) ** 2, (k2 * dr) ** 2


def _window_fits(preds: Tensor, ks: Sequence[int], gauss_ks: Sequence[int], limit: int) -> bool:
    return (
        preds.ndim == 4
        and max(ks) <= limit
        and max(gauss_ks) <= limit
        and preds.shape[-2] >= max(ks[0], gauss_ks[0])
        and preds.shape[-1] >= max(ks[1], gauss_ks[1])
    )


def _fused_ok(preds: Tensor, ks: Sequence[int], gauss_ks: Sequence[int]) -> bool:
    """The forward-only window kernel applies (SSIM, UQI, SCC, VIF): no gradient wanted, windows up to 33."""
    return not (preds.requires_grad and torch.is_grad_enabled()) and _window_fits(preds, ks, gauss_ks, 33)


def _wants_grad(preds: Tensor, target: Tensor) -> bool:
    return torch.is_grad_enabled() and (preds.requires_grad or target.requires_grad)


def _fused_grad_ok(preds: Tensor, target: Tensor, ks: Sequence[int], gauss_ks: Sequence[int]) -> bool:
    """The differentiable kernel pair applies (SSIM only): ROCm, a gradient wanted, windows up to 15."""
    return (
        preds.is_cuda
        and _wants_grad(preds, target)
        and _window_fits(preds, ks, gauss_ks, ops.SSIM_GRAD_MAX_WINDOW)
        and preds.shape[0] * preds.shape[1] <= 65535
    )


def _fused_means(preds: Tensor, target: Tensor, wh: Tensor, ww: Tensor, c1, c2, eps: float, mode: int,
                 grad: bool = False):
    """Per-image mean (over channels and valid windows) of the SSIM/UQI map and of the contrast sensitivity;
    ``grad``: through the differentiable kernel pair (SSIM mode, ROCm)."""
    b, c, h, w = preds.shape
    acc = torch.float64 if preds.dtype == torch.float64 else torch.float32
    consts = torch.stack([torch.as_tensor(v, dtype=acc, device=preds.device) for v in (c1, c2, eps)])
    n = c * (h - wh.numel() + 1) * (w - ww.numel() + 1)
    if grad:  # consts keeps the graph of a data_range=None c1 / c2 (as_tensor and stack are differentiable)
        sums = ops.ssim2d_sums_grad(preds.reshape(b * c, h, w), target.reshape(b * c, h, w), wh, ww, consts)
        sums = sums.reshape(b, c, 2).sum(1) / n
        return sums[:, 0].to(preds.dtype), sums[:, 1].to(preds.dtype)
    part = ops.ssim2d_partials(preds.reshape(b * c, h, w), target.reshape(b * c, h, w), wh, ww, consts, mode)
    sums = part.sum(1).reshape(b, c, 2).sum(1) / n
    return sums[:, 0].to(preds.dtype), sums[:, 1].to(preds.dtype)


def _window3d_fits(preds: Tensor, ks: Sequence[int], gauss_ks: Sequence[int], in_plane_limit: int) -> bool:
    return (
        preds.ndim == 5
        and preds.is_cuda
        and max(ks[0], gauss_ks[0]) <= 11
        and max(*ks[1:], *gauss_ks[1:]) <= in_plane_limit
        and all(n >= max(k, g) for n, k, g in zip(preds.shape[2:], ks, gauss_ks))
        and preds.shape[0] * preds.shape[1] <= 65535
    )


def _fused3d_ok(preds: Tensor, target: Tensor, ks: Sequence[int], gauss_ks: Sequence[int]) -> bool:
    """The forward-only volume kernel applies: ROCm, no gradient wanted by either input, in-plane windows up to 33."""
    return not _wants_grad(preds, target) and _window3d_fits(preds, ks, gauss_ks, 33)


def _fused3d_grad_ok(preds: Tensor, target: Tensor, ks: Sequence[int], gauss_ks: Sequence[int]) -> bool:
    """The differentiable volume kernels apply: ROCm, a gradient wanted, in-plane windows up to 15."""
    return _wants_grad(preds, target) and _window3d_fits(preds, ks, gauss_ks, ops.SSIM_GRAD_MAX_WINDOW)


def _fused3d_means(preds: Tensor, target: Tensor, taps: Sequence[Tensor], c1, c2, grad: bool = False):
    """Per-volume mean (over channels and valid windows) of the SSIM map and of the contrast sensitivity; ``grad``:
    through the differentiable kernels."""
    b, c, d, h, w = preds.shape
    acc = torch.float64 if preds.dtype == torch.float64 else torch.float32
    consts = torch.stack([torch.as_tensor(v, dtype=acc, device=preds.device) for v in (c1, c2, 0.0)])
    n = c * (d - taps[0].numel() + 1) * (h - taps[1].numel() + 1) * (w - taps[2].numel() + 1)
    if grad:  # consts keeps the graph of a data_range=None c1 / c2 (as_tensor and stack are differentiable)
        sums = ops.ssim3d_sums_grad(preds.reshape(b * c, d, h, w), target.reshape(b * c, d, h, w), *taps, consts)
        sums = sums.reshape(b, c, 2).sum(1) / n
        return sums[:, 0].to(preds.dtype), sums[:, 1].to(preds.dtype)
    part = ops.ssim3d_partials(preds.reshape(b * c, d, h, w), target.reshape(b * c, d, h, w), *taps, consts)
    sums = part.sum(1).reshape(b, c, 2).sum(1) / n
    return sums[:, 0].to(preds.dtype), sums[:, 1].to(preds.dtype)


_MAP_DTYPES = (torch.float32, torch.float64, torch.float16, torch.bfloat16)


def _fused_map_ok(preds: Tensor, target: Tensor, ks: Sequence[int], gauss_ks: Sequence[int]) -> bool:
    """A map kernel applies: ROCm image or volume, no gradient wanted by either input, windows within its limits."""
    if not preds.is_cuda or _wants_grad(preds, target) or preds.dtype not in _MAP_DTYPES:
        return False
    if preds.ndim == 4:
        return (_window_fits(preds, ks, gauss_ks, ops.SSIM_MAP_MAX_WINDOW)
                and preds.shape[0] * preds.shape[1] <= 65535)
    return _window3d_fits(preds, ks, gauss_ks, ops.SSIM_MAP_MAX_WINDOW)


def _fused_map(preds: Tensor, target: Tensor, taps: Sequence[Tensor], c1, c2) -> Tuple[Tensor, Tensor]:
    """``(per_image, full)`` of ``_ssim_update_conv(..., return_full_image=True)`` from one map-kernel launch."""
    b, c = preds.shape[:2]
    acc = torch.float64 if preds.dtype == torch.float64 else torch.float32
    consts = torch.stack([torch.as_tensor(v, dtype=acc, device=preds.device) for v in (c1, c2, 0.0)])
    planes = (b * c, *preds.shape[2:])
    op = ops.ssim2d_map if preds.ndim == 4 else ops.ssim3d_map
    full, part = op(preds.reshape(planes), target.reshape(planes), *taps, consts)
    n = c * math.prod(s - t.numel() + 1 for s, t in zip(preds.shape[2:], taps))  # the crop: windows fully inside
    per_image = part[..., 0].sum(1).reshape(b, c).sum(1) / n
    return per_image.to(preds.dtype), full.reshape(preds.shape)


def _ssim_update(
    preds: Tensor,
    target: Tensor,
    gaussian_kernel: bool = True,
    sigma: Union[float, Sequence[float]] = 1.5,
    kernel_size: Union[int, Sequence[int]] = 11,
    data_range: Optional[Union[float, Tuple[float, float]]] = None,
    k1: float = 0.01,
    k2: float = 0.03,
    return_full_image: bool = False,
    return_contrast_sensitivity: bool = False,
) -> Union[Tensor, Tuple[Tensor, Tensor]]:
    """Per-image SSIM (and optionally the contrast sensitivity or the full SSIM map)."""
    ks, sg = _normalise_args(preds, kernel_size, sigma)
    if return_full_image and return_contrast_sensitivity:
        raise ValueError("Arguments `return_full_image` and `return_contrast_sensitivity` are mutually exclusive.")
    preds, target, c1, c2 = _data_range_consts(preds, target, data_range, k1, k2)
    gauss_ks = [int(3.5 * s + 0.5) * 2 + 1 for s in sg]
    grad = _fused_grad_ok(preds, target, ks, gauss_ks)
    # a ROCm target that alone wants a gradient must not take the forward-only kernel either
    fwd = _fused_ok(preds, ks, gauss_ks) and not (preds.is_cuda and _wants_grad(preds, target))
    if not return_full_image and (grad or fwd) and (gaussian_kernel or ks == gauss_ks):
        wh, ww = _window_1d(gauss_ks if gaussian_kernel else ks, sg, gaussian_kernel, preds.dtype, preds.device)
        sim, cs = _fused_means(preds, target, wh, ww, c1, c2, 0.0, ops.SSIM_MODE, grad)
        return (sim, cs) if return_contrast_sensitivity else sim
    grad3d = _fused3d_grad_ok(preds, target, ks, gauss_ks)
    if not return_full_image and (grad3d or _fused3d_ok(preds, target, ks, gauss_ks)) and \
            (gaussian_kernel or ks == gauss_ks):
        acc = torch.float64 if preds.dtype == torch.float64 else torch.float32
        taps = _window_1d(gauss_ks if gaussian_kernel else ks, sg, gaussian_kernel, acc, preds.device)
        sim, cs = _fused3d_means(preds, target, taps, c1, c2, grad3d)
        return (sim, cs) if return_contrast_sensitivity else sim
    if return_full_image and _fused_map_ok(preds, target, ks, gauss_ks) and (gaussian_kernel or ks == gauss_ks):
        acc = torch.float64 if preds.dtype == torch.float64 else torch.float32
        taps = _window_1d(gauss_ks if gaussian_kernel else ks, sg, gaussian_kernel, acc, preds.device)
        return _fused_map(preds, target, taps, c1, c2)
    return _ssim_update_conv(preds, target, gaussian_kernel, ks, sg, gauss_ks, c1, c2, return_full_image,
                             return_contrast_sensitivity)


def _ssim_update_conv(preds, target, gaussian_kernel, ks, sg, gauss_ks, c1, c2, return_full_image,
                      return_contrast_sensitivity):
    """Explicit formulation: reflect pad, depthwise convolution of the 5 moment maps, crop the padded border."""
    is_3d = preds.ndim == 5
    channel, dtype, device = preds.size(1), preds.dtype, preds.device
    pads = [(k - 1) // 2 for k in gauss_ks]
    if is_3d:
        preds = _reflection_pad_3d(preds, pads[2], pads[1], pads[0])
        target = _reflection_pad_3d(target, pads[2], pads[1], pads[0])
        kernel = _gaussian_kernel_3d(channel, gauss_ks, sg, dtype, device) if gaussian_kernel else None
    else:
        preds = F.pad(preds, (pads[1], pads[1], pads[0], pads[0]), mode="reflect")
        target = F.pad(target, (pads[1], pads[1], pads[0], pads[0]), mode="reflect")
        kernel = _gaussian_kernel_2d(channel, gauss_ks, sg, dtype, device) if gaussian_kernel else None
    if kernel is None:
        kernel = torch.ones((channel, 1, *ks), dtype=dtype, device=device) / torch.prod(
            torch.tensor(ks, dtype=dtype, device=device))
    stacked = torch.cat((preds, target, preds * preds, target * target, preds * target))
    conv = F.conv3d if is_3d else F.conv2d
    mu_p, mu_t, e_pp, e_tt, e_pt = conv(stacked, kernel, groups=channel).split(preds.shape[0])
    mpp, mtt, mpt = mu_p.pow(2), mu_t.pow(2), mu_p * mu_t
    s_pp = torch.clamp(e_pp - mpp, min=0.0)
    s_tt = torch.clamp(e_tt - mtt, min=0.0)
    s_pt = e_pt - mpt
    upper = 2 * s_pt.to(dtype) + c2
    lower = (s_pp + s_tt).to(dtype) + c2
    full = ((2 * mpt + c1) * upper) / ((mpp + mtt + c1) * lower)
    crop = (Ellipsis,) + tuple(slice(p, -p if p else None) for p in pads)
    ssim_idx = full[crop]
    per_image = ssim_idx.reshape(ssim_idx.shape[0], -1).mean(-1)
    if return_contrast_sensitivity:
        cs = (upper / lower)[crop]
        return per_image, cs.reshape(cs.shape[0], -1).mean(-1)
    if return_full_image:
        return per_image, full
    return per_image


def _ssim_compute(similarities: Tensor, reduction: _Reduction = "elementwise_mean") -> Tensor:
    return reduce(similarities, reduction)


def structural_similarity_index_measure(
    preds: Tensor,
    target: Tensor,
    gaussian_kernel: bool = True,
    sigma: Union[float, Sequence[float]] = 1.5,
    kernel_size: Union[int, Sequence[int]] = 11,
    reduction: _Reduction = "elementwise_mean",
    data_range: Optional[Union[float, Tuple[float, float]]] = None,
    k1: float = 0.01,
    k2: float = 0.03,
    return_full_image: bool = False,
    return_contrast_sensitivity: bool = False,
) -> Union[Tensor, Tuple[Tensor, Tensor]]:
    """Structural similarity index (2-D images or 3-D volumes)."""
    preds, target = _ssim_check_inputs(preds, target)
    pack = _ssim_update(preds, target, gaussian_kernel, sigma, kernel_size, data_range, k1, k2, return_full_image,
                        return_contrast_sensitivity)
    if isinstance(pack, tuple):
        return _ssim_compute(pack[0], reduction), pack[1]
    return _ssim_compute(pack, reduction)


def _multiscale_ssim_update(
    preds: Tensor,
    target: Tensor,
    gaussian_kernel: bool = True,
    sigma: Union[float, Sequence[float]] = 1.5,
    kernel_size: Union[int, Sequence[int]] = 11,
    data_range: Optional[Union[float, Tuple[float, float]]] = None,
    k1: float = 0.01,
    k2: float = 0.03,
    betas: Tuple[float, ...] = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333),
    normalize: Optional[Literal["relu", "simple"]] = None,
) -> Tensor:
    """Per-image MS-SSIM: contrast sensitivity at the coarse-to-fine scales, SSIM at the last one."""
    is_3d = preds.ndim == 5
    ks = list(kernel_size) if isinstance(kernel_size, Sequence) else (3 if is_3d else 2) * [kernel_size]
    sg = list(sigma) if isinstance(sigma, Sequence) else (3 if is_3d else 2) * [sigma]
    if preds.size()[-1] < 2 ** len(betas) or preds.size()[-2] < 2 ** len(betas):
        raise ValueError(
            f"For a given number of `betas` parameters {len(betas)}, the image height and width dimensions must be"
            f" larger than or equal to {2 ** len(betas)}."
        )
    div = max(1, (len(betas) - 1)) ** 2
    if preds.size()[-2] // div <= ks[0] - 1:
        raise ValueError(
            f"For a given number of `betas` parameters {len(betas)} and kernel size {ks[0]},"
            f" the image height must be larger than {(ks[0] - 1) * div}."
        )
    if preds.size()[-1] // div <= ks[1] - 1:
        raise ValueError(
            f"For a given number of `betas` parameters {len(betas)} and kernel size {ks[1]},"
            f" the image width must be larger than {(ks[1] - 1) * div}."
        )
    cs_list: List[Tensor] = []
    sim = None
    pool = F.avg_pool3d if is_3d else F.avg_pool2d
    for _ in range(len(betas)):
        sim, cs = _ssim_update(preds, target, gaussian_kernel, sg, ks, data_range, k1, k2,
                               return_contrast_sensitivity=True)
        if normalize == "relu":
            sim, cs = torch.relu(sim), torch.relu(cs)
        cs_list.append(cs)
        preds = pool(preds, (2, 2, 2) if is_3d else (2, 2))
        target = pool(target, (2, 2, 2) if is_3d else (2, 2))
    cs_list[-1] = sim
    stack = torch.stack(cs_list)
    if normalize == "simple":
        stack = (stack + 1) / 2
    w = torch.tensor(betas, device=stack.device).view(-1, 1)
    return torch.prod(stack**w, dim=0)


def _multiscale_ssim_compute(mcs_per_image: Tensor, reduction: _Reduction = "elementwise_mean") -> Tensor:
    return reduce(mcs_per_image, reduction)


def multiscale_structural_similarity_index_measure(
    preds: Tensor,
    target: Tensor,
    gaussian_kernel: bool = True,
    sigma: Union[float, Sequence[float]] = 1.5,
    kernel_size: Union[int, Sequence[int]] = 11,
    reduction: _Reduction = "elementwise_mean",
    data_range: Optional[Union[float, Tuple[float, float]]] = None,
    k1: float = 0.01,
    k2: float = 0.03,
    betas: Tuple[float, ...] = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333),
    normalize: Optional[Literal["relu", "simple"]] = "relu",
) -> Tensor:
    """Multi-scale structural similarity index."""
    if not isinstance(betas, tuple):
        raise ValueError("Argument `betas` is expected to be of a type tuple.")
    if isinstance(betas, tuple) and not all(isinstance(beta, float) for beta in betas):
        raise ValueError("Argument `betas` is expected to be a tuple of floats.")
    if normalize and normalize not in ("relu", "simple"):
        raise ValueError("Argument `normalize` to be expected either `None` or one of 'relu' or 'simple'")
    preds, target = _ssim_check_inputs(preds, target)
    mcs = _multiscale_ssim_update(preds, target, gaussian_kernel, sigma, kernel_size, data_range, k1, k2, betas,
                                  normalize)
    return _multiscale_ssim_compute(mcs, reduction)


# ----------------------------------------------------------------------------------------------------------- UQI
def _uqi_update(preds: Tensor, target: Tensor) -> Tuple[Tensor, Tensor]:
    if preds.dtype != target.dtype:
        raise TypeError(
            "Expected `preds` and `target` to have the same data type."
            f" Got preds: {preds.dtype} and target: {target.dtype}."
        )
    _check_same_shape(preds, target)
    if len(preds.shape) != 4:
        raise ValueError(
            "Expected `preds` and `target` to have BxCxHxW shape."
            f" Got preds: {preds.shape} and target: {target.shape}."
        )
    return preds, target


def _uqi_compute(
    preds: Tensor,
    target: Tensor,
    kernel_size: Sequence[int] = (11, 11),
    sigma: Sequence[float] = (1.5, 1.5),
    reduction: Optional[Literal["elementwise_mean", "sum", "none"]] = "elementwise_mean",
) -> Tensor:
    if len(kernel_size) != 2 or len(sigma) != 2:
        raise ValueError(
            "Expected `kernel_size` and `sigma` to have the length of two."
            f" Got kernel_size: {len(kernel_size)} and sigma: {len(sigma)}."
        )
    if any(x % 2 == 0 or x <= 0 for x in kernel_size):
        raise ValueError(f"Expected `kernel_size` to have odd positive number. Got {kernel_size}.")
    if any(y <= 0 for y in sigma):
        raise ValueError(f"Expected `sigma` to have positive number. Got {sigma}.")
    eps = torch.finfo(preds.dtype).eps
    square = kernel_size[0] == kernel_size[1]  # the reference pads H by the W half-width (identical when square)
    if reduction in ("elementwise_mean", "sum") and square and _fused_ok(preds, list(kernel_size), [1, 1]):
        b, c, h, w = preds.shape
        wh, ww = _window_1d(kernel_size, sigma, True, preds.dtype, preds.device)
        acc = torch.float64 if preds.dtype == torch.float64 else torch.float32
        consts = torch.tensor([0.0, 0.0, eps], dtype=acc, device=preds.device)
        part = ops.ssim2d_partials(preds.reshape(b * c, h, w), target.reshape(b * c, h, w), wh, ww, consts,
                                   ops.UQI_MODE)
        total = part[..., 0].sum()
        if reduction == "sum":
            return total.to(preds.dtype)
        n = b * c * (h - kernel_size[0] + 1) * (w - kernel_size[1] + 1)
        return (total / n).to(preds.dtype)
    if reduction in ("none", None) and square and _fused_map_ok(preds, target, list(kernel_size), [1, 1]):
        b, c, h, w = preds.shape
        wh, ww = _window_1d(kernel_size, sigma, True, preds.dtype, preds.device)
        acc = torch.float64 if preds.dtype == torch.float64 else torch.float32
        consts = torch.tensor([0.0, 0.0, eps], dtype=acc, device=preds.device)
        full, _ = ops.ssim2d_map(preds.reshape(b * c, h, w), target.reshape(b * c, h, w), wh, ww, consts,
                                 ops.UQI_MODE, reflect=False)
        return full.reshape(b, c, *full.shape[1:])
    return reduce(_uqi_map(preds, target, kernel_size, sigma, eps), reduction)


def _uqi_map(preds: Tensor, target: Tensor, kernel_size: Sequence[int], sigma: Sequence[float], eps: float) -> Tensor:
    channel = preds.size(1)
    kernel = _gaussian_kernel_2d(channel, kernel_size, sigma, preds.dtype, preds.device)
    ph, pw = (kernel_size[0] - 1) // 2, (kernel_size[1] - 1) // 2
    preds = F.pad(preds, (ph, ph, pw, pw), mode="reflect")
    target = F.pad(target, (ph, ph, pw, pw), mode="reflect")
    stacked = torch.cat((preds, target, preds * preds, target * target, preds * target))
    mu_p, mu_t, e_pp, e_tt, e_pt = F.conv2d(stacked, kernel, groups=channel).split(preds.shape[0])
    mpp, mtt, mpt = mu_p.pow(2), mu_t.pow(2), mu_p * mu_t
    s_pp = torch.clamp(e_pp - mpp, min=0.0)
    s_tt = torch.clamp(e_tt - mtt, min=0.0)
    upper = 2 * (e_pt - mpt)
    lower = s_pp + s_tt
    uqi = ((2 * mpt) * upper) / ((mpp + mtt) * lower + eps)
    return uqi[..., ph:-ph if ph else None, pw:-pw if pw else None]


def universal_image_quality_index(
    preds: Tensor,
    target: Tensor,
    kernel_size: Sequence[int] = (11, 11),
    sigma: Sequence[float] = (1.5, 1.5),
    reduction: Optional[Literal["elementwise_mean", "sum", "none"]] = "elementwise_mean",
) -> Tensor:
    """Universal image quality index (Wang & Bovik)."""
    preds, target = _uqi_update(preds, target)
    return _uqi_compute(preds, target, kernel_size, sigma, reduction)


def _uqi_plane_means(a: Tensor, b: Tensor, kernel_size: Sequence[int] = (11, 11),
                     sigma: Sequence[float] = (1.5, 1.5)) -> Tensor:
    """Mean UQI of every ``[P, 1, H, W]`` plane pair (the reference's ``reduction='none'`` map, averaged per plane)."""
    eps = torch.finfo(a.dtype).eps
    if kernel_size[0] == kernel_size[1] and _fused_ok(a, list(kernel_size), [1, 1]):
        p, _, h, w = a.shape
        wh, ww = _window_1d(kernel_size, sigma, True, a.dtype, a.device)
        acc = torch.float64 if a.dtype == torch.float64 else torch.float32
        consts = torch.tensor([0.0, 0.0, eps], dtype=acc, device=a.device)
        part = ops.ssim2d_partials(a.reshape(p, h, w), b.reshape(p, h, w), wh, ww, consts, ops.UQI_MODE)
        n = (h - kernel_size[0] + 1) * (w - kernel_size[1] + 1)
        return (part[..., 0].sum(1) / n).to(a.dtype)
    return _uqi_map(a, b, kernel_size, sigma, eps).flatten(1).mean(1)
