"""LPIPS / PPL (reference ``tests/unittests/image/test_lpips.py``, ``test_perceptual_path_length.py``).  torchvision and
the ImageNet backbones are unavailable, so the tests run random backbones and check (a) the fused layer distance
against the composite formula, (b) loading of the reference's shipped LPIPS heads (safe ``weights_only`` load) and
of torchvision-layout backbone checkpoints, (c) PPL's interpolation / trimming arithmetic."""
import os

import pytest
import torch

from torchmetrics_amd import ops
from torchmetrics_amd.functional.image.lpips import _Backbone, _LPIPS, _NoTrainLpips
from torchmetrics_amd.functional.image.perceptual_path_length import _interpolate, perceptual_path_length
from torchmetrics_amd.image import LearnedPerceptualImagePatchSimilarity, PerceptualPathLength

_REF_LPIPS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_heads")


def _manual_lpips(net: _LPIPS, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    x0, x1 = (a - net.shift) / net.scale, (b - net.shift) / net.scale
    f0, f1 = net.net(x0), net.net(x1)
    tot = 0
    for k in range(len(f0)):
        n0 = f0[k] / (f0[k].pow(2).sum(1, keepdim=True).sqrt() + 1e-8)
        n1 = f1[k] / (f1[k].pow(2).sum(1, keepdim=True).sqrt() + 1e-8)
        w = net.lins[k].model[-1].weight.reshape(1, -1, 1, 1)
        tot = tot + ((n0 - n1) ** 2 * w).sum(1).mean((1, 2))
    return tot


@pytest.mark.parametrize("net_type", ["alex", "vgg", "squeeze"])
def test_lpips_random_backbone(net_type, device="cpu"):
    torch.manual_seed(0)
    net = _NoTrainLpips(pretrained=False, net=net_type, pnet_rand=True).to(device)
    a, b = torch.rand(3, 3, 64, 64, device=device) * 2 - 1, torch.rand(3, 3, 64, 64, device=device) * 2 - 1
    with torch.no_grad():
        got = net(a, b).reshape(-1)
        ref = _manual_lpips(net, a, b)
    assert torch.allclose(got, ref, rtol=1e-4, atol=1e-6)
    # composite (differentiable) path agrees and produces gradients
    a.requires_grad_(True)
    val = net(a, b).sum()
    val.backward()
    assert a.grad is not None and torch.isclose(val.detach(), ref.sum(), rtol=1e-4)


def test_lpips_module_and_errors():
    m = LearnedPerceptualImagePatchSimilarity(net_type="squeeze", pretrained=False, pnet_rand=True, normalize=True)
    a, b = torch.rand(4, 3, 48, 48), torch.rand(4, 3, 48, 48)
    m.update(a[:2], b[:2])
    m.update(a[2:], b[2:])
    with torch.no_grad():
        ref = m.net(a, b, normalize=True).reshape(-1).mean()
    assert torch.isclose(m.compute(), ref, rtol=1e-5)
    with pytest.raises(ValueError):
        m.update(a * 3, b)
    with pytest.raises(FileNotFoundError):
        LearnedPerceptualImagePatchSimilarity(net_type="alex")  # no local ImageNet backbone, nothing downloaded
    with pytest.raises(ValueError):
        LearnedPerceptualImagePatchSimilarity(net_type="resnet", pnet_rand=True, pretrained=False)


@pytest.mark.parametrize("net_type", ["alex", "vgg", "squeeze"])
def test_lpips_loads_reference_heads(net_type):
    path = os.path.join(_REF_LPIPS, f"{net_type}.pth")
    net = _NoTrainLpips(pretrained=True, net=net_type, pnet_rand=True, model_path=path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    for k, v in sd.items():
        assert torch.equal(net.state_dict()[k], v), k


def test_backbone_torchvision_layout():
    src = _Backbone("vgg")
    flat = {}
    for k in range(1, src.n_slices + 1):
        for name, mod in getattr(src, f"slice{k}")._modules.items():
            for pn, p in mod.state_dict().items():
                flat[f"features.{name}.{pn}"] = p
    flat["classifier.0.weight"] = torch.zeros(1)  # ignored
    dst = _Backbone("vgg")
    dst.load_torchvision(flat)
    x = torch.rand(1, 3, 32, 32)
    assert all(torch.equal(u, v) for u, v in zip(src(x), dst(x)))


class _Gen(torch.nn.Module):
    def __init__(self, z=8):
        super().__init__()
        self.z = z
        self.lin = torch.nn.Linear(z, 3 * 32 * 32)

    def forward(self, z):
        return 255 * torch.sigmoid(self.lin(z)).reshape(-1, 3, 32, 32)

    def sample(self, n):
        return torch.randn(n, self.z)


def test_ppl():
    torch.manual_seed(0)
    z1, z2 = torch.randn(5, 8), torch.randn(5, 8)
    assert torch.allclose(_interpolate(z1, z2, 0.5, "lerp"), (z1 + z2) / 2)
    s = _interpolate(z1, z2, 1e-4, "slerp_unit")
    assert torch.allclose(s.norm(dim=-1), torch.ones(5), atol=1e-5)
    sim = _LPIPS(pretrained=False, net="alex", pnet_rand=True)
    gen = _Gen()
    torch.manual_seed(1)
    mean, std, d = perceptual_path_length(gen, num_samples=20, batch_size=8, sim_net=sim, resize=None,
                                          lower_discard=None, upper_discard=None)
    assert 0 < d.numel() <= 20 and (d >= 0).all()  # lower bound defaults to 0 like the reference
    assert torch.isclose(mean, d.mean()) and torch.isclose(std, d.std())
    m = PerceptualPathLength(num_samples=20, batch_size=8, sim_net=sim, lower_discard=0.1, upper_discard=0.9)
    m.update(gen)
    _, _, d2 = m.compute()
    assert d2.numel() <= 20


@pytest.mark.gpu
@pytest.mark.parametrize("net_type", ["alex", "vgg", "squeeze"])
def test_lpips_fused_kernel_gpu(net_type):
    test_lpips_random_backbone(net_type, device="cuda")
    f0, f1 = torch.randn(3, 37, 9, 11, device="cuda"), torch.randn(3, 37, 9, 11, device="cuda")
    w = torch.randn(37, device="cuda")
    got = ops.lpips_layer(f0, f1, w)
    ref = ops.lpips_layer(f0.cpu(), f1.cpu(), w.cpu())
    assert torch.allclose(got.cpu(), ref, rtol=1e-5, atol=1e-6)
    assert torch.equal(ops.lpips_layer(f0, f0, w), torch.zeros(3, device="cuda"))
