"""Dense-prediction multiclass updates (``csrc/classification/mc_dense.hip``): float scores ``[N, C, X]`` with X > 1.

The reference is the CPU contract ``ops.mc_update`` on the fp64 upcast of the exact input values (``torch.argmax`` on
the CPU returns the first maximum and ranks NaN highest, which is ``argmax_better``); counts are integers, so every
comparison is ``torch.equal``.
"""
import pytest
import torch

import torchmetrics_amd.functional as F
from torchmetrics_amd import ops
from torchmetrics_amd.classification import MulticlassConfusionMatrix, MulticlassJaccardIndex

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MODES = {"confmat": (ops.MC_CONFMAT, False), "stats": (ops.MC_STATS, False), "samplewise": (ops.MC_STATS, True)}
SHAPES = [(2, 3, 2), (3, 5, 49), (1, 19, 4099), (3, 19, 2056), (2, 16, 1024), (2, 17, 1024), (2, 110, 520),
          (2, 111, 520), (1, 150, 300), (1, 203, 260)]  # C = 150: the 90 KB histogram of one 1024-thread block


def _inputs(n, c, x, dtype, ignore=None):
    """Seeded scores and targets, about 1 in 11 of the targets ignored."""
    g = torch.Generator().manual_seed(n * 7919 + c * 31 + x)
    p = torch.randn(n, c, x, generator=g).to(dtype)
    t = torch.randint(0, c, (n, x), generator=g)
    if ignore is not None:
        t[torch.rand(n, x, generator=g) < 1 / 11] = ignore
    return p, t


def _out(n, c, mode, samplewise, device):
    size = c * c if mode == ops.MC_CONFMAT else (n if samplewise else 1) * (3 * c + 1)
    return torch.zeros(size, dtype=torch.int64, device=device), torch.zeros(1, dtype=torch.int32, device=device)


def _check(p, t, c, ignore, mode, samplewise, t_ref=None):
    """Run the kernel on (p, t) and compare with the CPU contract on (p, t_ref or t); returns the kernel's flag."""
    n = t.shape[0]
    out, flag = _out(n, c, mode, samplewise, "cuda")
    assert ops.mc_dense_update(p, t.cuda(), out, flag, c, ignore, mode, samplewise) is True
    ref, ref_flag = _out(n, c, mode, samplewise, "cpu")
    ops.mc_update(p.double().cpu(), t if t_ref is None else t_ref, ref, ref_flag, c, ignore, mode, samplewise)
    assert torch.equal(out.cpu(), ref)
    return int(flag.item())


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("ignore", [None, 255])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_dense_update_matches_cpu_contract(dtype, mode, ignore, shape):
    n, c, x = shape
    p, t = _inputs(n, c, x, dtype, ignore)
    assert _check(p.cuda(), t, c, ignore, *MODES[mode]) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_dense_update_offset_pointer(dtype):
    """A base pointer one element off 16-byte alignment: the narrower load width."""
    p, t = _inputs(3, 19, 2056, dtype, 255)
    dev = torch.cat([p.new_zeros(1), p.reshape(-1)]).cuda()[1:].view(p.shape)
    assert dev.data_ptr() % 16 == dev.element_size() and dev.is_contiguous()
    assert _check(dev, t, 19, 255, ops.MC_CONFMAT, False) == 0


@pytest.mark.parametrize("mode", ["confmat", "stats"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_dense_update_ties_nan_uniform_regions(dtype, mode):
    """4 score levels (ties), planted NaNs, scores constant over 16 pixels and targets over 64: long equal runs that
    cross thread and tile boundaries."""
    g = torch.Generator().manual_seed(11)
    p = torch.randint(0, 4, (2, 7, 96), generator=g).float().repeat_interleave(16, dim=2)
    p[torch.rand(p.shape, generator=g) < 0.02] = float("nan")
    t = torch.randint(0, 7, (2, 24), generator=g).repeat_interleave(64, dim=1)
    assert _check(p.to(dtype).cuda(), t, 7, None, *MODES[mode]) == 0


@pytest.mark.parametrize("mode", list(MODES))
def test_dense_update_flags_target_out_of_range(mode):
    p, t = _inputs(2, 5, 300, torch.float32)
    bad, masked = t.clone(), t.clone()
    bad[1, 77], masked[1, 77] = 5, 255
    assert _check(p.cuda(), bad, 5, 255, *MODES[mode], t_ref=masked) != 0


@pytest.mark.parametrize("samplewise", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize(("shape", "k"), [(s, k) for s in [(2, 19, 515), (1, 16, 64)] for k in (2, 5, 16)], ids=str)
def test_dense_topk_matches_label_path(shape, k, dtype, samplewise):
    """top_k: the workspace of the label path on the same values (topk_labels on [N X, C] rows + the label histogram)."""
    n, c, x = shape
    p, t = _inputs(n, c, x, dtype, 255)
    p, t = p.cuda(), t.cuda()
    ws, flag = _out(n, c, ops.MC_STATS, samplewise, "cuda")
    assert ops.mc_dense_update(p, t, ws, flag, c, 255, ops.MC_STATS, samplewise, k) is True
    labels = ops.topk_labels(p.permute(0, 2, 1).reshape(n * x, c), k).view(n, x, k).permute(0, 2, 1).contiguous()
    ref, _ = _out(n, c, ops.MC_STATS, samplewise, "cuda")
    ops.mc_update(labels, t, ref, flag, c, 255, ops.MC_STATS, samplewise)
    assert torch.equal(ws, ref) and int(flag.item()) == 0


@pytest.mark.parametrize("multidim_average", ["global", "samplewise"])
def test_stat_scores_top_k_takes_dense_kernel(monkeypatch, multidim_average):
    calls = []
    real = ops.mc_dense_update
    monkeypatch.setattr(ops, "mc_dense_update", lambda *a, **k: calls.append(1) or real(*a, **k))
    g = torch.Generator().manual_seed(5)
    p, t = torch.randn(2, 19, 24, 33, generator=g), torch.randint(0, 19, (2, 24, 33), generator=g)
    kw = dict(num_classes=19, top_k=3, average=None, multidim_average=multidim_average)  # per-class integer counts
    got = F.multiclass_stat_scores(p.cuda(), t.cuda(), **kw)
    assert calls
    assert torch.equal(got.cpu(), F.multiclass_stat_scores(p, t, **kw))


@pytest.mark.parametrize("metric", [lambda: MulticlassConfusionMatrix(19, ignore_index=255),
                                    lambda: MulticlassJaccardIndex(19)], ids=["confmat", "jaccard"])
def test_modules_on_dense_bf16_match_cpu(metric):
    g = torch.Generator().manual_seed(6)
    gpu, cpu = metric().cuda(), metric()
    for step in range(3):  # two updates, then one forward
        p = torch.randn(2, 19, 24, 33, generator=g).bfloat16()
        t = torch.randint(0, 19, (2, 24, 33), generator=g)
        if getattr(gpu, "ignore_index", None) == 255:
            t[0, step] = 255
        if step < 2:
            gpu.update(p.cuda(), t.cuda()), cpu.update(p.float(), t)
        else:
            torch.testing.assert_close(gpu(p.cuda(), t.cuda()).cpu(), cpu(p.float(), t))
    torch.testing.assert_close(gpu.compute().cpu(), cpu.compute())


def test_dense_update_not_applicable():
    p, t = _inputs(2, 5, 64, torch.float32)
    cases = [(p, t, 1), (p[:, :, 0].cuda(), t[:, 0].cuda(), 1), (p.double().cuda(), t.cuda(), 1),
             (torch.randn(2, 19, 64).cuda(), t.cuda(), 17)]  # CPU tensors; X == 1; f64; top_k = 17
    for preds, target, k in cases:
        c = preds.shape[1]
        out, flag = _out(2, c, ops.MC_STATS, False, preds.device)
        assert ops.mc_dense_update(preds, target, out, flag, c, None, ops.MC_STATS, False, k) is False
        assert not out.any()
