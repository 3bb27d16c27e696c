"""The raw-bit shortcut of the 16-bit multiclass argmax kernel (``wave_argmax_raw16`` in
``csrc/classification/stat_scores.hip``) on the rows where raw bit patterns and float order part ways.

Every case holds the kernel to ``torch.argmax`` of the fp32 copy on the CPU (first maximum, any NaN wins, first NaN
among NaNs, -0 == +0 ties by column), through the four modes of the kernel: the functional confusion matrix and stats
workspace (``ops.mc_update``), ``MulticlassConfusionMatrix.forward`` (batch + global matrix in one pass) and the
``MulticlassAccuracy(average=None)`` update (straight into tp / fp / tn / fn).  C = 512 / 1000 / 1536 / 2048 is 1-4
16-byte chunks per lane (1000: a ragged last chunk); N = 3 / 8192 / 8193 / 20000 is fewer rows than waves, exactly one
row per wave (the loop-free kernel), one over, and the pipelined persistent grid.  All comparisons are exact.
"""
import functools

import pytest
import torch

import torchmetrics_amd as tm
from torchmetrics_amd import ops

DEV = "cuda"
ROWS = 64  # rows per row set
BITS = {  # +inf, -inf, +NaN, -NaN (two payloads each), 1.0
    torch.bfloat16: dict(pinf=0x7F80, ninf=0xFF80, pnan=(0x7FC1, 0x7FA5), nnan=(0xFFC1, 0xFF93)),
    torch.float16: dict(pinf=0x7C00, ninf=0xFC00, pnan=(0x7E01, 0x7D05), nnan=(0xFE01, 0xFC93)),
}


def _i16(u):
    return u - 0x10000 if u >= 0x8000 else u


def _pairs(C):
    """Column pairs (a < b) on both sides of every ownership boundary of the lane layout (lane l of round j owns columns
    (l + 64 j) * 8 .. + 7): two lanes, lane 63 of round 0 / lane 0 of round 1, last full chunk / tail, one word."""
    ps = [(7, 8), (8, 9), (C - 9, C - 8), (C - 8, C - 1), (C - 2, C - 1), (0, C - 1)]
    if C > 512:
        ps.append((511, 512))
    if C == 1000:
        ps += [(991, 992), (992, 999)]
    return ps


def _row_sets(dtype, C, g):
    """name -> [ROWS, C] rows, in a fixed order."""
    b = BITS[dtype]
    pairs = _pairs(C)
    sets = {}

    def neg():  # all negative, in [-2, -1): plenty of ties among the non-maxima
        return (-torch.rand(ROWS, C, generator=g) - 1).to(dtype)

    def small():  # in (-1, 1)
        return (torch.rand(ROWS, C, generator=g) * 2 - 1).to(dtype)

    def put(x, r, c, u):
        x.view(torch.int16)[r, c] = _i16(u)

    x = neg()
    for r in range(ROWS):  # maximum: the smallest positive subnormal; +-0 around it
        put(x, r, (r * 37 + 11) % C, 0x0001)
        put(x, r, (r * 37 + 12) % C, 0x0000 if r & 1 else 0x8000)
        put(x, r, (r * 37 + 5) % C, 0x8000 if r & 1 else 0x0000)
    sets["subnormal_max"] = x
    x = neg()
    for r in range(ROWS):  # maximum +-0: -0 before +0 and the reverse, the first of the two wins
        a, c = pairs[r % len(pairs)]
        put(x, r, a, 0x8000 if r & 1 else 0x0000)
        put(x, r, c, 0x0000 if r & 1 else 0x8000)
    sets["zero_max_signs"] = x
    x = neg()
    for r in range(ROWS):  # all negative, one maximum
        x[r, (r * 53 + 3) % C] = -0.5
    sets["all_negative"] = x
    x = neg()
    for r in range(ROWS):  # all negative, the maximum twice
        a, c = pairs[r % len(pairs)]
        x[r, a] = -0.25
        x[r, c] = -0.25
    sets["all_negative_ties"] = x
    x = neg()
    for r in range(ROWS):  # all negative but one -0
        put(x, r, (r * 29 + 1) % C, 0x8000)
    sets["all_negative_one_negzero"] = x
    x = small()
    for r in range(ROWS):  # a positive maximum and, elsewhere, a -NaN: the NaN wins
        x[r, (r * 17) % C] = 3.0
        put(x, r, (r * 41 + 20) % C, b["nnan"][r & 1])
    sets["positive_max_neg_nan"] = x
    x = small()
    for r in range(ROWS):  # +NaN and -NaN, different payloads: the first NaN wins
        a, c = pairs[r % len(pairs)]
        put(x, r, a, b["nnan"][0] if r & 1 else b["pnan"][1])
        put(x, r, c, b["pnan"][0] if r & 1 else b["nnan"][1])
        x[r, 3] = 3.0  # in no pair
    sets["nan_both_signs"] = x
    x = torch.randn(ROWS, C, generator=g).to(dtype)
    for r in range(ROWS):
        a, c = pairs[r % len(pairs)]
        put(x, r, a, b["pinf"])
        put(x, r, c, b["pinf"])
    sets["pos_inf_ties"] = x
    x = neg()
    x.view(torch.int16)[:] = _i16(b["ninf"])
    sets["all_neg_inf"] = x
    sets["all_equal_positive"] = torch.full((ROWS, C), 1.5).to(dtype)
    x = small()
    for r in range(ROWS):
        a, c = pairs[r % len(pairs)]
        x[r, a] = 2.0
        x[r, c] = 2.0
    sets["positive_ties"] = x
    return sets


# sets whose answer a plain maximum of the raw int16 patterns cannot give (the others are there for the tie order)
RAW_MAX_FAILS = ("all_negative", "all_negative_ties", "all_negative_one_negzero", "positive_max_neg_nan")
RAW_MAX_FAILS_ODD_ROWS = ("zero_max_signs", "nan_both_signs")  # odd rows: -0 / -NaN first, +0 / +NaN second


@functools.lru_cache(maxsize=2)
def _case(dtype, C, N):
    """(preds, target, argmax): the row sets at the head and, where they fit twice, again at the tail (the rows the
    persistent grid reaches through its next-row registers), random rows between."""
    g = torch.Generator().manual_seed(C * 31 + N)
    block = torch.cat(list(_row_sets(dtype, C, g).values()))
    B = block.shape[0]
    if N < B:
        preds = block[torch.arange(N) * (B // N) + 1].clone()
    else:
        preds = torch.randn(N, C, generator=g).to(dtype)
        preds[:B] = block
        if N >= 2 * B:
            preds[N - B:] = block
    target = torch.randint(0, C, (N,), generator=g)
    return preds, target, preds.float().argmax(1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("C", [512, 1000, 1536, 2048])
def test_row_sets_not_degenerate(dtype, C):
    """No GPU: the expected column of every row set is not what a naive maximum over the raw int16 patterns finds, or
    (the tie sets and the subnormal) the maximum sits in two columns / away from column 0."""
    g = torch.Generator().manual_seed(C)
    for name, x in _row_sets(dtype, C, g).items():
        want = x.float().argmax(1)
        naive = x.view(torch.int16).to(torch.int32).argmax(1)
        if name in RAW_MAX_FAILS:
            assert (want != naive).all(), name
        elif name in RAW_MAX_FAILS_ODD_ROWS:
            assert (want != naive)[1::2].all(), name
            assert (want == torch.tensor([_pairs(C)[r % len(_pairs(C))][0] for r in range(ROWS)])).all(), name
        elif name == "subnormal_max":
            assert (want != 0).all() and (x.float().max(1).values > 0).all(), name
        elif name in ("all_equal_positive", "all_neg_inf"):
            assert (want == 0).all(), name
        else:  # two columns hold the maximum and the first of them is the answer
            xf = x.float()
            assert ((xf == xf.max(1, keepdim=True).values).sum(1) == 2).all(), name
            assert (want == torch.tensor([_pairs(C)[r % len(_pairs(C))][0] for r in range(ROWS)])).all(), name


def _mc(preds, target, C, ignore, mode, dev):
    out = torch.zeros(C * C if mode == ops.MC_CONFMAT else 3 * C + 1, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.mc_update(preds.to(dev), target.to(dev), out, flag, C, ignore, mode, False)
    return out.cpu(), int(flag.item())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["confmat", "stats", "forward_dual", "accuracy_direct"])
@pytest.mark.parametrize("N", [3, 8192, 8193, 20000])
@pytest.mark.parametrize("C", [512, 1000, 1536, 2048])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_raw16_argmax_modes(dtype, C, N, mode):
    preds, target, amax = _case(dtype, C, N)
    if mode in ("confmat", "stats"):  # ignored rows, one out-of-range target: skipped, and the flag word says so
        t = target.clone()
        t[::13] = -100
        t[1] = C
        keep = (t != -100) & (t != C)
        op_mode = ops.MC_CONFMAT if mode == "confmat" else ops.MC_STATS
        gpu, fg = _mc(preds, t, C, -100, op_mode, DEV)
        cpu, fc = _mc(preds, t, C, -100, op_mode, "cpu")
        assert fg == fc != 0
        assert torch.equal(gpu, cpu)
        if mode == "confmat":
            assert torch.equal(gpu, torch.bincount(t[keep] * C + amax[keep], minlength=C * C))
    elif mode == "forward_dual":
        t = target.clone()
        t[::7] = 2
        keep = t != 2
        direct = torch.bincount(t[keep] * C + amax[keep], minlength=C * C).reshape(C, C)
        m = tm.MulticlassConfusionMatrix(C, ignore_index=2).to(DEV)
        for i in range(3):  # the first call creates the flag word in Python; the next two take the dual kernel
            val = m(preds.to(DEV), t.to(DEV))
            assert m.forward.native_calls == i, m.forward.decline_line
            assert torch.equal(val.cpu(), direct)
        assert torch.equal(m.compute().cpu(), 3 * direct)
    else:
        m = tm.MulticlassAccuracy(C, average=None).to(DEV)
        ref = tm.MulticlassAccuracy(C, average=None)
        for _ in range(3):  # the first update runs in Python (stats workspace), the next two go straight to the states
            m.update(preds.to(DEV), target.to(DEV))
            ref.update(preds, target)
        assert m.update.native_calls == 2  # the stats-direct launcher, not the Python update's workspace kernel
        hit = amax == target
        tp = torch.bincount(target[hit], minlength=C)
        fp = torch.bincount(amax[~hit], minlength=C)
        fn = torch.bincount(target[~hit], minlength=C)
        want = dict(tp=tp, fp=fp, fn=fn, tn=N - tp - fp - fn)
        for k in ("tp", "fp", "tn", "fn"):
            assert torch.equal(getattr(m, k).cpu(), 3 * want[k]), k
            assert torch.equal(getattr(m, k).cpu(), getattr(ref, k)), k
