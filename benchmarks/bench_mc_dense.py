"""Dense-prediction multiclass updates (csrc/classification/mc_dense.hip) against the dispatch they replace.

Inputs are segmentation-shaped: logits [N, C, H, W] and targets [N, H, W] that are constant over 16 x 16 pixel blocks
(8 x 8 in the 24 x 24 input), about 3 % of the pixels set to the ignore label 255, the logits unit noise plus 3 at the target class (so the predicted
maps are mostly uniform regions too, as label maps are).  Per input: ``MulticlassConfusionMatrix(C, ignore_index=255)
.update`` and ``MulticlassAccuracy(C, average="macro", ignore_index=255).update``; one ``top_k=5`` accuracy row against
the ``torch.topk`` + label-histogram path.  Times are device events around one call, 5 warm-up calls, the median of
``--calls`` (>= 30).

``TM_AMD_MC_DENSE`` is read once per process, so the parent (which never opens the GPU) starts one child process per
setting and alternates them: new, old, new, old, ... (``--lds-kb K`` adds the new kernels with
``TM_AMD_MC_DENSE_LDS_KB=K`` as a third setting: LDS histogram against global atomics for large C).  Each child also times a device-to-device copy of a 512 MB buffer
(read + written bytes over time); ``floor`` = input bytes / that bandwidth, ``x_floor`` = update time / floor.  The raw
child lines go to ``--out``; the summary lines (medians over the rounds, the old path's round-to-round spread, whether
the two paths left identical metric states) are printed and appended to it.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
INPUTS = [  # (N, C, H, W, dtype, top_k)
    (8, 19, 512, 1024, "bfloat16", 1),
    (8, 19, 512, 1024, "float32", 1),
    (8, 150, 512, 512, "bfloat16", 1),
    (16, 21, 512, 512, "float16", 1),
    (256, 19, 24, 24, "bfloat16", 1),  # X = 576: just above the smallest X that mc_update sends to the dense kernels
    (8, 19, 512, 1024, "bfloat16", 5),
]


def child(calls: int) -> None:
    import torch

    import torchmetrics_amd as tm
    from torchmetrics_amd import ops

    dense = os.environ.get("TM_AMD_MC_DENSE", "1") != "0"
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)

    def timed(fn):
        for _ in range(5):
            fn()
        ts = []
        for _ in range(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return statistics.median(ts)

    src = torch.empty(512 << 20, dtype=torch.uint8, device=dev).fill_(1)
    dst = torch.empty_like(src)
    copy_us = timed(lambda: dst.copy_(src))
    copy_tbps = 2 * src.numel() / copy_us / 1e6
    del src, dst
    print(json.dumps({"dense": dense, "case": "copy 512 MB", "us": round(copy_us, 1), "TBps": round(copy_tbps, 3)}),
          flush=True)

    for n, c, h, w, dtype, top_k in INPUTS:
        t = torch.randint(0, c, (n, h // 8, w // 8) if h < 64 else (n, h // 16, w // 16), device=dev, generator=g)
        t = t.repeat_interleave(h // t.shape[1], 1).repeat_interleave(w // t.shape[2], 2).contiguous()
        p = torch.randn(n, c, h, w, device=dev, generator=g, dtype=getattr(torch, dtype))
        p.scatter_add_(1, t.unsqueeze(1), torch.full((n, 1, h, w), 3.0, device=dev, dtype=p.dtype))
        t[torch.rand(t.shape, device=dev, generator=g) < 0.03] = 255
        nbytes = p.numel() * p.element_size() + t.numel() * 8
        metrics = [("acc_top5", tm.MulticlassAccuracy(c, top_k=5, average="macro", ignore_index=255))] if top_k > 1 else [
            ("confmat", tm.MulticlassConfusionMatrix(c, ignore_index=255)),
            ("acc_macro", tm.MulticlassAccuracy(c, average="macro", ignore_index=255))]
        saved = ops.mc_dense_update
        if top_k > 1 and not dense:
            ops.mc_dense_update = lambda *a, **k: False  # torch.topk labels + the label histogram kernel
        try:
            for name, m in metrics:
                m = m.to(dev)
                us = timed(lambda: m.update(p, t))
                state = hashlib.sha1(m.compute().cpu().numpy().tobytes()).hexdigest()[:12]
                floor_us = nbytes / copy_tbps / 1e6
                print(json.dumps({"dense": dense, "case": f"{n}x{c}x{h}x{w} {dtype}", "kind": name,
                                  "us": round(us, 1), "TBps": round(nbytes / us / 1e6, 3),
                                  "x_floor": round(us / floor_us, 2), "state": state}), flush=True)
        finally:
            ops.mc_dense_update = saved
        del p, t


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3, help="child processes per setting, alternated new / old")
    ap.add_argument("--lds-kb", type=int, default=None, help="also time TM_AMD_MC_DENSE_LDS_KB=<this>")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mc_dense_bench.jsonl"))
    a = ap.parse_args()
    if a.child:
        child(max(30, a.calls))
        return
    settings = [("new", {"TM_AMD_MC_DENSE": "1"}), ("old", {"TM_AMD_MC_DENSE": "0"})]
    if a.lds_kb is not None:  # a third alternated setting: the dense kernels with a smaller LDS-histogram limit
        settings.append((f"new_lds{a.lds_kb}", {"TM_AMD_MC_DENSE": "1", "TM_AMD_MC_DENSE_LDS_KB": str(a.lds_kb)}))
    rows = []
    for r in range(a.rounds):
        for variant, knobs in settings:
            env = dict(os.environ, PYTHONPATH=str(ROOT), **knobs)
            res = subprocess.run([sys.executable, __file__, "--child", "--calls", str(a.calls)], env=env, cwd=ROOT,
                                 capture_output=True, text=True, timeout=420)
            if res.returncode != 0:  # nothing more is started on the GPU after a failed child
                sys.stderr.write(res.stdout + res.stderr)
                raise SystemExit(f"child ({variant}, round {r}) exited with {res.returncode}")
            rows += [dict(json.loads(line), variant=variant, round=r) for line in res.stdout.splitlines()
                     if line.startswith("{")]
            print(f"# round {r}: {variant} done", file=sys.stderr, flush=True)
    out = [json.dumps(row) for row in rows]
    for case, kind in sorted({(row["case"], row["kind"]) for row in rows if "kind" in row}):
        sel = {v: [row for row in rows if row.get("kind") == kind and row["case"] == case and row["variant"] == v]
               for v, _ in settings}
        us = {v: [row["us"] for row in sel[v]] for v in sel}
        med = {v: statistics.median(us[v]) for v in us}
        out.append(json.dumps({
            "summary": case, "kind": kind, "median_us": med, "speedup": round(med["old"] / med["new"], 2),
            "old_spread": round((max(us["old"]) - min(us["old"])) / min(us["old"]), 3), "runs_us": us,
            "new_x_floor": statistics.median(row["x_floor"] for row in sel["new"]),
            "same_state": len({row["state"] for v in sel for row in sel[v]}) == 1}))
        print(out[-1], flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
