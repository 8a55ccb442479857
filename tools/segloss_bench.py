#!/usr/bin/env python
"""Segmentation-loss benchmark: the ``pixel_seg_fwd`` + ``pixel_seg_bwd`` pair (focal cross-entropy
+ soft Dice on the fused LArTPC head) against the ``pixel_ce_fwd`` + ``pixel_ce_bwd`` pair it sits
beside, in one process on the same operands, and the LArTPC training step of ``run.py`` with the
loss off and on.  Writes the results as JSON (``--out``) and as the report
``profiles/seg_loss.md`` (``--md``).

Kernel pairs: 4 × 10,240 rows (four events at the LArTPC query capacity), C = 64, K = 3, every
fifth label ignored, background weight 0; γ ∈ {0, 2}, Dice off and on.  Times are device events
around back-to-back calls of the two bindings (launches plus their scratch allocation) after
``--warmup`` calls; every window lasts at least ``--window-ms``, and the configurations alternate
over ``--rounds`` rounds (median, min - max), so drift hits all of them alike.

Training step: the captured hipGraph step over ``LArPerceiver.event_loss`` (512 × 512 events, batch
4, FusedAdam with L2 decay and clip, as ``run.py --device-collate``), one engine per loss, the
engines alternating; a host clock around ``--steps`` replays ending in a device synchronise.

Measuring needs a GPU (no CPU fallback); ``--render results.json --md report.md`` only rewrites the
report from saved results.

    python tools/segloss_bench.py --out profiles/seg_loss.json --md profiles/seg_loss.md
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CE = "pixel_ce"
# name → (γ, ce_weight, dice_weight, ε)
SEG = {"pixel_seg γ=0": (0.0, 1.0, 0.0, 1.0), "pixel_seg γ=2": (2.0, 1.0, 0.0, 1.0),
       "pixel_seg γ=0 + Dice": (0.0, 1.0, 0.5, 1.0), "pixel_seg γ=2 + Dice": (2.0, 1.0, 0.5, 1.0),
       "pixel_seg γ=1.5 + Dice": (1.5, 1.0, 0.5, 1.0)}


def timed(fn, warmup: int, window_ms: float):
    """(mean milliseconds per call, calls) over one window of at least ``window_ms``."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()

    def window(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / reps

    pilot = window(20)
    reps = max(20, math.ceil(1.1 * window_ms / max(pilot, 1e-4)))
    return window(reps), reps


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def measure_pairs(a, res):
    from perceiver_io_amd.ops import ext

    K = ext.require()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    R, C, NK = a.rows, 64, 3
    h = torch.randn(R, C, device=dev)
    W = torch.randn(NK, C, device=dev) * 0.3
    b = torch.randn(NK, device=dev) * 0.1
    lab = torch.randint(0, NK, (R,), device=dev)
    lab[::5] = -100
    wts = torch.tensor([0.0, 1.0, 1.0], device=dev)
    gout = torch.ones(1, device=dev)
    dH, dW, db = torch.empty_like(h), torch.zeros_like(W), torch.zeros_like(b)

    def ce_pair():
        stats, _ = K.pixel_ce_fwd(h, W, b, lab, wts)
        K.pixel_ce_bwd(h, W, b, lab, wts, gout, stats, dH, dW, db)

    def seg_pair(p):
        def run():
            stats, _ = K.pixel_seg_fwd(h, W, b, lab, wts, *p)
            K.pixel_seg_bwd(h, W, b, lab, wts, *p, gout, stats, dH, dW, db)
        return run

    # results must not change: γ = 0 without Dice is the weighted cross-entropy
    l0 = K.pixel_ce_fwd(h, W, b, lab, wts)[1]
    l1 = K.pixel_seg_fwd(h, W, b, lab, wts, 0.0, 1.0, 0.0, 1.0)[1]
    res["gamma0_loss_vs_pixel_ce"] = [float(l1), float(l0)]
    paths = {CE: ce_pair, **{n: seg_pair(p) for n, p in SEG.items()}}
    rounds = {n: [] for n in paths}
    calls = {}
    for _ in range(a.rounds):
        for n, fn in paths.items():
            ms, calls[n] = timed(fn, a.warmup, a.window_ms)
            rounds[n].append(ms * 1e3)
    res["rows"], res["channels"], res["classes"] = R, C, NK
    res["pairs_us"] = {n: {**spread(v), "calls": calls[n]} for n, v in rounds.items()}


def measure_step(a, res):
    from perceiver_io_amd import ops
    from perceiver_io_amd.data.lartpc import DenseCollator, sparse_collate
    from perceiver_io_amd.data.synthetic import lartpc_event
    from perceiver_io_amd.models.lartpc import LArPerceiver, SegLoss, class_weights
    from perceiver_io_amd.ops.optim import FusedAdam
    from perceiver_io_amd.train.engine import StepEngine

    dev = torch.device("cuda")
    events = [lartpc_event(i, a.size) for i in range(a.batch)]
    shapes = sparse_collate(events, bucket=2048)
    kcap, qcap = shapes[0].shape[1], shapes[3].shape[1]
    img, lab = DenseCollator()(events)
    batch = (img.to(dev), lab.to(dev), torch.zeros(a.batch, dtype=torch.int32, device=dev))
    w = class_weights(dev)
    engines = {}
    with ops.backend("hip"):
        for name, cfg in (("weighted CE (pixel_ce)", None), ("focal γ=2 + 0.5 Dice (pixel_seg)", SegLoss(2.0, 1.0, 0.5, 1.0))):
            torch.manual_seed(0)
            model = LArPerceiver(a.size).to(dev)
            opt = FusedAdam(model.trained_parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=10.0)
            fn = (lambda m, c: lambda bt: m.event_loss(bt, w, kcap, qcap, loss=c)[0])(model, cfg)
            eng = StepEngine(fn, opt, device=dev, graph=True, warmup_eager=0)
            for _ in range(a.warmup):
                eng.step(batch)
            engines[name] = eng
        rounds = {n: [] for n in engines}
        for _ in range(a.rounds):
            for n, eng in engines.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    eng.step(batch)
                torch.cuda.synchronize()
                rounds[n].append((time.perf_counter() - t0) / a.steps * 1e3)
    res["step"] = {"size": a.size, "batch": a.batch, "key_capacity": kcap, "query_capacity": qcap, "steps": a.steps}
    res["step_ms"] = {n: spread(v) for n, v in rounds.items()}


def measure(a):
    if not torch.cuda.is_available():
        raise SystemExit("segloss_bench needs a GPU")
    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "window_ms": a.window_ms, "rounds": a.rounds}
    measure_pairs(a, res)
    if not a.no_step:
        measure_step(a, res)
    return res


def render(res) -> str:
    pairs = res["pairs_us"]
    base = pairs[CE]["median"]
    out = ["# Focal + soft-Dice loss on the fused LArTPC head", "",
           f"Measured by `tools/segloss_bench.py` on {res['device']}: device events around back-to-back calls, "
           f"{res['warmup']} warm-up calls, windows of at least {res['window_ms']:g} ms, {res['rounds']} alternating "
           "rounds (median, min – max).", "",
           "## Kernel pairs", "",
           f"Forward + backward of the head and its loss, {res['rows']:,} rows × {res['channels']} channels, "
           f"K = {res['classes']}: per call pair of the two bindings (row kernel, finalize; row kernel, "
           "`pixel_ce_wgrad_kernel`; scratch allocation).  Both pairs read `h` twice and write `dH` once.", "",
           "| pair | µs per fwd + bwd | vs `pixel_ce` |", "|---|---|---|"]
    for n, v in pairs.items():
        out.append(f"| `{n}` | {v['median']:.1f} ({v['min']:.1f} – {v['max']:.1f}; {v['calls']} calls / window) | "
                   f"{v['median'] / base:.2f}× |")
    l1, l0 = res["gamma0_loss_vs_pixel_ce"]
    out += ["", f"γ = 0 without Dice computes the weighted cross-entropy: loss {l1:.7f} against `pixel_ce_fwd`'s {l0:.7f}."]
    if "step_ms" in res:
        s = res["step"]
        steps = res["step_ms"]
        names = list(steps)
        out += ["", "## Training step", "",
                f"The captured step of `run.py --device-collate` ({s['size']} × {s['size']} events, batch {s['batch']}, "
                f"{s['key_capacity']:,} key and {s['query_capacity']:,} query slots per event), host clock around "
                f"{s['steps']} replays ending in a device synchronise, the two engines alternating.", "",
                "| loss | ms per step |", "|---|---|"]
        for n in names:
            v = steps[n]
            out.append(f"| {n} | {v['median']:.3f} ({v['min']:.3f} – {v['max']:.3f}) |")
        out += ["", f"Ratio of the medians: {steps[names[1]]['median'] / steps[names[0]]['median']:.3f}."]
    return "\n".join(out) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=4 * 10240)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50, help="replays per timed window of the training step")
    ap.add_argument("--no-step", action="store_true", help="kernel pairs only")
    ap.add_argument("--out", default=None, help="results as JSON")
    ap.add_argument("--md", default=None, help="report as markdown")
    ap.add_argument("--render", default=None, metavar="JSON", help="rewrite --md from saved results (no GPU)")
    a = ap.parse_args(argv)
    if a.render:
        with open(a.render) as f:
            res = json.load(f)
    else:
        res = measure(a)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
    text = render(res)
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
