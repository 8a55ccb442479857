"""The step guard and the per-tensor statistics (``csrc/health.hip``) against the plain fused update
launch on the flat buffers of the benchmark models, and the mlm256 step with the guard off, on, and
on with statistics due on every step.  Writes ``profiles/step_guard.md``.  Nothing here asserts a
budget: the numbers are recorded.

(a) kernel level, as ``tools/ema_bench.py``: hipGraph replays of ``--inner`` launches in windows of
    at least ``--window`` seconds, alternating rounds, median [min, max]:
    ``update`` (the plain AdamW launch), ``guarded update`` (the same launch with the guard's words),
    ``sumsq + step_guard``, ``tensor_stats`` due and not due (two launches each).
(b) step level: the mlm256 benchmark step (``StepEngine``, captured graph) with ``skip_nonfinite`` off,
    on, and on with ``tensor_stats`` requested before every step.  ``--parent-step-us`` (the parent
    commit's step, measured by its ``tools/ema_bench.py`` "off" side — the same loop — in the same
    session on the same box) is set against the guard-off figure in the report.

    python tools/step_guard_bench.py [--rounds 5] [--window 0.5] [--inner 20] [--parent-step-us X]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the benchmark's own model builders; not changed)
from tools.ema_bench import KERNEL_CONFIGS, _ab, _graph_of, _shapes, _window  # noqa: E402

KERNEL_SIDES = ("update", "guarded update", "sumsq + step_guard", "tensor_stats due", "tensor_stats not due")
STEP_SIDES = (("guard off", {}), ("guard on", {"skip_nonfinite": True}),
              ("guard on + stats every step", {"skip_nonfinite": True, "tensor_stats": True}))


def bench_kernels(a):
    from perceiver_io_amd.ops import ext
    from perceiver_io_amd.ops.optim import FusedAdamW

    K = ext.require()
    rows = []
    for config in KERNEL_CONFIGS:
        shapes = _shapes(config)
        g = torch.Generator().manual_seed(0)
        params = [torch.nn.Parameter((torch.randn(*s, generator=g) * 0.05).cuda()) for s in shapes]
        opt = FusedAdamW(params, lr=1e-6, weight_decay=0.01, skip_nonfinite=True, tensor_stats=True)
        f = opt.flat
        f.grad.copy_(torch.randn(f.numel, generator=g) * 1e-2)
        opt.stage_hyper()
        due = opt.hyper.clone()
        due[6] = 1.0
        K.sumsq(f.grad, opt.norm_part)
        K.step_guard(opt.norm_part, opt.hyper, opt.guard, 1.0)
        torch.cuda.synchronize()
        assert opt.health()["skipped"] == 0
        grp = opt.param_groups[0]

        def update(**kw):
            K.adamw(f.data, f.grad, opt.exp_avg, opt.exp_avg_sq, f.shadow, opt.hyper, grp["eps"], grp["weight_decay"], 0.0,
                    1.0, **kw)

        def guard():
            K.sumsq(f.grad, opt.norm_part)
            K.step_guard(opt.norm_part, opt.hyper, opt.guard, 1.0)

        def stats(hyper):
            K.tensor_stats(f.grad, f.data, hyper, opt.chunk_tab, opt.stats_tensor_tab, opt.stats_part, opt.stats, 1.0,
                           guard=opt.guard, skip_stats=opt.skip_stats)

        graphs = {"update": _graph_of(update, a.inner),
                  "guarded update": _graph_of(lambda: update(guard=opt.guard), a.inner),
                  "sumsq + step_guard": _graph_of(guard, a.inner),
                  "tensor_stats due": _graph_of(lambda: stats(due), a.inner),
                  "tensor_stats not due": _graph_of(lambda: stats(opt.hyper), a.inner)}
        for gr in graphs.values():  # warm-up
            _window(gr, a.inner, 0.05)
        r = _ab(graphs, lambda gr: _window(gr, a.inner, a.window), a.rounds)
        assert torch.isfinite(f.data).all() and opt.health()["skipped"] == 0
        rows.append(dict(config=config, numel=f.numel, tensors=len(params), us=r))
        print(f"{config:9s} numel {f.numel:9d}: " + "  ".join(f"{k} {r[k][0]:7.1f} us" for k in KERNEL_SIDES), flush=True)
        del opt, graphs, params
        torch.cuda.empty_cache()
    return rows


def bench_step(a):
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops.optim import FusedAdamW
    from perceiver_io_amd.train.engine import StepEngine

    ops.set_backend("auto")
    dev = torch.device("cuda", torch.cuda.current_device())
    args = bench.parse(["--config", "mlm256"])
    sides = {}
    for name, kw in STEP_SIDES:
        torch.manual_seed(1234)
        lit, loss_fn, make_batch, _, lr, _ = bench.build(args, dev)
        lit.to(dev)
        opt = FusedAdamW([p for p in lit.model.parameters() if p.requires_grad], lr=lr, weight_decay=0.01, **kw)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=lr, total_steps=50000, pct_start=0.1,
                                                    cycle_momentum=False)
        eng = StepEngine(loss_fn, opt, sched, device=dev, graph=True)
        g = torch.Generator(device="cpu").manual_seed(99)
        data = [tuple(t.to(dev) for t in make_batch(g)) for _ in range(4)]
        sides[name] = (eng, data, lit)
        for i in range(8):
            _step(sides[name], i)
        torch.cuda.synchronize()
        assert eng.replays > 0

    def measure(side):
        n = 16
        while True:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                loss = _step(side, i)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert torch.isfinite(loss).item()
            if dt >= a.window:
                return dt * 1e6 / n
            n *= 2

    r = _ab(sides, measure, a.rounds)
    ops.check_device_errors()
    for name, kw in STEP_SIDES:
        opt = sides[name][0].opt
        assert not kw or opt.health()["skipped"] == 0
        assert not kw.get("tensor_stats") or bool((opt.tensor_stats()[:, 0] > 0).any())
    print("mlm256 step: " + "  ".join(f"{n} {r[n][0]:8.1f} us [{r[n][1]:.1f}, {r[n][2]:.1f}]" for n, _ in STEP_SIDES),
          flush=True)
    return r


def _step(side, i):
    eng, data = side[0], side[1]
    if eng.opt.track_stats:
        eng.opt.request_stats()
    return eng.step(data[i % 4], ring_view=True)


def report(a, rows, step):
    cell = lambda v: f"{v[0]:.1f} [{v[1]:.1f}, {v[2]:.1f}]"  # noqa: E731
    out = ["# Step guard and per-tensor statistics (`csrc/health.hip`) against the fused update", "",
           f"Written by `tools/step_guard_bench.py` on {torch.cuda.get_device_name(0)}: hipGraph replays of {a.inner} "
           f"launches, windows ≥ {a.window} s between device events, {a.rounds} alternating rounds, median [min, max] in "
           "µs.  All numbers of a table come from one process on one device.  No budget is asserted: these overheads "
           "had not been measured before.", "",
           "## Kernel level", "",
           "`update` is the plain single-group AdamW launch, `guarded update` the same launch reading the guard's "
           "words (a step that is not skipped); `tensor_stats` is two launches (per chunk, per tensor) that return "
           "before any load when neither due nor skipped.", "",
           "| flat buffer | elements | tensors | " + " | ".join(KERNEL_SIDES) + " |", "|---|---|---|" + "---|" * len(KERNEL_SIDES)]
    for r in rows:
        out.append(f"| {r['config']} | {r['numel']} | {r['tensors']} | " + " | ".join(cell(r["us"][k]) for k in KERNEL_SIDES) + " |")
    out += ["", "Back-to-back replays keep the small buffers in the cache hierarchy; at the mlm256 and imagenet sizes "
            "the times are launch and drain latency, the lartpc row is the streaming comparison.", ""]
    if step is None:
        out += ["## Step level", "", "Not measured in this run (`--no-step`).", ""]
    else:
        off = step["guard off"]
        out += ["## Step level (mlm256, batch 64 × 512, captured step, one GPU)", "",
                "\"guard off\" holds no launch, buffer or hyper word more than the step before this feature.", "",
                "| step | µs per step | against guard off |", "|---|---|---|"]
        for name, _ in STEP_SIDES:
            s = step[name]
            out.append(f"| {name} | {cell(s)} | {s[0] - off[0]:+.1f} µs ({(s[0] / off[0] - 1) * 100:+.2f} %) |")
        on = step["guard on"][0] / off[0] - 1
        out.append("")
        if on > 0.02:
            k = next(r for r in rows if r["config"] == "mlm256")["us"]
            out.append(f"Guard on costs {on * 100:.2f} % over guard off, more than the 1–2 % box-to-box spread.  The added "
                       f"launches are `sumsq` + `step_guard` ({k['sumsq + step_guard'][0]:.1f} µs back to back at this size; "
                       f"the guarded update itself costs {k['guarded update'][0] - k['update'][0]:+.1f} µs over the plain "
                       "one): the step's tail is a serial chain, so each added launch adds its launch and drain latency.")
        else:
            out.append(f"Guard on costs {on * 100:+.2f} % over guard off, within the 1–2 % box-to-box spread.")
        out.append("")
        if a.parent_step_us:
            p = a.parent_step_us
            out += [f"The parent commit's mlm256 step, measured in the same session on the same box by its "
                    f"`tools/ema_bench.py` \"off\" side (the same loop): {p:.1f} µs; guard off here: {off[0]:.1f} µs "
                    f"({(off[0] / p - 1) * 100:+.2f} %).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print(f"wrote {a.out}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (at least)")
    ap.add_argument("--inner", type=int, default=20, help="launches per captured graph")
    ap.add_argument("--no-step", action="store_true", help="kernel level only")
    ap.add_argument("--parent-step-us", type=float, default=0.0, help="the parent commit's mlm256 step of this session")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_guard.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("step_guard_bench needs a GPU: timings from anything else say nothing")
    from perceiver_io_amd.ops import ext

    ext.require()
    rows = bench_kernels(a)
    step = None if a.no_step else bench_step(a)
    report(a, rows, step)


if __name__ == "__main__":
    main()
