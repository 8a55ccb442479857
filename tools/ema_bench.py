"""Weight-EMA kernels (``csrc/ema.hip``: ``ema_update``, ``ema_swap``) against the fused AdamW
launch (``adamw4_kernel``) on the flat buffers of the benchmark models, and the mlm256 step with and
without an attached ``WeightEMA``.  Writes ``profiles/ema.md``.

(a) kernel level: the parameter shapes of the models ``bench.build`` constructs for ``mlm256``,
    ``imagenet`` and ``lartpc`` are laid out in a ``FlatParameterSpace`` (fp32 + bf16 shadow);
    ``--inner`` launches of each kernel are captured in one hipGraph per side and replayed in
    windows of at least ``--window`` seconds between two device events.  The sides alternate in
    ``--rounds`` rounds; the median round is reported with the min–max spread.
(b) step level: the mlm256 benchmark step (``StepEngine``, captured graph, bench batch, the
    engine ``bench.py`` runs) without an average — the step as it was before the EMA existed:
    ``hyper[5]`` stays 0 and nothing more is launched — against ``update_every`` = 1 and 4: wall
    time per step over windows of at least ``--window`` seconds, alternating, same process.

    python tools/ema_bench.py [--rounds 5] [--window 0.5] [--inner 20] [--out profiles/ema.md]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the benchmark's own model builders; not changed)

KERNEL_CONFIGS = ("mlm256", "imagenet", "lartpc")
# streamed bytes per element: AdamW reads p g m v (16), writes m v p (12) + shadow (2); the EMA
# update reads e w (8), writes e (4); the swap reads w e (8), writes w e (8) + shadow (2)
BYTES = {"adamw": 30, "ema_update": 12, "ema_swap": 18}


def _shapes(config):
    args = bench.parse(["--config", config])
    lit = bench.build(args, torch.device("cpu"))[0]
    model = lit.model
    params = model.trained_parameters() if config == "lartpc" else [p for p in model.parameters() if p.requires_grad]
    return [tuple(p.shape) for p in params]


def _graph_of(fn, inner):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    return g


def _window(graph, inner, seconds):
    """µs per launch: replays between two device events until the window is at least ``seconds``"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 4
    while True:
        e0.record()
        for _ in range(n):
            graph.replay()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= seconds * 1e3:
            return ms * 1e3 / (n * inner)
        n = max(n * 2, int(n * seconds * 1.2e3 / max(ms, 1e-3)))


def _ab(sides, measure, rounds):
    t = {n: [] for n in sides}
    for _ in range(rounds):
        for n, s in sides.items():
            t[n].append(measure(s))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in t.items()}


def bench_kernels(a):
    from perceiver_io_amd.ops import ext
    from perceiver_io_amd.ops.optim import FusedAdamW, WeightEMA

    K = ext.require()
    rows = []
    for config in KERNEL_CONFIGS:
        shapes = _shapes(config)
        g = torch.Generator().manual_seed(0)
        params = [torch.nn.Parameter((torch.randn(*s, generator=g) * 0.05).cuda()) for s in shapes]
        opt = FusedAdamW(params, lr=1e-6, weight_decay=0.01)
        f = opt.flat
        f.grad.copy_(torch.randn(f.numel, generator=g) * 1e-2)
        opt.stage_hyper()  # hyper[5] = 0: the AdamW side launches nothing else
        ema = WeightEMA(f, decay=0.9999, warmup=False)
        hyper = opt.hyper.clone()
        hyper[5] = ema.one_minus_decay(1)
        torch.cuda.synchronize()
        graphs = {"adamw": _graph_of(opt.device_update, a.inner),
                  "ema_update": _graph_of(lambda: K.ema_update(ema.avg, f.data, hyper), a.inner),
                  # an even number of swaps per graph: the buffers end where they started
                  "ema_swap": _graph_of(lambda: K.ema_swap(f.data, ema.avg, f.shadow), a.inner)}
        for gr in graphs.values():  # warm-up
            _window(gr, a.inner, 0.05)
        r = _ab(graphs, lambda gr: _window(gr, a.inner, a.window), a.rounds)
        assert torch.isfinite(f.data).all() and torch.isfinite(ema.avg).all()
        n = f.numel
        row = dict(config=config, numel=n, us=r, gbps={k: BYTES[k] * n / (r[k][0] * 1e-6) / 1e9 for k in r})
        rows.append(row)
        print(f"{config:9s} numel {n:9d}: " + "  ".join(
            f"{k} {r[k][0]:7.1f} us [{r[k][1]:.1f}, {r[k][2]:.1f}] {row['gbps'][k]:6.0f} GB/s" for k in r), flush=True)
        del opt, ema, graphs, params
        torch.cuda.empty_cache()
    return rows


STEP_SIDES = (("off", None), ("every step", 1), ("every 4th step", 4))


def bench_step(a):
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops.optim import FusedAdamW, WeightEMA
    from perceiver_io_amd.train.engine import StepEngine

    ops.set_backend("auto")
    dev = torch.device("cuda", torch.cuda.current_device())
    args = bench.parse(["--config", "mlm256"])
    sides = {}
    for name, every in STEP_SIDES:
        torch.manual_seed(1234)
        lit, loss_fn, make_batch, _, lr, _ = bench.build(args, dev)
        lit.to(dev)
        opt = FusedAdamW([p for p in lit.model.parameters() if p.requires_grad], lr=lr, weight_decay=0.01)
        if every is not None:
            opt.attach_ema(WeightEMA(opt.flat, decay=0.9999, warmup=True, update_every=every))
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=lr, total_steps=50000, pct_start=0.1,
                                                    cycle_momentum=False)
        eng = StepEngine(loss_fn, opt, sched, device=dev, graph=True)
        g = torch.Generator(device="cpu").manual_seed(99)
        data = [tuple(t.to(dev) for t in make_batch(g)) for _ in range(4)]
        for i in range(8):
            eng.step(data[i % 4], ring_view=True)
        torch.cuda.synchronize()
        assert eng.replays > 0
        sides[name] = (eng, data, lit)

    def measure(side):
        eng, data = side[0], side[1]
        n = 16
        while True:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                loss = eng.step(data[i % 4], ring_view=True)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert torch.isfinite(loss).item()
            if dt >= a.window:
                return dt * 1e6 / n
            n *= 2

    r = _ab(sides, measure, a.rounds)
    ops.check_device_errors()
    for name, _ in STEP_SIDES:
        ema = sides[name][0].opt.ema
        assert ema is None or (torch.isfinite(ema.avg).all() and not torch.equal(ema.avg, sides[name][0].opt.flat.data))
    print("mlm256 step: " + "  ".join(f"{n} {r[n][0]:8.1f} us [{r[n][1]:.1f}, {r[n][2]:.1f}]" for n, _ in STEP_SIDES),
          flush=True)
    return r


def report(a, rows, step):
    out = ["# Weight EMA (`csrc/ema.hip`) against the fused AdamW launch", "",
           f"Written by `tools/ema_bench.py` on {torch.cuda.get_device_name(0)}: hipGraph replays of {a.inner} launches, "
           f"windows ≥ {a.window} s between device events, {a.rounds} alternating rounds, median [min, max].  All "
           "numbers of this file come from one process on one device.", "",
           "## Kernel level", "",
           f"Byte model: AdamW {BYTES['adamw']} B/element, `ema_update` {BYTES['ema_update']} B/element, `ema_swap` "
           f"{BYTES['ema_swap']} B/element (with the bf16 shadow).", "",
           "| flat buffer | elements | AdamW µs | `ema_update` µs | `ema_swap` µs | update / AdamW | AdamW GB/s | "
           "`ema_update` GB/s | `ema_swap` GB/s |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        u = r["us"]
        cell = lambda k: f"{u[k][0]:.1f} [{u[k][1]:.1f}, {u[k][2]:.1f}]"  # noqa: E731
        out.append(f"| {r['config']} | {r['numel']} | {cell('adamw')} | {cell('ema_update')} | {cell('ema_swap')} | "
                   f"{u['ema_update'][0] / u['adamw'][0]:.2f} | {r['gbps']['adamw']:.0f} | "
                   f"{r['gbps']['ema_update']:.0f} | {r['gbps']['ema_swap']:.0f} |")
    out += ["", "Back-to-back replays of one launch keep small buffers in the cache hierarchy: the GB/s columns are "
            "the byte model over the time, not HBM traffic.  At the mlm256 and imagenet sizes no side is "
            "bandwidth-bound and the times are launch and drain latency; the lartpc row is the streaming "
            "comparison.", ""]
    if step is None:
        out += ["## Step level", "", "Not measured in this run (`--no-step`).", ""]
    else:
        off = step["off"]
        out += ["## Step level (mlm256, batch 64 × 512, captured step, one GPU)", "",
                "\"off\" is the step without an average: `hyper[5]` stays 0 and the captured graph holds no launch "
                "more than before the EMA existed, so it stands for the previous step time, measured here in the "
                "same process and alternating with the other sides.", "",
                "| weight EMA | µs per step | against off |", "|---|---|---|"]
        for name, _ in STEP_SIDES:
            s = step[name]
            out.append(f"| {name} | {s[0]:.1f} [{s[1]:.1f}, {s[2]:.1f}] | {s[0] - off[0]:+.1f} µs "
                       f"({(s[0] / off[0] - 1) * 100:+.2f} %) |")
        e1, e4 = step["every step"][0] - off[0], step["every 4th step"][0] - off[0]
        out += ["", f"`update_every=4` keeps the launch in the graph (it returns at once on three steps of four): it "
                f"costs {e4:+.1f} µs per step against {e1:+.1f} µs with an update on every step, i.e. it recovers "
                f"{e1 - e4:.1f} µs.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print(f"wrote {a.out}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (at least)")
    ap.add_argument("--inner", type=int, default=20, help="launches per captured graph (even: swaps pair up)")
    ap.add_argument("--no-step", action="store_true", help="kernel level only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema.md"))
    a = ap.parse_args()
    if a.inner % 2:
        raise SystemExit("--inner must be even: an odd number of swaps leaves the buffers exchanged")
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench needs a GPU: timings from anything else say nothing")
    from perceiver_io_amd.ops import ext

    ext.require()
    rows = bench_kernels(a)
    step = None if a.no_step else bench_step(a)
    report(a, rows, step)


if __name__ == "__main__":
    main()
