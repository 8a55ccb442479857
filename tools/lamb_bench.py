"""Fused LAMB (``csrc/lamb.hip``: moments pass, trust reduction, apply pass) against the fused
AdamW launch (``adamw4_kernel``) on flat buffers of the benchmark models, and the mlm256 step with
either optimizer.  Writes ``profiles/lamb.md``.

(a) kernel level: the parameter shapes of the models ``bench.build`` constructs for ``mlm256``,
    ``imagenet`` and ``lartpc`` are laid out in a ``FlatParameterSpace`` (fp32 + bf16 shadow);
    ``--inner`` optimizer updates are captured in one hipGraph per side and replayed in windows of
    at least ``--window`` seconds between two device events.  The sides alternate in ``--rounds``
    rounds; the median round is reported with the min–max spread.
(b) step level: the mlm256 benchmark step (``StepEngine``, captured graph, bench batch) with
    ``FusedLamb`` against ``FusedAdamW``: wall time per step over windows of at least ``--window``
    seconds, alternating, same process.

    python tools/lamb_bench.py [--rounds 5] [--window 0.5] [--inner 20] [--out profiles/lamb.md]
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
# streamed bytes per element: AdamW reads p g m v (16), writes m v p (12) + shadow (2);
# LAMB pass 1 reads p g m v (16), writes m v (8); pass 2 reads p m v (12), writes p (4) + shadow (2)
ADAMW_BYTES, LAMB_BYTES = 30, 42


def _shapes(config):
    args = bench.parse(["--config", config])
    lit = bench.build(args, torch.device("cpu"))[0]
    model = lit.model
    params = model.trained_parameters() if config == "lartpc" else [p for p in model.parameters() if p.requires_grad]
    return [tuple(p.shape) for p in params]


def _optimizer(cls, shapes, **kw):
    g = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter((torch.randn(*s, generator=g) * 0.05).cuda()) for s in shapes]
    opt = cls(params, lr=1e-6, **kw)
    opt.flat.grad.copy_(torch.randn(opt.flat.numel, generator=g) * 1e-2)
    for p, o in zip(opt.flat.params, opt.flat.offsets):  # padding of the gradient stays zero
        end = o + p.numel()
        opt.flat.grad[end:(end + 63) // 64 * 64].zero_()
    opt.stage_hyper()
    return opt


def _graph_of(opt, inner):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        opt.device_update()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            opt.device_update()
    return g


def _window(graph, inner, seconds):
    """µs per update: replays between two device events until the window is at least ``seconds``"""
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
    from perceiver_io_amd.ops.optim import LAMB_CHUNK, FusedAdamW, FusedLamb

    rows = []
    for config in KERNEL_CONFIGS:
        shapes = _shapes(config)
        opts = {"adamw": _optimizer(FusedAdamW, shapes, weight_decay=0.01),
                "lamb": _optimizer(FusedLamb, shapes, weight_decay=0.01)}
        graphs = {n: _graph_of(o, a.inner) for n, o in opts.items()}
        for g in graphs.values():  # warm-up
            _window(g, a.inner, 0.05)
        r = _ab(graphs, lambda g: _window(g, a.inner, a.window), a.rounds)
        lamb = opts["lamb"]
        assert torch.isfinite(lamb.flat.data).all() and torch.isfinite(lamb.last_trust()).all()
        n = lamb.flat.numel
        row = dict(config=config, numel=n, tensors=len(shapes), chunks=int(lamb.chunk_tab.shape[0]), us=r,
                   ratio=r["lamb"][0] / r["adamw"][0],
                   gbps={k: (LAMB_BYTES if k == "lamb" else ADAMW_BYTES) * n / (r[k][0] * 1e-6) / 1e9 for k in r})
        rows.append(row)
        print(f"{config:9s} numel {n:9d} tensors {len(shapes):4d} chunks {row['chunks']:5d} (LAMB_CHUNK {LAMB_CHUNK}): "
              f"adamw {r['adamw'][0]:7.1f} us [{r['adamw'][1]:.1f}, {r['adamw'][2]:.1f}]  "
              f"lamb {r['lamb'][0]:7.1f} us [{r['lamb'][1]:.1f}, {r['lamb'][2]:.1f}]  ratio {row['ratio']:.2f}", flush=True)
        del opts, graphs
        torch.cuda.empty_cache()
    return rows


def bench_step(a):
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops.optim import FusedAdamW, FusedLamb
    from perceiver_io_amd.train.engine import StepEngine

    ops.set_backend("auto")
    dev = torch.device("cuda", torch.cuda.current_device())
    args = bench.parse(["--config", "mlm256"])
    sides = {}
    for name, cls in (("adamw", FusedAdamW), ("lamb", FusedLamb)):
        torch.manual_seed(1234)
        lit, loss_fn, make_batch, _, lr, _ = bench.build(args, dev)
        lit.to(dev)
        opt = cls([p for p in lit.model.parameters() if p.requires_grad], lr=lr, weight_decay=0.01)
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
    print(f"mlm256 step: adamw {r['adamw'][0]:8.1f} us [{r['adamw'][1]:.1f}, {r['adamw'][2]:.1f}]  "
          f"lamb {r['lamb'][0]:8.1f} us [{r['lamb'][1]:.1f}, {r['lamb'][2]:.1f}]", flush=True)
    return r


def report(a, rows, step):
    from perceiver_io_amd.ops.optim import LAMB_CHUNK

    out = ["# Fused LAMB (`csrc/lamb.hip`) against the fused AdamW launch", "",
           f"Written by `tools/lamb_bench.py` on {torch.cuda.get_device_name(0)}: hipGraph replays of {a.inner} updates, "
           f"windows ≥ {a.window} s between device events, {a.rounds} alternating rounds, median [min, max].", "",
           f"`LAMB_CHUNK` = {LAMB_CHUNK} elements: one 256-thread block per chunk, 4 × 16-byte loads per array and "
           "thread, all in flight before the arithmetic.", "",
           "The trust ratios are a launch of their own (one block per tensor sums that tensor's chunk partials in "
           "fp64, fixed order).  Folded into pass 2, every chunk block would re-sum its tensor's partials: for the "
           "LArTPC query table (≈16.8 M elements, ≈4100 chunks) that is ≈4100 blocks × 4100 pairs ≈ 134 MB of extra "
           "L2 reads against ≈300 MB of streamed traffic for the pass itself, so the separate launch was chosen.", "",
           "## Kernel level", "",
           f"Byte model: AdamW {ADAMW_BYTES} B/element, LAMB {LAMB_BYTES} B/element (pass 1: 24, pass 2: 18) → "
           f"{LAMB_BYTES / ADAMW_BYTES:.2f}× when HBM-bound.", "",
           "| flat buffer | elements | tensors | chunks | AdamW µs | LAMB µs (3 launches) | ratio | AdamW GB/s | LAMB GB/s |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        ad, la = r["us"]["adamw"], r["us"]["lamb"]
        out.append(f"| {r['config']} | {r['numel']} | {r['tensors']} | {r['chunks']} | {ad[0]:.1f} [{ad[1]:.1f}, {ad[2]:.1f}] | "
                   f"{la[0]:.1f} [{la[1]:.1f}, {la[2]:.1f}] | {r['ratio']:.2f} | {r['gbps']['adamw']:.0f} | "
                   f"{r['gbps']['lamb']:.0f} |")
    out += ["", "Back-to-back replays of one update keep small buffers in the cache hierarchy: the GB/s columns are "
            "the byte model over the time, not HBM traffic.  At the mlm256 and imagenet sizes neither optimizer is "
            "bandwidth-bound: LAMB is three dependent launches against one, and the ratio there is launch and drain "
            "latency rather than bytes; the lartpc row is the streaming comparison.", ""]
    if step is not None:
        ad, la = step["adamw"], step["lamb"]
        out += ["## Step level (mlm256, batch 64 × 512, captured step, one GPU)", "",
                "| optimizer | µs per step |", "|---|---|",
                f"| FusedAdamW | {ad[0]:.1f} [{ad[1]:.1f}, {ad[2]:.1f}] |",
                f"| FusedLamb | {la[0]:.1f} [{la[1]:.1f}, {la[2]:.1f}] |", "",
                f"Difference: {la[0] - ad[0]:+.1f} µs per step ({(la[0] / ad[0] - 1) * 100:+.2f} %).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print(f"wrote {a.out}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (at least)")
    ap.add_argument("--inner", type=int, default=20, help="optimizer updates per captured graph")
    ap.add_argument("--no-step", action="store_true", help="kernel level only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lamb.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lamb_bench needs a GPU: timings from anything else say nothing")
    from perceiver_io_amd.ops import ext

    ext.require()
    rows = bench_kernels(a)
    step = None if a.no_step else bench_step(a)
    report(a, rows, step)


if __name__ == "__main__":
    main()
