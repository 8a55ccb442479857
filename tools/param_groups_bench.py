"""The grouped AdamW launch (``adamw_grouped_kernel``, csrc/elementwise.hip) against the
single-group launch (``adamw4_kernel``) on flat buffers of the benchmark models, and the seq_clf_ft
step with and without parameter groups.  Writes ``profiles/param_groups.md`` (a hand-written
``## Notes`` section at the end of an existing report is kept).

(a) kernel level: the parameter shapes of the models ``bench.build`` constructs for ``mlm256``,
    ``seq_clf_ft`` and ``lartpc`` in a ``FlatParameterSpace`` (fp32 + bf16 shadow); one group against
    G = 2 (1-d tensors undecayed) and G = 4 (that split × tensor parity with another lr), measured as
    in ``tools/lamb_bench.py``: ``--inner`` updates per captured hipGraph, windows of at least
    ``--window`` seconds between two device events, ``--rounds`` alternating rounds, median with the
    min–max spread.  The yardstick is the single-group launch on the same buffer in the same
    process, its spread the margin.
(b) step level: the seq_clf_ft benchmark step (``StepEngine``, captured graph, bench batch) with
    one group against the groups of ``--model.no_decay_1d=true --model.encoder_lr_scale=0.1``.

    python tools/param_groups_bench.py [--rounds 5] [--window 0.5] [--inner 20]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402  (the benchmark's own model builders; not changed)
from lamb_bench import ADAMW_BYTES, _ab, _graph_of, _shapes, _window  # noqa: E402

KERNEL_CONFIGS = ("mlm256", "seq_clf_ft", "lartpc")
SIDES = ("one group", "G = 2", "G = 4")
NOTES = "## Notes"  # report(): an existing report's text from this heading on is kept


def _groups(params, G):
    """G = 1: one group; 2: ndim ≤ 1 undecayed; 4: that split × tensor parity at a tenth of the lr."""
    if G == 1:
        return [{"params": params}]
    key = (lambda i, p: int(p.dim() <= 1)) if G == 2 else (lambda i, p: 2 * (i % 2) + int(p.dim() <= 1))
    out = [{"params": [], "weight_decay": 0.0 if j % 2 else 0.01, "lr": 1e-6 * (0.1 if j >= 2 else 1.0)} for j in range(G)]
    for i, p in enumerate(params):
        out[key(i, p)]["params"].append(p)
    return [g for g in out if g["params"]]


def _optimizer(shapes, G):
    from perceiver_io_amd.ops.optim import FusedAdamW

    g = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter((torch.randn(*s, generator=g) * 0.05).cuda()) for s in shapes]
    opt = FusedAdamW(_groups(params, G), lr=1e-6, weight_decay=0.01)
    opt.flat.grad.copy_(torch.randn(opt.flat.numel, generator=g) * 1e-2)
    for p, o in zip(opt.flat.params, opt.flat.offsets):  # padding of the gradient stays zero
        end = o + p.numel()
        opt.flat.grad[end:(end + 63) // 64 * 64].zero_()
    opt.stage_hyper()
    return opt


def bench_kernels(a):
    rows = []
    for config in KERNEL_CONFIGS:
        shapes = _shapes(config)
        opts = {n: _optimizer(shapes, G) for n, G in zip(SIDES, (1, 2, 4))}
        assert [len(o.param_groups) for o in opts.values()] == [1, 2, 4], config
        graphs = {n: _graph_of(o, a.inner) for n, o in opts.items()}
        for g in graphs.values():  # warm-up
            _window(g, a.inner, 0.05)
        r = _ab(graphs, lambda g: _window(g, a.inner, a.window), a.rounds)
        assert all(torch.isfinite(o.flat.data).all() for o in opts.values())
        n = opts[SIDES[0]].flat.numel
        row = dict(config=config, numel=n, tensors=len(shapes), chunks=int(opts[SIDES[1]].chunk_tab.shape[0]), us=r,
                   gbps={k: ADAMW_BYTES * n / (r[k][0] * 1e-6) / 1e9 for k in r})
        rows.append(row)
        print(f"{config:10s} numel {n:9d} tensors {len(shapes):4d} chunks {row['chunks']:5d}: " + "  ".join(
            f"{k} {r[k][0]:7.1f} us [{r[k][1]:.1f}, {r[k][2]:.1f}]" for k in SIDES), flush=True)
        del opts, graphs
        torch.cuda.empty_cache()
    return rows


def bench_step(a):
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops.optim import FusedAdamW
    from perceiver_io_amd.train.engine import StepEngine

    ops.set_backend("auto")
    dev = torch.device("cuda", torch.cuda.current_device())
    args = bench.parse(["--config", "seq_clf_ft"])
    sides = {}
    for name, grouped in (("one group", False), ("no_decay_1d + encoder_lr_scale=0.1", True)):
        torch.manual_seed(1234)
        lit, loss_fn, make_batch, _, lr, wd = bench.build(args, dev)
        lit.to(dev)
        if grouped:
            lit.hparams["no_decay_1d"], lit.hparams["encoder_lr_scale"] = True, 0.1
            groups = lit.optimizer_groups()
            assert len(groups) == 4
        else:
            groups = [p for p in lit.model.parameters() if p.requires_grad]
        opt = FusedAdamW(groups, lr=lr, weight_decay=wd)
        eng = StepEngine(loss_fn, opt, None, device=dev, graph=True)
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
    print("seq_clf_ft step: " + "  ".join(f"{k} {v[0]:8.1f} us [{v[1]:.1f}, {v[2]:.1f}]" for k, v in r.items()), flush=True)
    return r


def report(a, rows, step):
    from perceiver_io_amd.ops.optim import LAMB_CHUNK

    out = ["# Grouped AdamW (`adamw_grouped_kernel`) against the single-group launch (`adamw4_kernel`)", "",
           f"Written by `tools/param_groups_bench.py` on {torch.cuda.get_device_name(0)}: hipGraph replays of {a.inner} "
           f"updates, windows ≥ {a.window} s between device events, {a.rounds} alternating rounds, median [min, max].", "",
           f"The grouped kernel walks the chunk table of the LAMB update (chunks of ≤ {LAMB_CHUNK} elements at tensor "
           "boundaries) with at most 2048 workgroups, 4 × 16-byte loads per array and thread in flight before the "
           "arithmetic, and reads lr / weight decay / eps of the chunk's group from `hyper[8 + 4j]`.  G = 2: 1-d tensors "
           "undecayed; G = 4: that split × tensor parity at a tenth of the lr.  The yardstick is the single-group launch "
           "on the same buffer in the same process; its min–max spread is the margin.", "",
           "## Kernel level", "",
           f"Byte model: {ADAMW_BYTES} B/element on both sides (the tables add 24 B per chunk and 4 B per tensor).", "",
           "| flat buffer | elements | tensors | chunks | one group µs | G = 2 µs | G = 4 µs | one group GB/s | G = 2 GB/s | G = 4 GB/s |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for r in rows:
        us = r["us"]
        out.append(f"| {r['config']} | {r['numel']} | {r['tensors']} | {r['chunks']} | "
                   + " | ".join(f"{us[k][0]:.1f} [{us[k][1]:.1f}, {us[k][2]:.1f}]" for k in SIDES) + " | "
                   + " | ".join(f"{r['gbps'][k]:.0f}" for k in SIDES) + " |")
        one = us[SIDES[0]]
        spread = one[2] - one[1]
        for k in SIDES[1:]:
            over = us[k][0] - one[2]
            verdicts.append(f"- {r['config']}, {k}: median {us[k][0]:.1f} µs against the slowest single-group repeat "
                            f"{one[2]:.1f} µs (spread {spread:.1f} µs): "
                            + (f"**outside the margin by {over - spread:.1f} µs**" if over > spread else "within the margin"))
    out += ["", "Back-to-back replays of one update keep small buffers in the cache hierarchy: the GB/s columns are the "
            "byte model over the time, not HBM traffic; the lartpc row is the streaming comparison.", "",
            "Grouped median against the single-group spread:", ""] + verdicts + [""]
    if step is not None:
        out += ["## Step level (seq_clf_ft, batch 128 × 512, captured step, one GPU)", "",
                "| parameter groups | µs per step |", "|---|---|"]
        out += [f"| {k} | {v[0]:.1f} [{v[1]:.1f}, {v[2]:.1f}] |" for k, v in step.items()]
        (k0, v0), (k1, v1) = step.items()
        out += ["", f"Difference: {v1[0] - v0[0]:+.1f} µs per step ({(v1[0] / v0[0] - 1) * 100:+.2f} %).", ""]
    # whatever was written by hand below the "## Notes" heading of an earlier report stays
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = f.read()
        if NOTES in old:
            out += [old[old.index(NOTES):].rstrip("\n"), ""]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_groups.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("param_groups_bench needs a GPU: timings from anything else say nothing")
    from perceiver_io_amd.ops import ext

    ext.require()
    rows = bench_kernels(a)
    step = None if a.no_step else bench_step(a)
    report(a, rows, step)


if __name__ == "__main__":
    main()
