"""Whole-word masking (``text_mask_words_kernel``) against the token-level ``text_mask_kernel`` and
a ``copy_`` of the same bytes, and the mlm256 step with whole-word masking off and on.  Writes
``profiles/whole_word_masking.md``.

(a) kernel level, shapes (64, 512) and (8, 8192), ids uniform over the shipped vocabulary, 20 %
    padding: ``--inner`` launches of each side are captured in one hipGraph and replayed in
    windows of at least ``--window`` seconds between two device events.  The sides alternate in
    ``--rounds`` rounds; the median round is reported with the min–max spread.  Byte model per
    token: ids 8 + pad 1 read, masked ids 8 + labels 8 written = 25 B; the ``copy_`` side copies
    12.5 B per token (read + write = the same 25 B).
(b) step level: the mlm256 benchmark step (``StepEngine``, captured graph, the batch ``bench.py``
    builds) with the model's ``TextMasking`` as it is and replaced by one with ``whole_word=True``
    (shipped continuation table, ``word_clump`` 2.0, so the wider selection capacity is part of the
    measurement): wall time per step over windows of at least ``--window`` seconds, alternating,
    same process.  It also prints ``word_clump()`` of the benchmark batch.

    python tools/mask_bench.py [--rounds 5] [--window 0.5] [--inner 20] [--out profiles/whole_word_masking.md]
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

SHAPES = ((64, 512), (8, 8192))
V, UNK, MASK, LO, P = 10003, 1, 2, 3, 0.15
BYTES_PER_TOKEN = 25


def _table():
    from perceiver_io_amd.data.imdb import shipped_tokenizer
    from perceiver_io_amd.utils.tokenizer import continuation_table

    return continuation_table(shipped_tokenizer(V))


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
    from perceiver_io_amd.ops import emulation, ext
    from perceiver_io_amd.utils.tokenizer import pack_bits, word_clump

    K = ext.require()
    table = _table()
    packed = pack_bits(table).cuda()
    rows = []
    for shape in SHAPES:
        g = torch.Generator().manual_seed(0)
        x = torch.randint(0, V, shape, generator=g).cuda()
        pad = (torch.rand(shape, generator=g) < 0.2).cuda()
        n = x.numel()
        state = torch.tensor([0x123456789AB, 0, 0], device="cuda")
        # the timed kernel computes what its emulation computes, at this size
        st_e = state.clone()
        got = K.text_mask_words(x, pad, state, packed, UNK, MASK, P, LO, V, True)
        want = emulation.text_mask_words(x, pad, st_e, packed, UNK, MASK, P, LO, V, True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(state, st_e)
        src = torch.empty(n * BYTES_PER_TOKEN // 2, dtype=torch.uint8, device="cuda").random_()
        dst = torch.empty_like(src)
        graphs = {"text_mask": _graph_of(lambda: K.text_mask(x, pad, state, UNK, MASK, P, LO, V, True), a.inner),
                  "text_mask_words": _graph_of(
                      lambda: K.text_mask_words(x, pad, state, packed, UNK, MASK, P, LO, V, True), a.inner),
                  "copy_": _graph_of(lambda: dst.copy_(src), a.inner)}
        for gr in graphs.values():  # warm-up
            _window(gr, a.inner, 0.05)
        r = _ab(graphs, lambda gr: _window(gr, a.inner, a.window), a.rounds)
        assert int(state[2]) == 0 and torch.equal(dst, src)
        row = dict(shape=shape, tokens=n, us=r, clump=word_clump(x, pad, table.cuda(), UNK),
                   gbps={k: BYTES_PER_TOKEN * n / (r[k][0] * 1e-6) / 1e9 for k in r})
        rows.append(row)
        print(f"{shape}: " + "  ".join(f"{k} {r[k][0]:6.2f} us [{r[k][1]:.2f}, {r[k][2]:.2f}] {row['gbps'][k]:6.0f} GB/s"
                                      for k in r) + f"  word_clump {row['clump']:.3f}", flush=True)
        del graphs
    return rows


STEP_SIDES = ("off", "whole-word")


def bench_step(a):
    from perceiver_io_amd import ops
    from perceiver_io_amd.models import TextMasking
    from perceiver_io_amd.ops.optim import FusedAdamW
    from perceiver_io_amd.train.engine import StepEngine
    from perceiver_io_amd.utils.tokenizer import word_clump

    ops.set_backend("auto")
    dev = torch.device("cuda", torch.cuda.current_device())
    args = bench.parse(["--config", "mlm256"])
    table = _table()
    sides, clump = {}, None
    for name in STEP_SIDES:
        torch.manual_seed(1234)
        lit, loss_fn, make_batch, _, lr, _ = bench.build(args, dev)
        if name == "whole-word":
            lit.model.masking = TextMasking(args.vocab, whole_word=True, continuation=table, word_clump=2.0)
        lit.to(dev)
        opt = FusedAdamW([p for p in lit.model.parameters() if p.requires_grad], lr=lr, weight_decay=0.01)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=lr, total_steps=50000, pct_start=0.1,
                                                    cycle_momentum=False)
        eng = StepEngine(loss_fn, opt, sched, device=dev, graph=True)
        g = torch.Generator(device="cpu").manual_seed(99)
        data = [tuple(t.to(dev) for t in make_batch(g)) for _ in range(4)]
        clump = word_clump(data[0][1], data[0][2], table.to(dev), UNK)
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
    ops.mlm_head.check_overflow(reset=True)  # raises if a selected position fell out of the capacity
    print("mlm256 step: " + "  ".join(f"{n} {r[n][0]:8.1f} us [{r[n][1]:.1f}, {r[n][2]:.1f}]" for n in STEP_SIDES)
          + f"  word_clump of the batch {clump:.3f}", flush=True)
    return r, clump


def report(a, rows, step):
    out = ["# Whole-word masking (`text_mask_words_kernel`) against token-level masking", "",
           f"Written by `tools/mask_bench.py` on {torch.cuda.get_device_name(0)}: hipGraph replays of {a.inner} "
           f"launches, windows ≥ {a.window} s between device events, {a.rounds} alternating rounds, median [min, max].  "
           "All numbers of this file come from one process on one device.", "",
           "## Kernel level", "",
           f"Ids uniform over the shipped {V}-entry vocabulary (2,051 continuation pieces), 20 % padding.  Byte "
           f"model: {BYTES_PER_TOKEN} B per token (ids and pad read, masked ids and labels written); `copy_` moves "
           "the same bytes (12.5 B per token read and written).  Back-to-back replays keep these buffers in the cache "
           "hierarchy: the GB/s columns are the byte model over the time, not HBM traffic.", "",
           "| shape | tokens | `text_mask` µs | `text_mask_words` µs | `copy_` µs | words / token-level | "
           "`text_mask` GB/s | `text_mask_words` GB/s | `copy_` GB/s | `word_clump()` |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        u = r["us"]
        cell = lambda k: f"{u[k][0]:.2f} [{u[k][1]:.2f}, {u[k][2]:.2f}]"  # noqa: E731
        out.append(f"| {r['shape'][0]} × {r['shape'][1]} | {r['tokens']} | {cell('text_mask')} | "
                   f"{cell('text_mask_words')} | {cell('copy_')} | {u['text_mask_words'][0] / u['text_mask'][0]:.2f} | "
                   f"{r['gbps']['text_mask']:.0f} | {r['gbps']['text_mask_words']:.0f} | {r['gbps']['copy_']:.0f} | "
                   f"{r['clump']:.3f} |")
    out += ["", "`word_clump()` is Σ len² / Σ len over the words of the batch.  Uniform random ids are the only text "
            "available here; `LitMaskedLanguageModel`'s default `word_clump = 2.0` is a setting for real corpora, not "
            "a measurement.", ""]
    if step is None:
        out += ["## Step level", "", "Not measured in this run (`--no-step`).", ""]
    else:
        r, clump = step
        off, on = r["off"], r["whole-word"]
        out += ["## Step level (mlm256, batch 64 × 512, captured step, one GPU)", "",
                "\"off\" is the step as it is without the flag: `TextMasking` launches `text_mask_kernel` and the "
                "capacities are those of `clump = 1`.  \"whole-word\" replaces the module by one with the shipped "
                "continuation table and `word_clump = 2.0`, so it pays for the other kernel and for the wider "
                f"selection capacity.  `word_clump()` of the benchmark batch: {clump:.3f}.", "",
                "| masking | µs per step | against off |", "|---|---|---|",
                f"| off | {off[0]:.1f} [{off[1]:.1f}, {off[2]:.1f}] | |",
                f"| whole-word | {on[0]:.1f} [{on[1]:.1f}, {on[2]:.1f}] | {on[0] - off[0]:+.1f} µs "
                f"({(on[0] / off[0] - 1) * 100:+.2f} %) |", ""]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whole_word_masking.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mask_bench needs a GPU: timings from anything else say nothing")
    from perceiver_io_amd.ops import ext

    ext.require()
    rows = bench_kernels(a)
    step = None if a.no_step else bench_step(a)
    report(a, rows, step)


if __name__ == "__main__":
    main()
