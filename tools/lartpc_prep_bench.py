#!/usr/bin/env python
"""LArTPC input-side benchmark: the host collator against ``event_compact`` (csrc/lartpc_prep.hip).

Four measurements on ``--batch`` events of ``--size`` × ``--size`` in one process, written as JSON
(``--out``) and as the report ``profiles/lartpc_prep.md`` (``--md``):

1. ``sparse_collate`` on the host, one thread (what one DataLoader worker does per batch);
2. ``event_compact`` per dihedral code against ``nonzero_compact`` on the same events and against a
   device ``copy_`` of the two input planes (device events, windows of at least ``--window-ms``,
   median of three; figures are per call of the binding: launches plus output allocation);
3. ``run.py`` fit throughput on events generated once and kept in memory: the host collator at 1
   and 4 workers against ``--device-collate --augment dihedral``;
4. the captured training step at fixed capacities (dataset maxima) against the bucketed shapes
   (batch maxima) of the same batches, and with ``event_compact`` inside the step.

Measuring needs a GPU (no CPU fallback); ``--render results.json --md report.md`` only rewrites the
report from saved results.

    python tools/lartpc_prep_bench.py --out profiles/lartpc_prep.json --md profiles/lartpc_prep.md
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import math
import os
import re
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

README_STEP_MS = 0.837  # README: the sparse fused graph step of the lartpc bench config, 4 events


def timed(fn, warmup: int, window_ms: float):
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
    return window(max(20, math.ceil(1.1 * window_ms / max(pilot, 1e-4))))


def median3(fn, a):
    return statistics.median(timed(fn, a.warmup, a.window_ms) for _ in range(3)) * 1e3


class MemoryEvents(torch.utils.data.Dataset):
    """Events generated once (the synthetic generator costs far more than any collator)."""

    cache: dict = {}

    def __init__(self, n, size=512, seed=0):
        from perceiver_io_amd.data.synthetic import SyntheticLArTPC

        key = (n, size, seed)
        if key not in self.cache:
            src = SyntheticLArTPC(n, size, seed)
            self.cache[key] = [src[i] for i in range(n)]
        self.events = self.cache[key]

    def __len__(self):
        return len(self.events)

    def __getitem__(self, i):
        return self.events[i]


def host_collate(a, res):
    from perceiver_io_amd.data.lartpc import sparse_collate

    events = [MemoryEvents(a.events, a.size, 0)[i] for i in range(a.batch)]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # a DataLoader worker runs torch on one thread
    try:
        runs = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(10):
                sparse_collate(events)
            runs.append((time.perf_counter() - t0) / 10 * 1e3)
    finally:
        torch.set_num_threads(threads)
    res["sparse_collate_ms"] = {"median": statistics.median(runs), "min": min(runs), "max": max(runs)}


def kernels(a, res):
    from perceiver_io_amd.data.lartpc import DenseCollator
    from perceiver_io_amd.ops import ext

    K = ext.require()
    data = MemoryEvents(a.events, a.size, 0)
    img, lab = (t.cuda() for t in DenseCollator()([data[i] for i in range(a.batch)]))
    flat = img.reshape(a.batch, -1)
    counts = K.event_compact(img, lab, torch.zeros(a.batch, dtype=torch.int32, device="cuda"), 0, 0, 6, 3)[5]
    kcap, qcap = (-(-int(c) // a.bucket) * a.bucket for c in counts.max(0).values.tolist())
    res["counts"], res["capacities"] = counts.tolist(), [kcap, qcap]
    per = {}
    for code in range(8):
        words = torch.full((a.batch,), code, dtype=torch.int32, device="cuda")
        per[str(code)] = median3(lambda: K.event_compact(img, lab, words, kcap, qcap, 6, 3), a)
    res["event_compact_us"] = per
    words = torch.zeros(a.batch, dtype=torch.int32, device="cuda")
    res["event_compact_count_only_us"] = median3(lambda: K.event_compact(img, lab, words, 0, 0, 6, 3), a)
    res["nonzero_compact_us"] = median3(lambda: K.nonzero_compact(flat, kcap), a)
    nbytes = img.numel() * 4 + lab.numel()
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    res["copy_bytes"] = nbytes
    res["copy_us"] = median3(lambda: dst.copy_(src), a)


def fits(a, res):
    import run

    run.SyntheticLArTPC = MemoryEvents  # same events for every variant, no generator in the loop
    MemoryEvents(a.events, a.size, 0), MemoryEvents(a.val_events, a.size, 1)
    base = ["--events", str(a.events), "--val-events", str(a.val_events), "--size", str(a.size), "--batch-size",
            str(a.batch), "--epochs", str(a.epochs), "--log-every", "1000000", "--bucket", str(a.bucket)]
    variants = {"host collate, 1 worker": ["--workers", "1"], "host collate, 4 workers": ["--workers", "4"],
                "device collate + dihedral, 1 worker": ["--workers", "1", "--device-collate", "--augment", "dihedral"]}
    out = {k: [] for k in variants}
    graphs = {}
    for _ in range(a.rounds):  # alternate the variants: drift hits all of them alike
        for name, extra in variants.items():
            with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()) as buf:
                run.main(base + extra + ["--log-dir", os.path.join(tmp, "runs"), "--ckpt-dir", os.path.join(tmp, "ckpt")])
            text = buf.getvalue()
            out[name].append(float(re.search(r"throughput: ([0-9.]+) samples/s", text).group(1)))
            m = re.search(r"captured training graphs: (\d+)", text)
            if m:
                graphs[name] = int(m.group(1))
            if "overflow" in text:
                raise SystemExit(f"{name}: the fit reported a capacity overflow")
    res["fit_samples_per_s"] = out
    res["fit_training_graphs"] = graphs
    res["fit_steps"] = a.epochs * (a.events // a.batch)


def steps(a, res):
    from perceiver_io_amd.data.lartpc import DenseCollator, sparse_collate
    from perceiver_io_amd.models.lartpc import LArPerceiver, class_weights
    from perceiver_io_amd.ops.optim import FusedAdam
    from perceiver_io_amd.train.engine import StepEngine

    data = MemoryEvents(a.events, a.size, 0)
    groups = [[data[i] for i in range(s, s + a.batch)] for s in range(0, a.events, a.batch)]
    bucketed = [tuple(t.cuda() for t in sparse_collate(g, a.bucket)) for g in groups]
    kmax = max(b[0].shape[1] for b in bucketed)
    qmax = max(b[3].shape[1] for b in bucketed)

    def at_capacity(g):
        out = sparse_collate(g, max(kmax, qmax))  # one bucket of the dataset maximum
        return tuple(t.contiguous().cuda() for t in (out[0][:, :kmax], out[1][:, :kmax], out[2][:, :kmax], out[3][:, :qmax], out[4][:, :qmax]))

    fixed = [at_capacity(g) for g in groups]
    dense = [tuple(t.cuda() for t in DenseCollator()(g)) + (torch.full((a.batch,), i % 8, dtype=torch.int32, device="cuda"),)
             for i, g in enumerate(groups)]
    w = class_weights("cuda")
    res["step_shapes"] = {"bucketed": sorted({(b[0].shape[1], b[3].shape[1]) for b in bucketed}), "fixed": [kmax, qmax]}
    out = {}
    for name, batches in (("bucketed shapes (batch maxima)", bucketed), ("fixed capacities (dataset maxima)", fixed),
                          ("fixed capacities, event_compact in the step", dense)):
        torch.manual_seed(0)
        model = LArPerceiver(a.size).cuda()
        opt = FusedAdam(model.trained_parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=10.0)
        if len(batches[0]) == 3:
            fn = lambda b: model.event_loss(b, w, kmax, qmax)[0]  # noqa: E731
        else:
            fn = lambda b: model.sparse_loss(b, w)[0]  # noqa: E731
        eng = StepEngine(fn, opt, device="cuda", graph=True, warmup_eager=0)
        pos = [0]

        def one():
            eng.step(batches[pos[0] % len(batches)], ring_view=True)
            pos[0] += 1

        for _ in range(len(batches)):  # every shape captured before the clock starts
            one()
        out[name] = {"us": median3(one, a), "graphs": eng.num_graphs}
    res["step"] = out


def measure(a):
    if not torch.cuda.is_available():
        raise SystemExit("lartpc_prep_bench needs a GPU")
    res = {"size": a.size, "batch": a.batch, "events": a.events, "bucket": a.bucket, "warmup": a.warmup,
           "window_ms": a.window_ms, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "argv": " ".join(sys.argv[1:])}
    for part in (host_collate, kernels, steps, fits):
        part(a, res)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
    return res


def render(res) -> str:
    B, size = res["batch"], res["size"]
    hc = res["sparse_collate_ms"]
    ec = res["event_compact_us"]
    row = [ec[str(c)] for c in range(4)]
    tr = [ec[str(c)] for c in range(4, 8)]
    nz, cp = res["nonzero_compact_us"], res["copy_us"]
    L = ["# LArTPC batch building on the device (`event_compact`)", "",
         f"`python tools/lartpc_prep_bench.py {res['argv']}` on {res['device']}: {B} events of {size} × {size}, "
         f"capacities rounded to {res['bucket']}.  Kernel figures are device events around back-to-back calls of the "
         f"binding (launches plus output allocation), windows of at least {res['window_ms']:.0f} ms after "
         f"{res['warmup']} warm-up calls, median of three.", "",
         "## 1. The host collator", "",
         f"`sparse_collate` on {B} events, one thread (one DataLoader worker): median {hc['median']:.2f} ms "
         f"(min {hc['min']:.2f}, max {hc['max']:.2f}, five runs of ten calls, host clock).  The README's sparse fused graph step "
         f"is {README_STEP_MS} ms for {B} events: one worker collates {hc['median'] / README_STEP_MS:.1f}× slower than the "
         f"device steps, and {math.ceil(hc['median'] / README_STEP_MS)} workers would be needed to keep up, before the "
         "five padded tensors are shipped.  The fits of section 3 show what that means end to end.", "",
         "## 2. `event_compact` per code", "",
         f"Key / query counts per event: {res['counts']}; capacities {res['capacities']}.", "",
         "| call | µs | × `nonzero_compact` | × `copy_` |", "|---|---|---|---|"]
    for c in range(8):
        kind = "row-major" if c < 4 else "transposed: column reads"
        L.append(f"| `event_compact`, code {c} ({kind}) | {ec[str(c)]:.1f} | {ec[str(c)] / nz:.2f} | {ec[str(c)] / cp:.2f} |")
    L += [f"| `event_compact`, counting call (capacities 0) | {res['event_compact_count_only_us']:.1f} | "
          f"{res['event_compact_count_only_us'] / nz:.2f} | {res['event_compact_count_only_us'] / cp:.2f} |",
          f"| `nonzero_compact` (keys only, no labels, no transform) | {nz:.1f} | 1.00 | {nz / cp:.2f} |",
          f"| `copy_` of {res['copy_bytes']:,} bytes (both input planes, device to device) | {cp:.1f} | {cp / nz:.2f} | 1.00 |", "",
          f"Row-major codes 0–3: {min(row):.1f}–{max(row):.1f} µs; transposed codes 4–7: {min(tr):.1f}–{max(tr):.1f} µs "
          f"({statistics.mean(tr) / ec['0']:.2f}× code 0).  A transposed code walks the output rows and so reads the source down "
          "its columns: every lane of a load touches another cache line (64 lines per wave and load instead of 2 for the "
          "image, 1 for the labels).  The kernel does not stage those reads through LDS; it relies on the planes "
          f"({size * size * 4 // 1024} KB + {size * size // 1024} KB per event) staying in L2, where neighbouring segments "
          "reuse the lines.  The figures above are the measured price of that choice.", "",
          "## 3. `run.py` fit throughput", "",
          f"`run.main` on {res['events']} training events generated once and kept in memory (the synthetic generator is not "
          f"in the loop), {res['fit_steps']} steps per fit, throughput as `run.py` prints it (from step 2 on, validation "
          f"included), the variants alternating over {res['rounds']} rounds in one process:", "",
          "| variant | samples/s (median) | min – max | training graphs |", "|---|---|---|---|"]
    for name, v in res["fit_samples_per_s"].items():
        g = res["fit_training_graphs"].get(name, "per bucket")
        L.append(f"| {name} | {statistics.median(v):.0f} | {min(v):.0f} – {max(v):.0f} | {g} |")
    med = {k: statistics.median(v) for k, v in res["fit_samples_per_s"].items()}
    h1, h4, dv = (med[k] for k in res["fit_samples_per_s"])
    st = res["step"]
    names = list(st)
    ceiling = B / (st[names[2]]["us"] * 1e-6)
    L += ["", f"The device path with one worker runs at {dv / h1:.2f}× the host collator with one worker and at {dv / h4:.2f}× the "
          f"host collator with four.  Its own step (section 4) would allow {ceiling:.0f} samples/s, so every variant is bound by "
          f"the host side of the fit, and the collator is only part of that: the device path still stacks and ships "
          f"{res['copy_bytes'] / 2**20:.1f} MB of dense planes per batch from pageable memory, against well under 1 MB of sparse "
          "tensors.  With four workers the host collator is not the bottleneck; what the device path adds there is the "
          "augmentation and the single captured graph, not throughput."]
    L += ["", "## 4. The step at fixed capacities", "",
          f"The captured training step (`StepEngine`, FusedAdam) cycling over the {res['events'] // B} batches of the same "
          f"events, already on the device.  Bucketed shapes met: {res['step_shapes']['bucketed']}; fixed capacities: "
          f"{res['step_shapes']['fixed']}.", "",
          "| step | µs | graphs |", "|---|---|---|"]
    for n in names:
        L.append(f"| {n} | {st[n]['us']:.1f} | {st[n]['graphs']} |")
    L += ["", f"Padding every batch to the dataset maximum costs {st[names[1]]['us'] - st[names[0]]['us']:+.1f} µs per step "
          f"against the batch maxima; building the batch inside the step adds {st[names[2]]['us'] - st[names[1]]['us']:+.1f} µs.", ""]
    return "\n".join(L)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--val-events", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--bucket", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--render", default=None, help="rewrite --md from saved results, measure nothing")
    a = ap.parse_args(argv)
    if a.render:
        with open(a.render) as f:
            res = json.load(f)
    else:
        res = measure(a)
    if a.md:
        with open(a.md, "w") as f:
            f.write(render(res))
    print(json.dumps({k: res[k] for k in res if k not in ("counts",)}))


if __name__ == "__main__":
    main()
