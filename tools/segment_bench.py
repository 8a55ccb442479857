#!/usr/bin/env python
"""LArTPC inference benchmark: ``LArPerceiver.segment`` (sparse, fused head, no dense logits)
against the dense path ``model(img).argmax(1)`` on the fused backend, on the same synthetic
events in one process, plus ``nonzero_compact`` (every launch configuration) and
``pixel_predict`` alone.  Writes the results as JSON (``--out``) and as the report
``profiles/lartpc_segment.md`` (``--md``).

Times are device events around back-to-back calls after ``--warmup`` calls of the same shape.
Every timed window lasts at least ``--window-ms`` (the call count is sized from a short pilot);
the end-to-end paths alternate over ``--rounds`` rounds (median, min - max), the kernels take the
median of three windows.  Kernel figures are per *call* of the binding: launches plus output
allocation, issued back to back.  Measuring needs a GPU (no CPU fallback);
``--render results.json --md report.md`` only rewrites the report from saved results.

    python tools/segment_bench.py --out profiles/lartpc_segment.json --md profiles/lartpc_segment.md
"""
from __future__ import annotations

import argparse
import json
import math
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DENSE = "dense model(img).argmax(1)"
SEG_SYNC = "segment(img)"
SEG_CAP = "segment(img, capacity=C)"


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


def median3(fn, a):
    runs = [timed(fn, a.warmup, a.window_ms) for _ in range(3)]
    return {"us": statistics.median(r[0] for r in runs) * 1e3, "calls": runs[0][1]}


def measure(a):
    from perceiver_io_amd import ops
    from perceiver_io_amd.data.synthetic import SyntheticLArTPC
    from perceiver_io_amd.models.lartpc import LArPerceiver
    from perceiver_io_amd.ops import ext

    if not torch.cuda.is_available():
        raise SystemExit("segment_bench needs a GPU")
    K = ext.require()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = LArPerceiver(a.size).to(dev).eval()
    data = SyntheticLArTPC(a.batch, a.size, seed=1)  # run.py's validation events
    img = torch.stack([data[i][0] for i in range(a.batch)]).to(dev)
    flat = img.reshape(a.batch, -1).contiguous()
    npix = flat.shape[1]
    res = {"size": a.size, "batch": a.batch, "npix": npix, "warmup": a.warmup, "window_ms": a.window_ms,
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    with torch.no_grad(), ops.backend("hip"):
        seg = model.segment(img)
        cap = seg.classes.shape[1]
        res["count"] = seg.count.tolist()
        res["capacity"] = cap
        dense_cls = model(img).argmax(1)
        lit = flat != 0
        res["lit_pixels_agreeing_with_dense_argmax"] = float((seg.class_map[lit].long() == dense_cls[lit]).float().mean())

        paths = {DENSE: lambda: model(img).argmax(1), SEG_SYNC: lambda: model.segment(img),
                 SEG_CAP: lambda: model.segment(img, capacity=cap)}
        rounds = {k: [] for k in paths}
        calls = {}
        for _ in range(a.rounds):  # alternate the paths: drift hits all of them alike
            for name, fn in paths.items():
                ms, calls[name] = timed(fn, a.warmup, a.window_ms)
                rounds[name].append(ms)
        res["end_to_end_ms"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "calls": calls[k]}
                                for k, v in rounds.items()}

        # nonzero_compact alone: S segments per sample x V loads per thread and tile
        res["nonzero_compact"] = {f"S={S},V={V}": median3(lambda: K.nonzero_compact(flat, cap, S, V), a)
                                  for V in (4, 8) for S in (1, 2, 4, 8, 16, 32, 64, 128, 256)}
        res["nonzero_compact_default"] = median3(lambda: K.nonzero_compact(flat, cap), a)
        res["nonzero_count_only"] = median3(lambda: K.nonzero_compact(flat, 0), a)

        # pixel_predict alone on the decoder output of these events
        values, index, kmask, _ = K.nonzero_compact(flat, cap)
        h = model.sparse_hidden(values, index, kmask, index)
        lin = model.decoder.output_adapter.linear
        h2 = h.reshape(-1, h.shape[-1]).float().contiguous()
        w, b = lin.weight.detach().contiguous(), lin.bias.detach().contiguous()
        qi, qv = index.reshape(-1).contiguous(), (~kmask).reshape(-1).contiguous()
        lab = torch.randint(0, 3, (h2.shape[0],), device=dev)
        res["pixel_predict_rows"] = h2.shape[0]
        res["pixel_predict_channels"] = h2.shape[1]
        res["pixel_predict"] = median3(lambda: K.pixel_predict(h2, w, b, qi, qv, cap, npix), a)
        res["pixel_predict_with_labels"] = median3(lambda: K.pixel_predict(h2, w, b, qi, qv, cap, npix, lab), a)

        def aten_head():  # the ATen equivalent of the head: logits, argmax, softmax max, scatter
            z = torch.addmm(b, h2, w.t())
            c = z.argmax(-1)
            p = torch.softmax(z, -1).max(-1).values
            m = torch.zeros(a.batch, npix, dtype=torch.uint8, device=dev)
            m.view(-1)[(torch.arange(h2.shape[0], device=dev) // cap * npix + qi)[qv]] = c[qv].to(torch.uint8)
            return c, p, m

        res["aten_head"] = median3(aten_head, a)
        ops.check_device_errors()
        save()

        # the two sync-free paths replayed as captured graphs: device time without the host's
        # launch cost.  Last, and a capture that fails ends the run: nothing else is started on
        # the device after it (the results so far are already saved).
        replay = {}
        for name in (DENSE, SEG_CAP):
            fn = paths[name]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    fn()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                keep = fn()  # noqa: F841  (the graph's outputs stay alive)
            runs = [timed(graph.replay, a.warmup, a.window_ms) for _ in range(3)]
            replay[name] = {"ms": statistics.median(r[0] for r in runs), "calls": runs[0][1]}
            del graph, keep
        res["graph_replay_ms"] = replay
    ops.check_device_errors()
    save()
    return res


# ---- report ------------------------------------------------------------------------------------
def kernel_resources():
    """{kernel: {VGPRs, SGPRs, LDS, scratch, occupancy}} of the two kernels from hipcc's
    ``-Rpass-analysis=kernel-resource-usage`` (None when hipcc is not there)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    if not hipcc:
        return None
    src = os.path.join(ROOT, "perceiver_io_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast",
                            "-munsafe-fp-atomics", "-I", src, "-c", os.path.join(src, "pixel_head.hip"), "-o",
                            os.path.join(tmp, "pixel_head.o"), "-Rpass-analysis=kernel-resource-usage"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        return None
    out, cur = {}, None
    keys = {"VGPRs": "VGPRs", "TotalSGPRs": "SGPRs", "ScratchSize [bytes/lane]": "scratch",
            "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "LDS"}
    for line in r.stdout.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            dem = subprocess.run(["c++filt", v], stdout=subprocess.PIPE, text=True).stdout.strip() if shutil.which("c++filt") else v
            name = re.sub(r"^(void )?pio::|\(.*$", "", dem)
            cur = name if ("pixel_predict" in name or "nonzero" in name) else None
            if cur:
                out[cur] = {}
        elif cur and k in keys:
            out[cur][keys[k]] = v
    return out


def render(res, path):
    e2e, rep = res["end_to_end_ms"], res.get("graph_replay_ms", {})
    cap, B, size = res["capacity"], res["batch"], res["size"]

    def ms(d):
        return f"{d['median']:.3f} ({d['min']:.3f} – {d['max']:.3f}; {d['calls']} calls / window)"

    def rp(name):
        return f"{rep[name]['ms']:.3f}" if name in rep else "not measured"

    nz = res["nonzero_compact"]
    S_list = (1, 2, 4, 8, 16, 32, 64, 128, 256)
    L = [f"# LArTPC inference: `segment` against the dense path ({res['device']})", "",
         f"Written by `python tools/segment_bench.py --md {os.path.relpath(path, ROOT)}`: {size}×{size} events, batch {B}, the",
         f"`SyntheticLArTPC(seed=1)` events `run.py` validates on ({' / '.join(f'{c:,}' for c in res['count'])} non-zero pixels,",
         f"capacity {cap:,} = the maximum rounded up to the 2,048 bucket), random-init `LArPerceiver({size})`, fused (`hip`)",
         f"backend, one process.  Device events around back-to-back calls after {res['warmup']} warm-up calls of the same",
         f"shape; every window lasts at least {res['window_ms']:.0f} ms.  End-to-end paths alternate over {res['rounds']} rounds (median,",
         "min – max); kernels: median of 3 windows.  `segment`'s class equals the dense `argmax` at",
         f"{100 * res['lit_pixels_agreeing_with_dense_argmax']:.1f} % of the lit pixels of these events.", "",
         "## End to end", "",
         "| path | eager calls, ms / batch | replayed as a captured graph, ms / batch |", "|---|---|---|",
         f"| `model(img).argmax(1)` (dense: {res['npix']:,} keys and queries per sample, `({B}, 3, {res['npix']})` fp32 logits, ATen argmax) | {ms(e2e[DENSE])} | {rp(DENSE)} |",
         f"| `segment(img)` (count pass, one host read of `count.max()`, compaction, sparse model, `pixel_predict`) | {ms(e2e[SEG_SYNC])} | – (host sync) |",
         f"| `segment(img, capacity={cap})` (no host sync) | {ms(e2e[SEG_CAP])} | {rp(SEG_CAP)} |", ""]
    if DENSE in rep and SEG_CAP in rep:
        d_e, s_e, s_s = e2e[DENSE]["median"], e2e[SEG_CAP]["median"], e2e[SEG_SYNC]["median"]
        d_g, s_g = rep[DENSE]["ms"], rep[SEG_CAP]["ms"]
        L += ["What this says:", "",
              f"* The dense path is bound by the device: {d_e:.2f} ms with the host launching each kernel, {d_g:.2f} ms replayed",
              "  as a graph.  On the fused backend the dense encoder never forms K/V (`attn_fwd_pe`, factored",
              "  PE projection), and the rest is a handful of large fused launches.",
              f"* The sparse path needs {s_g:.3f} ms of device time, **{d_g / s_g:.1f}× less than the dense path**.  Called eagerly",
              f"  it takes {s_e:.2f} ms: it is bound by the host, which issues its many small launches (three",
              "  cross-attention layers, three latent blocks, the decoder, compaction, head) one by one.  Called",
              f"  eagerly the gain over the dense path is therefore {d_e / s_e:.2f}× ({d_e / s_s:.2f}× with the count pass and its host",
              "  read).  The remedy is the one the training step uses: capture the fixed-capacity call",
              "  (`capacity=` makes the shapes static and removes the only host sync) in a hipGraph.  `segment`",
              "  does not do that itself; the replay column shows what it gives.",
              f"* The dense path writes {B * 3 * res['npix'] * 4 / 1e6:.1f} MB of fp32 logits per batch (on top of the decoder output for",
              f"  {B * res['npix']:,} rows); `segment` writes a {B * res['npix'] / 1e6:.1f} MB class map and decodes {B * cap:,} rows.", ""]
    best = min(nz.values(), key=lambda d: d["us"])["us"]
    L += ["## `nonzero_compact` launch configuration", "",
          f"`({B}, {res['npix']})` fp32 in, capacity {cap:,}.  µs per call of the binding (launches + five output allocations,",
          f"back to back; {nz['S=1,V=4']['calls']:,} – {nz['S=64,V=4']['calls']:,} calls per window).  S = segments per sample (S × {B} workgroups of 256",
          "threads), V = loads per thread and tile (tile = 256·V pixels).  S = 1 is a single launch (one",
          "workgroup per sample); S > 1 is a count launch followed by the scatter launch.", "",
          "| S | " + " | ".join(str(s) for s in S_list) + " |", "|---|" + "---|" * len(S_list)]
    for V in (4, 8):
        L.append(f"| V = {V} | " + " | ".join(f"{nz[f'S={s},V={V}']['us']:.1f}" for s in S_list) + " |")
    L += ["",
          f"One workgroup per sample walks {res['npix'] // 1024} tiles serially with a barrier each: {nz['S=1,V=4']['us']:.0f} µs for a {res['npix'] * 4 / 1e6:.0f} MB read.",
          f"Splitting wins by {nz['S=1,V=4']['us'] / nz['S=64,V=4']['us']:.0f}× although it costs a second launch and reads the image twice (the second",
          f"read hits L2); from S = 64 on the call sits at its floor (best {best:.1f} µs: two launches plus the",
          "allocations) and the tile size no longer matters.  Chosen: **S = 64 segments (fewer when the image",
          f"has fewer tiles), V = 4 (1,024-pixel tiles), 256 threads**: {64 * B} workgroups at this shape.  The",
          f"default call measures {res['nonzero_compact_default']['us']:.1f} µs; the count-only call (`cap = 0`, count launch + a scatter launch that",
          f"reads only the segment counts) {res['nonzero_count_only']['us']:.1f} µs.", "",
          "## `pixel_predict` alone", "",
          f"{res['pixel_predict_rows']:,} rows ({B} × {cap:,}) × {res['pixel_predict_channels']} channels, K = 3, grid 512 × 256 threads:", "",
          "| | µs per call |", "|---|---|",
          f"| `pixel_predict` (classes, confidence, class map incl. its {B * res['npix'] / 1e6:.0f} MB clear) | {res['pixel_predict']['us']:.1f} |",
          f"| `pixel_predict` with labels (+ confusion partials) | {res['pixel_predict_with_labels']['us']:.1f} |",
          f"| ATen: `addmm`, `argmax`, `softmax().max()`, `zeros` + masked index scatter | {res['aten_head']['us']:.1f} |", ""]
    kr = kernel_resources()
    L += ["## Kernel resources (hipcc `-Rpass-analysis=kernel-resource-usage`, gfx950)", ""]
    if kr:
        L += ["| kernel | VGPRs | SGPRs | LDS bytes / block | scratch bytes / lane | occupancy (waves / SIMD) |", "|---|---|---|---|---|---|"]
        for name, d in kr.items():
            L.append(f"| `{name}` | {d.get('VGPRs')} | {d.get('SGPRs')} | {d.get('LDS')} | {d.get('scratch')} | {d.get('occupancy')} |")
    else:
        L.append("not measured (no hipcc where this report was written)")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=500.0, help="least duration of every timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    ap.add_argument("--md", default=None, help="write the report here (profiles/lartpc_segment.md)")
    ap.add_argument("--render", default=None, metavar="JSON", help="no measurement: write --md from saved results")
    a = ap.parse_args(argv)
    if a.render:
        with open(a.render) as f:
            res = json.load(f)
    else:
        res = measure(a)
        print(json.dumps(res, indent=1))
    if a.md:
        render(res, a.md)


if __name__ == "__main__":
    main()
