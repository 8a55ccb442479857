"""Head-averaged attention weights (``csrc/attn_weights.hip``) against the ATen composition and the
bytes-moved floor.  Writes ``profiles/attention_maps.md``.

Kernel level, at the encoder cross-attention shapes of ``mlm256`` (64 × 4 heads × 256 latents ×
    512 tokens, head width 16), ``imagenet`` (32 × 4 × 32 × 50,176, head width 32) and ``lartpc``
    (4 × 4 × 32 × 8,192 key slots, head width 16, K a view of packed K|V rows, 40 % of the slots
    padded): ``attn_weights`` with the mass alone and with avg + mass, on bf16 operands and the
    ``attn_fwd`` LSE, and ``attn_fwd`` + mass (what ``ops.attention_mass`` launches), against

      * ATen: per-head scores (``matmul``), ``masked_fill``, fp32 ``softmax`` materialised as
        ``(B, H, Nq, Nk)``, ``mean`` over the heads, ``sum`` over the queries;
      * the floor: the bytes the kernel must move (Q, K, LSE and mask read once, the outputs written
        once) at 6.3 TB/s, the achievable HBM rate of one MI355X.

    Each side runs ``--inner`` times between two device events, in ``--rounds`` alternating rounds;
    the median round is reported with the min–max spread.

    python tools/attn_maps_bench.py [--rounds 5] [--inner 20] [--out profiles/attention_maps.md]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12  # achievable bytes/s
# name, B, H, Nq, Nk, D, packed K|V view, padded share of the key slots
SHAPES = [("mlm256", 64, 4, 256, 512, 16, True, 0.0),
          ("imagenet", 32, 4, 32, 224 * 224, 32, True, 0.0),
          ("lartpc", 4, 4, 32, 8192, 16, True, 0.4)]


def _time(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner  # µs


def _ab(sides, inner, rounds):
    for fn in sides.values():  # warm-up
        _time(fn, 3)
    t = {n: [] for n in sides}
    for _ in range(rounds):
        for n, fn in sides.items():
            t[n].append(_time(fn, inner))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in t.items()}


def bench_kernels(a):
    from perceiver_io_amd.ops import ext
    from perceiver_io_amd.ops.attention import pick_splits

    K = ext.require()
    rows = []
    for name, B, H, Nq, Nk, D, packed, padded in SHAPES:
        torch.manual_seed(0)
        C = H * D
        scale = D ** -0.5
        q = torch.randn(1, Nq, C, device="cuda").to(torch.bfloat16)  # the latent array: one stream for the batch
        kv = torch.randn(B, Nk, 2 * C if packed else C, device="cuda").to(torch.bfloat16)
        k = kv[:, :, :C]
        km = None
        if padded:
            km = torch.arange(Nk, device="cuda")[None, :] >= torch.tensor(
                [int(Nk * (1 - padded * (i + 1) / B)) for i in range(B)], device="cuda")[:, None]
        _, lse = K.attn_fwd(q, k, k, km, H, D, scale, 0.0, None, pick_splits(B, H, Nq, Nk))
        qf = q.float().view(1, Nq, H, D).transpose(1, 2) * scale
        kf = k.float().reshape(B, Nk, H, D).transpose(1, 2).contiguous()

        def aten():
            s = torch.matmul(qf, kf.transpose(-1, -2))
            if km is not None:
                s = s.masked_fill(km[:, None, None, :], float("-inf"))
            avg = torch.softmax(s, -1).mean(1)
            return avg, avg.sum(1)

        nsplit = pick_splits(B, H, Nq, Nk)

        def fwd_mass():  # what ops.attention_mass launches: the forward for its LSE (v := k), then the mass
            _, l2 = K.attn_fwd(q, k, k, km, H, D, scale, 0.0, None, nsplit)
            return K.attn_weights(q, k, km, l2, H, D, scale, False, True)

        sides = {"mass": lambda: K.attn_weights(q, k, km, lse, H, D, scale, False, True),
                 "fwd+mass": fwd_mass,
                 "avg+mass": lambda: K.attn_weights(q, k, km, lse, H, D, scale, True, True),
                 "aten": aten}
        _, m = sides["mass"]()
        ref = aten()[1]
        err = ((m - ref).norm() / ref.norm()).item()
        r = _ab(sides, a.inner, a.rounds)
        read = Nq * C * 2 + B * Nk * C * 2 + B * Nq * H * 4 + (B * Nk if km is not None else 0)
        floor = {"mass": (read + B * Nk * 4) / HBM * 1e6, "avg+mass": (read + B * Nk * 4 + B * Nq * Nk * 4) / HBM * 1e6}
        rows.append(dict(name=name, shape=(B, H, Nq, Nk, D), us=r, floor=floor, err=err))
        print(f"{name:9s} B{B} H{H} Nq{Nq} Nk{Nk} D{D}: " + "  ".join(
            f"{n} {r[n][0]:8.1f} us [{r[n][1]:.1f}, {r[n][2]:.1f}]" for n in r)
            + f"  floor mass {floor['mass']:.1f} / avg+mass {floor['avg+mass']:.1f} us, mass vs aten rel {err:.2e}", flush=True)
        del kv, kf, qf
        torch.cuda.empty_cache()
    return rows


def report(a, rows, resources):
    cell = lambda v: f"{v[0]:.1f} [{v[1]:.1f}, {v[2]:.1f}]"  # noqa: E731
    out = ["# Attention maps: `attn_weights` (`csrc/attn_weights.hip`)", "",
           f"Written by `tools/attn_maps_bench.py` on {torch.cuda.get_device_name(0)}: {a.inner} eager launches between two "
           f"device events, {a.rounds} alternating rounds, median [min, max] in µs.  All numbers of this file come from one "
           "process on one device.  Back-to-back launches on the same operands keep the smaller shapes in the cache "
           "hierarchy, so the floor (bytes once at 6.3 TB/s) is a lower bound on a cold call, not a roofline the warm "
           "loop must stay above.", "",
           "## Kernel level", "",
           "| shape (B, H, Nq, Nk, D) | mass only | avg + mass | `attn_fwd` + mass | ATen composition | ATen / mass | "
           "ATen / avg + mass | ATen / (`attn_fwd` + mass) | floor mass | mass / floor | floor avg + mass | "
           "avg + mass / floor | mass vs ATen (rel. Frobenius) |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        u, f = r["us"], r["floor"]
        out.append(f"| {r['name']} {r['shape']} | {cell(u['mass'])} | {cell(u['avg+mass'])} | {cell(u['fwd+mass'])} | "
                   f"{cell(u['aten'])} | {u['aten'][0] / u['mass'][0]:.1f}× | {u['aten'][0] / u['avg+mass'][0]:.1f}× | "
                   f"{u['aten'][0] / u['fwd+mass'][0]:.1f}× | {f['mass']:.1f} | "
                   f"{u['mass'][0] / f['mass']:.1f}× | {f['avg+mass']:.1f} | {u['avg+mass'][0] / f['avg+mass']:.1f}× | "
                   f"{r['err']:.1e} |")
    out += ["", "The ATen side is timed on operands already converted to fp32 and split into heads (its setup is not "
            "counted); the kernel side reads the bf16 projections as the fused layer holds them.  The \"mass only\" and "
            "\"avg + mass\" columns are the `attn_weights` launch alone, given an LSE; `ops.attention_mass` also pays for "
            "the `attn_fwd` call (`v := k`, output discarded) that produces that LSE, which the \"`attn_fwd` + mass\" "
            "column includes, so ATen / mass reads as kernel-only and ATen / (`attn_fwd` + mass) as the public op.  The "
            "floor counts K once: with more than one 32-query tile per chunk a wave reloads its K fragments per tile "
            "(mlm256: 8 tiles in 2 chunks, K read 4 times per chunk, from L1 / L2).  The last column compares "
            "bf16-operand MFMA scores with fp32 `matmul` scores of the same bf16 values.", ""]
    if resources:
        out += ["## Compile figures", "", resources.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print(f"wrote {a.out}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--resources", default=None, help="a markdown fragment with the compile's register / LDS figures to append")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_maps.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_maps_bench needs a GPU: timings from anything else say nothing")
    from perceiver_io_amd.ops import ext

    ext.require()
    rows = bench_kernels(a)
    resources = open(a.resources).read() if a.resources and os.path.exists(a.resources) else ""
    report(a, rows, resources)


if __name__ == "__main__":
    main()
