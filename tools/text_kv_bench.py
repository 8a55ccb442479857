"""The fused text input pass (``csrc/rowgemm.hip`` text_kv_fwd / text_kv_bwd) against the launches
it replaces, each side as one captured graph, at the benchmark configs' text shapes:

  forward : embed_fwd + ln_linear_fwd × 2            against  text_kv_fwd
  backward: ln_linear_bwd × 2 (the second adds the   against  text_kv_bwd
            first one's partial dx as its residual)

hipGraph replays of ``--inner`` repetitions in windows of at least ``--window`` seconds, alternating
rounds, median [min, max] (the loop of ``tools/ema_bench.py``).  The last columns set the bytes the
fused kernel must move (forward: x, mean/rstd and two bf16 K|V out; backward: two fp32 dK|dV and x
in, dx and the per-tile gradient slab out) against its time.  Nothing here asserts a budget.

    python tools/text_kv_bench.py [--rounds 5] [--window 0.3] [--inner 10] [--out FILE]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.ema_bench import _ab, _graph_of, _window  # noqa: E402

C, V, EPS = 64, 10003, 1e-5
SHAPES = (("mlm256 (headline)", 64, 512), ("long_mlm", 8, 8192), ("mlm64 / seq_clf_ft", 128, 512))
SIZES = [C, C, 2 * C * C, 2 * C]


def _slab(R, sizes):
    offs, P = [], 0
    for n in sizes:
        offs.append(P)
        P += (n + 3) // 4 * 4
    t = torch.empty(((R + 63) // 64, P), device="cuda")
    return t, [t[:, o:o + n] for o, n in zip(offs, sizes)]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from perceiver_io_amd.ops import ext

    K = ext.require()
    lines = ["| shape | rows | side | old path µs | fused µs | fused bytes | fused TB/s |", "|---|---:|---|---:|---:|---:|---:|"]
    for name, B, L in SHAPES:
        torch.manual_seed(0)
        R = B * L
        ids = torch.randint(0, V, (B, L), device="cuda")
        E, P = 0.1 * torch.randn(V, C, device="cuda"), 0.1 * torch.randn(L, C, device="cuda")
        lay = [[1 + 0.3 * torch.randn(C, device="cuda"), 0.2 * torch.randn(C, device="cuda"),
                (torch.randn(2 * C, C, device="cuda") / 8).to(torch.bfloat16), 0.1 * torch.randn(2 * C, device="cuda")]
               for _ in range(2)]
        x, mean, rstd, _, _ = K.text_kv_fwd(ids, E, P, 8.0, EPS, lay[0], lay[1])
        x2 = x.view(R, C)
        g = [torch.randn(R, 2 * C, device="cuda") for _ in range(2)]
        _, va = _slab(R, SIZES)
        _, vb = _slab(R, SIZES)
        _, vf = _slab(R, SIZES * 2)

        def fwd_old():
            y = K.embed_fwd(ids, E, P, 8.0).view(R, C)
            for l in lay:
                K.ln_linear_fwd(y, l[0], l[1], EPS, l[2], l[3], 0, None, True, True)

        def bwd_old():
            d = K.ln_linear_bwd(g[1], lay[1][2], x2, mean, rstd, lay[1][0], lay[1][1], None, True, *vb, slab=True)
            K.ln_linear_bwd(g[0], lay[0][2], x2, mean, rstd, lay[0][0], lay[0][1], d, True, *va, slab=True)

        sides = {"fwd old": fwd_old, "fwd fused": lambda: K.text_kv_fwd(ids, E, P, 8.0, EPS, lay[0], lay[1]),
                 "bwd old": bwd_old,
                 "bwd fused": lambda: K.text_kv_bwd(g[0], g[1], x2, mean, rstd, lay[0][:3], lay[1][:3], vf, slab=True)}
        graphs = {k: _graph_of(f, a.inner) for k, f in sides.items()}
        for gr in graphs.values():
            _window(gr, a.inner, 0.05)
        r = _ab(graphs, lambda gr: _window(gr, a.inner, a.window), a.rounds)
        nbytes = {"fwd": R * (C * 4 + 8 + 2 * 2 * C * 2),
                  "bwd": R * (2 * 2 * C * 4 + C * 4 + 8 + C * 4) + vf[0].shape[0] * 2 * sum(SIZES) * 4}
        for side in ("fwd", "bwd"):
            o, f = r[side + " old"], r[side + " fused"]
            lines.append(f"| {name} | {R} | {side} | {o[0]:.1f} [{o[1]:.1f}, {o[2]:.1f}] | {f[0]:.1f} [{f[1]:.1f}, {f[2]:.1f}] "
                         f"| {nbytes[side] / 1e6:.1f} MB | {nbytes[side] / f[0] / 1e6:.2f} |")
            print(lines[-1], flush=True)
        del graphs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
