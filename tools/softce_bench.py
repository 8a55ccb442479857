"""Soft-target classifier head and batch mixing (``csrc/soft_ce_head.hip``) against the ATen
compositions on the same rows, and the training step with mixing on next to the hard-label step.

(a) the head alone, forward + backward, at (M, V, C) ∈ {(32, 1000, 128), (128, 10, 128), (128, 2, 64)}:
    ``soft_ce_fwd`` + ``soft_ce_bwd`` vs ``F.linear`` + ``F.cross_entropy`` with probability targets
    + ``argmax`` under bf16 autocast, forward and backward;
(b) ``batch_mix`` at the ImageNet (32, 224, 224, 3) and MNIST (128, 28, 28, 1) batch shapes vs
    ``torch.lerp`` (MixUp) / a masked ``torch.where`` (CutMix) with the weight / box on the device;
(c) the ``imagenet`` and ``mnist`` training steps of ``bench.py`` on the graph path: MixUp + CutMix +
    label smoothing through ``LitImageClassifier.step`` (a fresh host draw staged per step) next to
    the same model's hard-label step through ``PerceiverIO.loss``.

Device events around ``--iters`` calls after ``--warmup`` calls; the sides alternate in ``--rounds``
rounds and the median round is reported with the min–max spread.  Needs a GPU.

    python tools/softce_bench.py [--iters 200] [--warmup 20] [--rounds 5] [--steps 50] [--out profiles/soft_ce.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEAD_SHAPES = [(32, 1000, 128), (128, 10, 128), (128, 2, 64)]
MIX_SHAPES = {"imagenet": (32, 224, 224, 3), "mnist": (128, 28, 28, 1)}


def _time(fn, iters):
    """mean µs per call over ``iters`` calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def _ab(fns, iters, warmup, rounds):
    """{name: (median µs, min, max)} of the alternated sides"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            t[n].append(_time(fn, iters))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in t.items()}


def _fmt(r, n):
    return f"{n} {r[n][0]:8.1f} us [{r[n][1]:.1f}, {r[n][2]:.1f}]"


def bench_head(a, K):
    rows = []
    for M, V, C in HEAD_SHAPES:
        g = torch.Generator(device="cpu").manual_seed(0)
        h = torch.randn(M, C, generator=g).cuda()
        w32 = (torch.randn(V, C, generator=g) * 0.3).cuda().requires_grad_()
        bias = (torch.randn(V, generator=g) * 0.1).cuda().requires_grad_()
        la, lb = (torch.randint(0, V, (M,), generator=g).cuda() for _ in range(2))
        lam = torch.rand(M, generator=g).cuda()
        eps = 0.1
        w = w32.detach().to(torch.bfloat16)
        bd = bias.detach()
        gout = torch.ones(1, device="cuda")
        dH, dW, db = torch.empty(M, C, device="cuda"), torch.zeros(V, C, device="cuda"), torch.zeros(V, device="cuda")
        hr = h.clone().requires_grad_()

        def fused():
            loss, lse, pred, hs, cnt = K.soft_ce_fwd(h, la, lb, lam, w, bd, eps)
            K.soft_ce_bwd(hs, la, lb, lam, w, bd, eps, lse, gout, cnt, dH, dW, db, True)
            return loss, pred

        def aten():
            hr.grad = w32.grad = bias.grad = None
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = F.linear(hr, w32, bias)
            t = (1 - eps) * (lam[:, None] * F.one_hot(la, V) + (1 - lam[:, None]) * F.one_hot(lb, V)) + eps / V
            loss = F.cross_entropy(logits.float(), t)
            pred = logits.argmax(-1)
            loss.backward()
            return loss, pred

        fl, fp = fused()
        al, ap_ = aten()
        err = abs(fl.item() - al.item()) / abs(al.item())
        agree = (fp.long() == ap_).float().mean().item()
        r = _ab({"soft_ce": fused, "aten": aten}, a.iters, a.warmup, a.rounds)
        rows.append(dict(M=M, V=V, C=C, us=r, loss_rel_err_vs_bf16_aten=err, argmax_agreement=agree))
        print(f"head M={M:4d} V={V:5d} C={C:3d}: {_fmt(r, 'soft_ce')}   {_fmt(r, 'aten')}   "
              f"loss rel err {err:.2e}, argmax agreement {agree:.3f}", flush=True)
    return rows


def bench_mix(a, K):
    rows = []
    for name, shape in MIX_SHAPES.items():
        B, H, W, _ = shape
        g = torch.Generator(device="cpu").manual_seed(1)
        x = torch.randn(shape, generator=g).cuda()
        y = torch.randint(0, 10, (B,), generator=g).cuda()
        box = (H // 4, H // 4 + H // 2, W // 8, W // 8 + W // 2)
        lam_cut = 1.0 - (box[1] - box[0]) * (box[3] - box[2]) / float(H * W)
        words = {"mixup": torch.tensor([1.0, 0.3, 0, 0, 0, 0], device="cuda"),
                 "cutmix": torch.tensor([2.0, lam_cut, *map(float, box)], device="cuda")}
        # the ATen sides read the weight / the box from device tensors too (no host values baked in)
        lam_d = torch.tensor(0.7, device="cuda")  # lerp(x, xf, 1 − λ)
        ys, xs = torch.arange(H, device="cuda")[:, None], torch.arange(W, device="cuda")[None, :]
        bx = torch.tensor(box, device="cuda")

        def aten_mixup():
            return torch.lerp(x, x.flip(0), lam_d), y.flip(0)

        def aten_cutmix():
            m = (ys >= bx[0]) & (ys < bx[1]) & (xs >= bx[2]) & (xs < bx[3])
            return torch.where(m[None, :, :, None], x.flip(0), x), y.flip(0)

        for mode, aten in (("mixup", aten_mixup), ("cutmix", aten_cutmix)):
            mix = words[mode]
            out = K.batch_mix(x, y, mix)[0]
            err = (out - aten()[0]).abs().max().item()
            r = _ab({"batch_mix": lambda: K.batch_mix(x, y, mix), "aten": aten}, a.iters, a.warmup, a.rounds)
            rows.append(dict(config=name, shape=list(shape), mode=mode, us=r, max_abs_diff=err,
                             bytes_moved=2 * x.numel() * 4))
            print(f"batch_mix {name:8s} {mode:6s}: {_fmt(r, 'batch_mix')}   {_fmt(r, 'aten')}   max |diff| {err:.1e}",
                  flush=True)
    return rows


def bench_step(a):
    import bench
    from perceiver_io_amd.ops.optim import FusedAdamW
    from perceiver_io_amd.train.engine import StepEngine

    rows = []
    for cfg in ("imagenet", "mnist"):
        res = {}
        for side in ("hard", "mixed"):
            torch.manual_seed(0)
            args = bench.parse(["--config", cfg, "--gpus", "1"])
            lit, loss_fn, make_batch, _, lr, wd = bench.build(args, torch.device("cuda"))
            lit = lit.to("cuda")
            lit.train()
            if side == "mixed":
                lit.hparams.update(label_smoothing=0.1, mixup_alpha=0.8, cutmix_alpha=1.0)
                loss_fn = lambda b, lit=lit: lit.step(b)[0]  # noqa: E731
            opt = FusedAdamW(lit.parameters(), lr=lr, weight_decay=wd)
            eng = StepEngine(loss_fn, opt, device="cuda", graph=True, warmup_eager=2)
            g = torch.Generator().manual_seed(0)
            batch = tuple(t.cuda() for t in make_batch(g))

            def step(eng=eng, lit=lit, batch=batch, side=side):
                eng.step(lit.graph_batch(batch) if side == "mixed" else batch, ring_view=True)

            res[side] = step
        r = _ab(res, a.steps, max(5, a.steps // 5), a.rounds)
        rows.append(dict(config=cfg, us=r, added_us=r["mixed"][0] - r["hard"][0]))
        print(f"step {cfg:8s}: {_fmt(r, 'hard')}   {_fmt(r, 'mixed')}   added {r['mixed'][0] - r['hard'][0]:+.1f} us",
              flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50, help="training steps per timed round of part (c)")
    ap.add_argument("--skip-steps", action="store_true", help="parts (a) and (b) only")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("softce_bench needs a GPU: timings from anything else say nothing")
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops import ext

    K = ext.require()
    res = dict(device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, rounds=a.rounds, steps=a.steps,
               head=bench_head(a, K), batch_mix=bench_mix(a, K))
    if not a.skip_steps:
        res["step"] = bench_step(a)
    ops.check_device_errors()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
