"""Vocabulary top-k head (``csrc/topk_head.hip``) against the ATen path on the same rows.

(a) the kernel pair ``vocab_topk`` vs ``F.linear(bf16) → float → topk`` + ``logsumexp`` on the same
    selected rows, for (M, V, C, k) ∈ {(64, 10003, 64, 5), (4992, 10003, 64, 5), (128, 1000, 128, 5)};
(b) ``predict_masked_samples`` end to end (64 sequences of L = 512, one ``[MASK]`` each): the fused
    path (``predict_topk``: only the ``[MASK]`` positions decoded) vs the materialising path
    (``model(ids, pad, masking=False)`` → ``(n, L, V)`` logits → ``topk``), with the peak of
    ``torch.cuda.max_memory_allocated`` over each.

Device events around ``--iters`` calls after ``--warmup`` calls; the two sides alternate in
``--rounds`` rounds and the median round is reported with the min–max spread.  Needs a GPU.

    python tools/topk_bench.py [--iters 200] [--warmup 20] [--rounds 5] [--out profiles/topk_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(64, 10003, 64, 5), (4992, 10003, 64, 5), (128, 1000, 128, 5)]


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


def bench_head(a, K):
    rows = []
    for M, V, C, k in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(0)
        R = 2 * M  # the selected rows are gathered out of a larger hidden state, as in prediction
        h = torch.randn(R, C, generator=g).cuda()
        w32 = (torch.randn(V, C, generator=g) * 0.3).cuda()
        w = w32.to(torch.bfloat16)
        bias = (torch.randn(V, generator=g) * 0.1).cuda()
        idx = torch.randperm(R, generator=g)[:M].cuda()
        bias16 = bias.to(torch.bfloat16)

        def fused():
            return K.vocab_topk(h, idx, w, bias, k)

        def aten():
            logits = F.linear(h.index_select(0, idx).to(torch.bfloat16), w, bias16).float()
            v, i = logits.topk(k, dim=-1)
            return v, i, torch.logsumexp(logits, -1)

        # same answer first (section 6 of the measuring notes): values against the bf16 ATen logits
        fv, fi, fl = fused()
        av, ai, al = aten()
        err = ((fv - av).norm() / av.norm()).item()
        agree = (fi[:, 0] == ai[:, 0]).float().mean().item()
        r = _ab({"vocab_topk": fused, "aten": aten}, a.iters, a.warmup, a.rounds)
        rows.append(dict(M=M, V=V, C=C, k=k, us=r, value_rel_err_vs_bf16_logits=err, top1_agreement=agree,
                         model_gflop=2.0 * M * V * C / 1e9))
        print(f"M={M:5d} V={V:5d} C={C:3d} k={k}: vocab_topk {r['vocab_topk'][0]:8.1f} us "
              f"[{r['vocab_topk'][1]:.1f}, {r['vocab_topk'][2]:.1f}]   aten {r['aten'][0]:8.1f} us "
              f"[{r['aten'][1]:.1f}, {r['aten'][2]:.1f}]   values rel err {err:.2e}, top-1 agreement {agree:.3f}",
              flush=True)
    return rows


def bench_fill_mask(a):
    from perceiver_io_amd import ops
    from perceiver_io_amd.data.imdb import Collator, shipped_tokenizer
    from perceiver_io_amd.tasks import LitMaskedLanguageModel
    from perceiver_io_amd.utils.misc import predict_masked_samples
    from perceiver_io_amd.utils.tokenizer import load_tokenizer

    torch.manual_seed(0)
    tok = load_tokenizer(shipped_tokenizer(10003))
    V, L, n, k = tok.get_vocab_size(), 512, 64, 5
    lit = LitMaskedLanguageModel(vocab_size=V, max_seq_len=L,
                                 optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3}},
                                 num_latents=64, num_latent_channels=64, num_encoder_layers=3,
                                 num_encoder_self_attention_layers_per_block=6).cuda().eval()
    model = lit.model
    collator = Collator(tok, L, pad_to_max=True)
    samples = [f"i have watched this [MASK] and it was awesome {i}" for i in range(n)]
    ids, pad = (t.cuda() for t in collator.encode(samples))
    assert ids.shape == (n, L) and int((ids == tok.token_to_id("[MASK]")).sum()) == n

    def encode(_):  # tokenised once: the timing is of the model side
        return ids, pad

    class _NoTopk:  # the same model behind a plain callable (no PerceiverMLM): the utility's materialising path
        def __init__(self, m):
            self.m, self.training = m, m.training

        def __call__(self, *args, **kw):
            return self.m(*args, **kw)

        def eval(self):
            self.m.eval()

        def train(self, mode=True):
            self.m.train(mode)

    sides = {"predict_topk": lambda: predict_masked_samples(samples, encode, tok, model, k, device="cuda"),
             "materialise": lambda: predict_masked_samples(samples, encode, tok, _NoTopk(model), k, device="cuda")}
    assert ops.use_hip(ids)
    out = {}
    peaks = {}
    for name, fn in sides.items():
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated()
    r = _ab(sides, max(1, a.iters // 10), max(1, a.warmup // 10), a.rounds)
    for name in sides:
        out[name] = dict(us=r[name], peak_bytes=peaks[name])
        print(f"predict_masked_samples n={n} L={L} k={k} [{name:12s}] {r[name][0] / 1e3:8.2f} ms "
              f"[{r[name][1] / 1e3:.2f}, {r[name][2] / 1e3:.2f}]   peak {peaks[name] / 1e6:8.1f} MB", flush=True)
    out["logits_bytes"] = n * L * V * 4
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench needs a GPU: timings from anything else say nothing")
    from perceiver_io_amd.ops import ext

    K = ext.require()
    res = dict(device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, rounds=a.rounds,
               head=bench_head(a, K), fill_mask=bench_fill_mask(a))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
