"""Vocabulary top-k head on the GPU (``csrc/topk_head.hip``): the kernel pair against its
emulation, the tie rule, the dispatcher, and ``predict_topk`` / ``predict_masked_samples`` on
the fused path against the eager fp32 path of the same model."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (M, V, C, k): many splits + ragged last chunk; > 2 row blocks; one row past a block, Kt = 8;
# one vocab entry past a chunk, wide head; a single partial chunk; classifier, V < 32, Kt = 1;
# k close to V
CASES = [(77, 10003, 64, 5), (300, 1000, 64, 3), (129, 2003, 64, 8), (33, 257, 128, 5), (130, 70, 64, 8),
         (5, 3, 64, 1), (6, 10, 128, 8)]

# fused bf16 path against eager fp32 on model outputs: the relative bound that
# tests/test_model_gpu.py::test_mlm_fused_matches_eager (the MLM) and its _three_way helper
# (test_image_classifier_fused_matches_eager, ``loss_tol=1e-2``) put on the fused loss of these
# two models against eager fp32 — the tightest figure that file allows between the two paths for
# this family (its per-tensor tolerance is 2e-2).  The loss is lse − logit[label], so the same
# figure bounds the top-k logits and the lse here.
MODEL_TOL = 1e-2


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


def _emu():
    from perceiver_io_amd.ops import emulation

    return emulation


def bf(x):
    return x.to(torch.bfloat16)


def rel_fro(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


_inputs = {}


def _case(M, V, C, k):
    """inputs as in test_fused_cross_entropy, the emulation's answer and the full reference
    logits: computed once per case, shared and never modified"""
    key = (M, V, C, k)
    if key not in _inputs:
        g = torch.Generator(device=DEV).manual_seed(5 + M + V)
        hf = bf(torch.randn(M, C, device=DEV, generator=g)).float()  # bf16-exact fp32 rows
        w = bf(torch.randn(V, C, device=DEV, generator=g) * 0.3)
        bias = torch.randn(V, device=DEV, generator=g) * 0.1
        ref = hf @ w.float().t() + bias
        _inputs[key] = (hf, w, bias, ref, _emu().vocab_topk(hf, None, w, bias, k))
    return _inputs[key]


def _gathered_logit_check(ref, values, indices, rel):
    """for every row and rank: the logit at the returned index is as large as the true one of
    that rank, and the returned value is the logit at that index — both to ``rel``·max|ref|
    (accepts any correct answer under near-ties and leaves no row out)"""
    k = values.shape[1]
    bound = rel * ref.abs().max().item()
    at = ref.gather(1, indices)
    e_rank = (at - ref.topk(k, dim=-1).values).abs().max().item()
    e_val = (at - values).abs().max().item()
    print(f"gathered-logit check: rank error {e_rank:.3e}, value error {e_val:.3e}, bound {bound:.3e}")
    assert e_rank <= bound, (e_rank, bound)
    assert e_val <= bound, (e_val, bound)


@pytest.mark.parametrize("M,V,C,k", CASES)
def test_vocab_topk_matches_emulation(M, V, C, k):
    hf, w, bias, ref, (ev, ei, el) = _case(M, V, C, k)
    values, indices, lse = _ext().vocab_topk(hf, None, w, bias, k)
    assert values.shape == (M, k) and indices.shape == (M, k) and lse.shape == (M,)
    assert values.dtype == torch.float32 and indices.dtype == torch.int64 and lse.dtype == torch.float32
    print(f"values {rel_fro(values, ev):.3e}, lse {rel_fro(lse, el):.3e}")
    assert rel_fro(values, ev) < 1e-3 and rel_fro(lse, el) < 1e-3
    assert (indices >= 0).all() and (indices < V).all()
    assert (indices.sort(dim=-1).values.diff(dim=-1) > 0).all()  # distinct within a row
    assert (values.diff(dim=-1) <= 0).all()  # non-increasing
    # fp32 accumulation-order error over C ≤ 128 bf16-exact products ≈ C·2⁻²³ of scale ≈ 1e-5
    _gathered_logit_check(ref, values, indices, 1e-4)


@pytest.mark.parametrize("M,V,C,k", [CASES[0], CASES[3], CASES[5]])
def test_vocab_topk_gathered_rows(M, V, C, k):
    hf, w, bias, _, _ = _case(M, V, C, k)
    direct = _ext().vocab_topk(hf, None, w, bias, k)
    idx = torch.randperm(2 * M, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))[:M]
    hbig = torch.zeros(2 * M, C, device=DEV)
    hbig[idx] = hf
    gathered = _ext().vocab_topk(hbig, idx, w, bias, k)
    assert all(torch.equal(a, b) for a, b in zip(gathered, direct))


@pytest.mark.parametrize("dup", [200, 21, 18, 49, 81])
def test_vocab_topk_tie_rule(dup):
    """two vocabulary rows with identical weights and bias give bit-identical logits: the lower
    index comes first.  V = 300 runs as two vocab splits of three and two chunks: 200 lies in the
    other split, 21 = 17 + 4 in the other lane half of the same tile, 18 in the same lane, 49 in
    the next tile and 81 in the next chunk of the same lane."""
    g = torch.Generator(device=DEV).manual_seed(7)
    M, V, C = 40, 300, 64
    w = bf(torch.randn(V, C, device=DEV, generator=g) * 0.3)
    bias = torch.randn(V, device=DEV, generator=g) * 0.1
    w[dup], bias[dup] = w[17], bias[17]
    hf = bf(8.0 * w[17].float()[None, :] + 0.05 * torch.randn(M, C, device=DEV, generator=g)).float()
    ref = hf @ w.float().t() + bias
    top3 = ref.topk(3, dim=-1)
    # on the reference logits: the pair is every row's maximum, clear of the third
    assert (top3.indices[:, :2].sort(dim=-1).values == torch.tensor(sorted((17, dup)), device=DEV)).all()
    assert (top3.values[:, 1] - top3.values[:, 2] > 1e-2 * ref.abs().max()).all()
    for k in (2, 5, 8):
        values, indices, _ = _ext().vocab_topk(hf, None, w, bias, k)
        assert (indices[:, 0] == 17).all() and (indices[:, 1] == dup).all()
        assert torch.equal(values[:, 0], values[:, 1])
    ei = _emu().vocab_topk(hf, None, w, bias, 2)[1]
    assert (ei[:, 0] == 17).all() and (ei[:, 1] == dup).all()


def test_vocab_topk_is_repeatable():
    hf, w, bias, _, _ = _case(*CASES[0])
    outs = [_ext().vocab_topk(hf, None, w, bias, CASES[0][3]) for _ in range(3)]
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))


def test_vocab_topk_empty():
    w = bf(torch.randn(50, 64, device=DEV))
    bias = torch.zeros(50, device=DEV)
    for h, idx in ((torch.zeros(0, 64, device=DEV), None),
                   (torch.zeros(4, 64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV))):
        values, indices, lse = _ext().vocab_topk(h, idx, w, bias, 3)
        assert values.shape == (0, 3) and indices.shape == (0, 3) and lse.shape == (0,)
        assert indices.dtype == torch.int64


def test_vocab_topk_dispatcher():
    """ops.mlm_head.vocab_topk: the kernel for C ∈ {64, 128}, k ≤ 8 (over the bf16 weight shadow);
    k = 9 and C = 32 take the PyTorch path on the selected rows and raise nothing"""
    from perceiver_io_amd.ops.mlm_head import vocab_topk

    g = torch.Generator(device=DEV).manual_seed(11)
    M, V = 50, 700
    for C, k, kernel in ((64, 5, True), (128, 8, True), (64, 9, False), (32, 5, False)):
        h = torch.randn(3, 40, C, device=DEV, generator=g)
        weight = torch.randn(V, C, device=DEV, generator=g) * 0.3
        bias = torch.randn(V, device=DEV, generator=g) * 0.1
        idx = torch.randperm(120, device=DEV, generator=g)[:M]
        values, indices, lse = vocab_topk(h, weight, bias, k, idx=idx)
        assert values.shape == (M, k) and indices.shape == (M, k) and lse.shape == (M,)
        if kernel:
            ev, _, el = _emu().vocab_topk(h.reshape(-1, C), idx, bf(weight), bias, k)
            assert rel_fro(values, ev) < 1e-3 and rel_fro(lse, el) < 1e-3
            _gathered_logit_check(bf(h.reshape(-1, C)[idx]).float() @ bf(weight).float().t() + bias, values, indices, 1e-4)
            # a head without a bias
            nv, ni, nl = vocab_topk(h, weight, None, k, idx=idx)
            zv, zi, zl = vocab_topk(h, weight, torch.zeros_like(bias), k, idx=idx)
            assert torch.equal(nv, zv) and torch.equal(ni, zi) and torch.equal(nl, zl)
        else:
            logits = F.linear(h.reshape(-1, C)[idx], weight, bias).float()
            tv, ti = logits.topk(k, dim=-1)
            assert torch.equal(values, tv) and torch.equal(indices, ti)
            assert torch.equal(lse, torch.logsumexp(logits, -1))


def _mlm(vocab=10003, L=96):
    from perceiver_io_amd.tasks import LitMaskedLanguageModel

    return LitMaskedLanguageModel(vocab_size=vocab, max_seq_len=L,
                                  optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3}},
                                  num_latents=64, num_latent_channels=64, num_encoder_layers=1,
                                  num_encoder_self_attention_layers_per_block=2).to(DEV).eval()


def test_mlm_predict_topk_matches_eager_logits():
    """[MASK] counts 0, 1 and 7 per sequence, one padded tail: the fused path (only the mask
    positions decoded, no logits) against the full fp32 logits of the eager backend"""
    from perceiver_io_amd import ops

    torch.manual_seed(0)
    V, L, k = 10003, 96, 5
    m = _mlm(V, L).model
    mask_id = m.masking.mask_token_id
    ids = torch.randint(3, V, (3, L))
    ids[1, 40] = mask_id
    ids[2, [0, 3, 4, 31, 32, 63, 70]] = mask_id
    pad = torch.zeros(3, L, dtype=torch.bool)
    pad[2, 80:] = True
    ids[2, 80:] = 0
    ids, pad = ids.to(DEV), pad.to(DEV)
    positions = ids == mask_id
    with ops.backend("torch"), torch.no_grad():
        logits, _ = m(ids, pad, masking=False)
        ref = logits[positions].float()
    assert ops.use_hip(ids)
    where, values, indices, lse = m.predict_topk(ids, pad, k=k)
    assert torch.equal(where, positions.nonzero()) and where.shape == (8, 2)
    assert values.shape == (8, k) and indices.shape == (8, k) and lse.shape == (8,)
    tv = ref.topk(k, dim=-1).values
    print(f"values {rel_fro(values, tv):.3e}, lse {rel_fro(lse, torch.logsumexp(ref, -1)):.3e}")
    assert rel_fro(values, tv) < MODEL_TOL
    assert rel_fro(lse, torch.logsumexp(ref, -1)) < MODEL_TOL
    _gathered_logit_check(ref, values, indices, MODEL_TOL)
    # a batch without any [MASK]
    w0, v0, i0, l0 = m.predict_topk(ids[:1], pad[:1], k=k)
    assert w0.shape == (0, 2) and v0.shape == (0, k) and i0.shape == (0, k) and l0.shape == (0,)


_MEMORY_PROBE = r"""
import torch
from perceiver_io_amd import ops
from perceiver_io_amd.data.imdb import Collator, shipped_tokenizer
from perceiver_io_amd.tasks import LitMaskedLanguageModel
from perceiver_io_amd.utils.misc import predict_masked_samples
from perceiver_io_amd.utils.tokenizer import load_tokenizer

torch.manual_seed(0)
tok = load_tokenizer(shipped_tokenizer(10003))
V, L, n, k = tok.get_vocab_size(), 512, 8, 3
model = LitMaskedLanguageModel(vocab_size=V, max_seq_len=L,
                               optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3}},
                               num_latents=64, num_latent_channels=64, num_encoder_layers=1,
                               num_encoder_self_attention_layers_per_block=2).cuda().eval().model
collator = Collator(tok, L, pad_to_max=True)
samples = ["i have watched this [MASK] and it was awesome", "a [MASK] show about [MASK] people"] * (n // 2)
ids, _ = collator.encode(samples)
assert ids.shape == (n, L) and ops.use_hip(ids.cuda())
torch.cuda.synchronize()
held = torch.cuda.memory_allocated()
torch.cuda.reset_peak_memory_stats()
out = predict_masked_samples(samples, collator.encode, tok, model, num_predictions=k, device="cuda")
torch.cuda.synchronize()
peak = torch.cuda.max_memory_allocated()
print(f"peak {peak / 1e6:.1f} MB ({held / 1e6:.1f} MB held before the call), bound {n * L * V * 4 / 1e6:.1f} MB")
assert peak < n * L * V * 4, (peak, n * L * V * 4)
assert len(out) == n and all(len(o) == k for o in out)
assert all(isinstance(s, str) and "[MASK]" not in s for o in out for s in o)
assert not model.training
print("MEMORY_OK")
"""


def test_predict_masked_samples_keeps_no_logits_tensor():
    """fill-mask on the GPU decodes only the [MASK] positions: ``torch.cuda.max_memory_allocated``
    over the call, the peak reset first, stays below one (n, L, V) fp32 logits tensor (n = 8,
    L = 512, V = 10003: 164 MB), model included.  Runs in a child process, so the peak is that
    of this model and this call alone (the suite's process holds other tests' tensors)."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", _MEMORY_PROBE], env=env, capture_output=True, text=True, timeout=240,
                       cwd=root)
    print(r.stdout[-500:])
    assert r.returncode == 0 and "MEMORY_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_predict_masked_samples_other_models_keep_the_materialising_path():
    """only a PerceiverMLM takes the fused path: any other callable with the model's forward
    (here a wrapper; a PerceiverIO has a predict_topk of another signature) runs as before"""
    from perceiver_io_amd.data.imdb import Collator, shipped_tokenizer
    from perceiver_io_amd.utils.misc import predict_masked_samples
    from perceiver_io_amd.utils.tokenizer import load_tokenizer

    torch.manual_seed(0)
    tok = load_tokenizer(shipped_tokenizer(10003))
    L, k = 64, 2
    model = _mlm(tok.get_vocab_size(), L).model

    class Wrapped(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.m = m

        def forward(self, *a, **kw):
            return self.m(*a, **kw)

        def predict_topk(self, x, pad_mask=None, k=1):  # the classifier's signature: must not be called
            raise AssertionError("predict_topk of a non-MLM model was called")

    collator = Collator(tok, L, pad_to_max=True)
    samples = ["i have watched this [MASK] and it was awesome", "a [MASK] show"]
    out = predict_masked_samples(samples, collator.encode, tok, Wrapped(model), num_predictions=k, device=DEV)
    assert len(out) == 2 and all(len(o) == k for o in out)
    assert all(isinstance(s, str) and "[MASK]" not in s for o in out for s in o)


def test_classifier_predict_topk_matches_eager_argmax():
    """the small image classifier of the three-way tests (test_model_gpu.py): the fused argmax
    equals the eager fp32 argmax wherever that backend's top-2 logits are further apart than the
    tolerance; seed and batch are such that ≥ 90 % of the rows qualify"""
    from perceiver_io_amd import ops
    from perceiver_io_amd.tasks import LitImageClassifier

    torch.manual_seed(13)
    lit = LitImageClassifier(image_shape=(28, 28, 1), num_classes=10,
                             optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3}},
                             num_latents=32, num_latent_channels=128, num_encoder_layers=3,
                             num_encoder_cross_attention_heads=4, num_encoder_self_attention_layers_per_block=2,
                             num_decoder_cross_attention_heads=1).eval()
    x = torch.randn(64, 28, 28, 1)
    m, x = lit.model.to(DEV), x.to(DEV)
    with ops.backend("torch"), torch.no_grad():
        ref = m(x).float()
    top2 = ref.topk(2, dim=-1).values
    clear = (top2[:, 0] - top2[:, 1]) > MODEL_TOL * ref.abs().max()
    print(f"rows with a clear argmax: {int(clear.sum())} / 64")
    assert clear.float().mean().item() >= 0.9
    values, indices, lse = m.predict_topk(x, k=3)
    assert values.shape == (64, 3) and indices.shape == (64, 3) and lse.shape == (64,)
    assert torch.equal(indices[clear, 0], ref.argmax(-1)[clear])
    assert rel_fro(lse, torch.logsumexp(ref, -1)) < MODEL_TOL
    i1 = m.predict_topk(x)[1]  # k = 1: the Kt = 1 instance
    assert torch.equal(i1[:, 0], indices[:, 0])


_CHECKED_PROBE = r"""
import torch
from perceiver_io_amd.ops import ext
K = ext.require()
assert K.checked_build()
h = torch.randn(16, 64, device="cuda")
w = (torch.randn(100, 64, device="cuda") * 0.3).to(torch.bfloat16)
b = torch.zeros(100, device="cuda")
idx = torch.tensor([0, 15, 3], device="cuda")
v, i, l = K.vocab_topk(h, idx, w, b, 4)
torch.cuda.synchronize()
assert K.check_errors(True) == 0
for bad in (16, -1):
    idx2 = torch.tensor([0, bad, 3], device="cuda")
    try:
        K.vocab_topk(h, idx2, w, b, 4)
        raise SystemExit("no error raised")
    except RuntimeError as e:
        assert "checked build" in str(e) and "vocab_topk" in str(e), e
assert K.check_errors(True) == 0
v2, i2, l2 = K.vocab_topk(h, idx, w, b, 4)
assert torch.equal(v, v2) and torch.equal(i, i2) and torch.equal(l, l2)
print("CHECKED_OK")
"""


def test_checked_build_flags_out_of_range_gather_rows():
    """the checked variant (PERCEIVER_CHECKED=1) clamps an ``idx`` entry outside [0, R) and
    raises; valid inputs pass.  Runs in a child process (the loaded variant is process-wide)."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PERCEIVER_CHECKED="1", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", _CHECKED_PROBE], env=env, capture_output=True, text=True, timeout=240,
                       cwd=root)
    assert r.returncode == 0 and "CHECKED_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
