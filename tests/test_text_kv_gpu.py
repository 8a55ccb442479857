"""The fused text input pass on the GPU: text_kv_fwd / text_kv_bwd (csrc/rowgemm.hip) against
embed_fwd + one ln_linear_fwd / ln_linear_bwd per layer, and the executor with TEXT_KV_FUSED on
against off (eager steps and a captured, replayed StepEngine graph)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
C, V, EPS, SCALE = 64, 50, 1e-5, 8.0
SHAPES = [(3, 40), (2, 64), (1, 7)]  # R = 120: partial last tile, tiles across samples; 128: two tiles; 7: < one tile


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


def _emu():
    from perceiver_io_amd.ops import emulation

    return emulation


def close(a, b, rel, name=""):
    """tests/test_kernels_gpu.py ``close``: relative Frobenius error ≤ min(rel, 1 %) and max-abs
    error ≤ rel × the reference's largest value."""
    a, b = a.float().cpu(), b.float().cpu()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    fro = ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()
    assert fro <= min(rel, 1e-2), f"{name}: relative Frobenius error {fro:.3e}"
    scale = b.abs().max().item() + 1e-6
    err = (a - b).abs().max().item()
    assert err <= rel * scale, f"{name}: max err {err:.3e} vs scale {scale:.3e}"


def _layer():
    return [1 + 0.3 * torch.randn(C, device=DEV), 0.2 * torch.randn(C, device=DEV),
            (torch.randn(2 * C, C, device=DEV) / 8).to(torch.bfloat16), 0.1 * torch.randn(2 * C, device=DEV)]


def _inputs(B, L, seed):
    torch.manual_seed(seed)
    ids = torch.randint(0, V, (B, L), device=DEV)
    return ids, 0.1 * torch.randn(V, C, device=DEV), 0.1 * torch.randn(L, C, device=DEV), _layer(), _layer()


@pytest.mark.parametrize("B,L", SHAPES)
def test_forward_equals_embed_then_two_projections(B, L):
    K = _ext()
    ids, E, P, la, lb = _inputs(B, L, 0)
    x, mean, rstd, kva, kvb = K.text_kv_fwd(ids, E, P, SCALE, EPS, la, lb)
    x0 = K.embed_fwd(ids, E, P, SCALE)
    assert torch.equal(x, x0)
    for l, kv in ((la, kva), (lb, kvb)):
        kv0, m0, r0 = K.ln_linear_fwd(x0.view(-1, C), l[0], l[1], EPS, l[2], l[3], 0, None, True, True)
        assert torch.equal(mean, m0) and torch.equal(rstd, r0)
        assert torch.equal(kv, kv0)


class _Slab:
    def __init__(self, R, sizes):
        self.offs, P = [], 0
        for n in sizes:
            self.offs.append(P)
            P += (n + 3) // 4 * 4
        self.sizes = sizes
        self.t = torch.full(((R + 63) // 64, P), float("nan"), device=DEV)

    def views(self):
        return [self.t[:, o:o + n] for o, n in zip(self.offs, self.sizes)]


SIZES = [C, C, 2 * C * C, 2 * C]


def _oracle_dx(ga, gb, x2, la, lb):
    """fp64, no bf16 rounding of activations or gradients (the weights are the bf16 ones)"""
    x = x2.double()
    mean = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt(x.var(-1, unbiased=False, keepdim=True) + EPS)
    xh = (x - mean) * rstd
    g = (ga.double() @ la[2].double()) * la[0].double() + (gb.double() @ lb[2].double()) * lb[0].double()
    return rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))


@pytest.mark.parametrize("B,L", SHAPES)
def test_backward_against_two_launches(B, L, capsys):
    """Slab partials bit-equal to the two-launch path (same products, same slab rows); dx within
    the existing ln_linear_bwd tolerance of the emulation, and no further from the fp64 oracle
    than the two-launch path's dx times 1.1 (the one new rounding is an fp32 add, far below the
    bf16 operand rounding both paths share).  A slab job left by a previous kernel rides along."""
    K, E_ = _ext(), _emu()
    R = B * L
    ids, E, P, la, lb = _inputs(B, L, 1)
    x, mean, rstd, _, _ = K.text_kv_fwd(ids, E, P, SCALE, EPS, la, lb)
    x2 = x.view(R, C)
    ga, gb = torch.randn(R, 2 * C, device=DEV), torch.randn(R, 2 * C, device=DEV)
    # a pending slab job of a previous kernel: 5 tiles of known partials into two destinations
    job = torch.randn(5, 72, device=DEV)
    jd = [torch.ones(40, device=DEV), torch.zeros(24, device=DEV)]
    new = _Slab(R, SIZES * 2)
    dx = K.text_kv_bwd(ga, gb, x2, mean, rstd, la[:3], lb[:3], new.views(), slab=True, job_slab=job, job_dsts=jd,
                       job_offs=[0, 48])
    close(jd[0], 1 + job[:, :40].sum(0), 1e-5, "job segment 0")
    close(jd[1], job[:, 48:72].sum(0), 1e-5, "job segment 1")
    old_a, old_b = _Slab(R, SIZES), _Slab(R, SIZES)
    d1 = K.ln_linear_bwd(ga, la[2], x2, mean, rstd, la[0], la[1], None, True, *old_a.views(), slab=True)
    d2 = K.ln_linear_bwd(gb, lb[2], x2, mean, rstd, lb[0], lb[1], d1, True, *old_b.views(), slab=True)
    names = ("dgamma", "dbeta", "dW", "dbias")
    for i, (t_new, t_old) in enumerate(zip(new.views(), old_a.views() + old_b.views())):
        assert torch.equal(t_new, t_old), names[i % 4] + " layer " + "ab"[i // 4]
    emu_t = [torch.zeros(n, device=DEV) for n in SIZES * 2]
    dx_e = E_.text_kv_bwd(ga, gb, x2, mean, rstd, la[:3], lb[:3], emu_t)
    close(dx, dx_e, 3e-2, "dx")
    for i, t in enumerate(emu_t):
        close(new.views()[i].sum(0), t, 1e-4 if i % 4 == 3 else 3e-2, names[i % 4] + " vs emulation")
    ref = _oracle_dx(ga, gb, x2, la, lb)
    e_new = ((dx.double() - ref).norm() / ref.norm()).item()
    e_old = ((d2.double() - ref).norm() / ref.norm()).item()
    with capsys.disabled():
        print(f"\n[text_kv_bwd R={R}] dx error vs fp64 oracle: fused {e_new:.4e}, two launches {e_old:.4e}")
    assert e_new <= 1.1 * e_old, (e_new, e_old)


def _mlm(layers=2, L=40):
    from perceiver_io_amd.tasks import LitMaskedLanguageModel

    return LitMaskedLanguageModel(vocab_size=V, max_seq_len=L,
                                  optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3}},
                                  num_latents=8, num_latent_channels=C, num_encoder_layers=layers,
                                  num_encoder_self_attention_layers_per_block=1).cuda()


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _loss_and_grads(m, ids, pad, xm, lab):
    from perceiver_io_amd import ops

    m.zero_grad()
    with ops.backend("hip"):
        loss = m.loss(ids, pad, labels=lab, x_masked=xm)
        loss.backward()
    return loss.item(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("layers,frozen", [(2, False), (3, False), (2, True)])
def test_model_fused_on_matches_off(layers, frozen, monkeypatch):
    """layers = 3: layer_n applied twice (its dK|dV accumulated before the shared backward);
    frozen: layer_n's kv_norm weight does not require grad.  Loss equal (the forward is the same
    arithmetic), every gradient within test_mlm_fused_matches_eager's per-tensor 2e-2."""
    from perceiver_io_amd import ops

    torch.manual_seed(0)
    m = _mlm(layers).model
    if frozen:
        m.encoder.layer_n[0][0].module.kv_norm.weight.requires_grad_(False)
    ids = torch.randint(3, V, (2, 40), device=DEV)
    pad = torch.zeros(2, 40, dtype=torch.bool, device=DEV)
    pad[1, 30:] = True
    xm, lab = m.masking(ids, pad)
    launches = []
    K = _ext()
    real = K.text_kv_bwd
    monkeypatch.setattr(K, "text_kv_bwd", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    monkeypatch.setattr(ops.fused, "TEXT_KV_FUSED", True)
    l_on, g_on = _loss_and_grads(m, ids, pad, xm, lab)
    assert len(launches) == 1
    monkeypatch.setattr(ops.fused, "TEXT_KV_FUSED", False)
    l_off, g_off = _loss_and_grads(m, ids, pad, xm, lab)
    assert len(launches) == 1
    assert l_on == l_off
    assert g_on.keys() == g_off.keys()
    bad = {n: _rel(g_on[n], g) for n, g in g_off.items() if g.norm() > 0 and _rel(g_on[n], g) > 2e-2}
    assert not bad, bad


def test_captured_steps_fused_on_matches_off(monkeypatch):
    """StepEngine with graph capture, replayed twice with different token ids: the KVSource entries
    filled in during capture hold nothing of a step (losses follow the per-layer path's)."""
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops.optim import FusedAdamW
    from perceiver_io_amd.train.engine import StepEngine

    torch.manual_seed(1)
    batches = [torch.randint(3, V, (2, 40), device=DEV) for _ in range(3)]
    pad = torch.zeros(2, 40, dtype=torch.bool, device=DEV)
    losses = {}
    for on in (True, False):
        monkeypatch.setattr(ops.fused, "TEXT_KV_FUSED", on)
        torch.manual_seed(2)
        m = _mlm().model
        with torch.no_grad():
            lab = batches[0].clone()
            lab[:, ::2] = -100
        opt = FusedAdamW(m.parameters(), lr=1e-3)
        eng = StepEngine(lambda b: m.loss(b[1], b[2], labels=lab, x_masked=b[1]), opt, device=DEV, graph=True,
                         warmup_eager=0)
        losses[on] = [eng.step((None, ids, pad)).item() for ids in batches]
        assert eng.captures == 1
    assert len(set(losses[True])) == 3  # every replay saw its own ids
    for a, b in zip(losses[True], losses[False]):
        assert abs(a - b) <= 1e-3 * abs(b), losses


_CHECKED_PROBE = r"""
import torch
from perceiver_io_amd.ops import ext
K = ext.require()
assert K.checked_build() and K.__name__.endswith("_C_check"), K.__name__
dev = "cuda"
E, P = torch.randn(50, 64, device=dev), torch.randn(8, 64, device=dev)
l = [torch.ones(64, device=dev), torch.zeros(64, device=dev), torch.randn(128, 64, device=dev).to(torch.bfloat16),
     torch.zeros(128, device=dev)]
K.text_kv_fwd(torch.randint(0, 50, (2, 8), device=dev), E, P, 1.0, 1e-5, l, l)
assert K.check_errors(True) == 0
try:
    K.text_kv_fwd(torch.tensor([[3, 50, 1, 2, 0, 0, 0, 0]], device=dev), E, P, 1.0, 1e-5, l, l)
    raise SystemExit("an id equal to V was not flagged")
except RuntimeError as e:
    assert "checked build" in str(e), e
assert K.check_errors(True) == 0
print("CHECKED_OK")
"""


def test_checked_build_flags_id_equal_to_vocab():
    """The checked variant flags an id equal to V in text_kv_fwd as it does in embed_fwd (a child
    process: the loaded variant is process-wide)."""
    import os
    import subprocess
    import sys

    from perceiver_io_amd.csrc.build import ext_path

    assert ext_path("_C_check").exists(), "the checked extension is not built"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PERCEIVER_CHECKED="1", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", _CHECKED_PROBE], env=env, capture_output=True, text=True, timeout=240,
                       cwd=root)
    assert r.returncode == 0 and "CHECKED_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
