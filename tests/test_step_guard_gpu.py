"""The step guard and the per-tensor statistics on the GPU (csrc/health.hip and the ``guard`` argument
of the flat-space update kernels), on the flat case of tests/optim_cases.py: ten tensors of 1 … 8193
elements (tails, one chunk, a chunk boundary, several chunks)."""
import itertools
import math

import pytest
import torch

from optim_cases import NUMELS, flat_case
from test_step_guard import INF, NAN, _bits, _check_stats, _stats_reference, poisoned_mlm, run_mlm

pytestmark = pytest.mark.gpu

DEV = "cuda"
GSCALE, CLIP = 0.5, 5.0  # the clip is active: ‖g‖ · GSCALE ≈ 72
GROUP_OPTS = [(2e-3, 0.01, 1e-8), (5e-4, 0.0, 1e-8)]


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


@pytest.fixture(scope="module")
def case():
    return flat_case(DEV)


def _hyper(step, groups=False, due=0.0):
    words = [GROUP_OPTS[0][0], float(step), 0.0, 0.9, 0.999, 0.25, due, 2.0]
    if groups:
        for lr, wd, eps in GROUP_OPTS:
            words += [lr, wd, eps, 0.0]
    return torch.tensor(words, dtype=torch.float32, device=DEV)


def _guard(words):
    return torch.tensor(words, dtype=torch.float32, device=DEV)


# ---- step_guard -------------------------------------------------------------------------------
def test_step_guard_kernel_against_the_emulation():
    from perceiver_io_amd.ops import emulation as E

    K = _ext()
    part = torch.rand(512, generator=torch.Generator().manual_seed(0)) * 40.0
    overflow = torch.zeros(512)
    overflow[3] = overflow[300] = 2.5e38  # finite partials, Σ overflows fp32
    seq = [part, part.clone().index_fill_(0, torch.tensor([17]), INF), part.clone().index_fill_(0, torch.tensor([511]), NAN),
           part * 2.0, overflow, part]
    dg, hg = torch.zeros(8, device=DEV), torch.zeros(8)
    for i, pt in enumerate(seq):
        K.step_guard(pt.to(DEV), _hyper(i + 1), dg, GSCALE)
        E.step_guard(pt, _hyper(i + 1).cpu(), hg, GSCALE)
        got, want = dg.cpu(), hg
        print(f"step {i + 1}: kernel {got.tolist()} emulation {want.tolist()}")
        assert got[[0, 1, 2, 3, 6, 7]].tolist() == want[[0, 1, 2, 3, 6, 7]].tolist(), i  # flags, counters: exact
        exact = math.sqrt(float(pt.double().sum())) * GSCALE  # the fp64 sum of the partials
        for w in (4, 5):
            if math.isfinite(want[w].item()):
                assert math.isfinite(got[w].item())
                ref = exact if (w == 4 or want[0].item() == 0.0) else want[w].item()
                # 512 positive fp32 terms at 2⁻²⁴ each bound the sum's error at 3.1e-5
                assert abs(got[w].item() - ref) <= 4e-5 * ref, (i, w, got[w].item(), ref)
            elif math.isnan(want[w].item()):
                assert math.isnan(got[w].item()), (i, w)
            else:
                assert got[w].item() == want[w].item(), (i, w)  # inf as it comes
    assert hg[:4].tolist() == [0.0, 3.0, 0.0, 3.0]


# ---- the update paths with a guard ---------------------------------------------------------------
class _Bufs:
    def __init__(self, K, case, nan_pad, poison=False):
        self.p, self.g, self.m, self.v = (case[k].clone() for k in "pgmv")
        if not nan_pad:
            self.m, self.v = torch.nan_to_num(self.m), torch.nan_to_num(self.v)
        if poison:
            self.g[case["offsets"][6] + 9] = INF
        self.shadow = torch.zeros(self.p.numel(), dtype=torch.bfloat16, device=DEV)
        self.loss, self.ring = torch.tensor(1.25, device=DEV), torch.zeros(4, device=DEV)
        self.part = torch.full((512,), NAN, device=DEV)
        K.sumsq(self.g, self.part)
        self.partials = torch.full((2 * case["chunk_tab"].shape[0],), NAN, device=DEV)
        self.trust = torch.full((len(NUMELS),), 7.0, device=DEV)

    def flat(self, lo=0):
        return [t[lo:] for t in (self.p, self.g, self.m, self.v, self.shadow)]

    def outputs(self):
        return dict(p=self.p, g=self.g, m=self.m, v=self.v, shadow=self.shadow, ring=self.ring, trust=self.trust,
                    partials=self.partials)


KINDS = {"adamw_vec": False, "adamw_scalar": False, "adamw_grouped": True, "lamb": False}  # kind → NaN padding in m, v


def _launch(K, kind, case, b, step, clip, zero_grad, guard):
    kw = dict(zero_grad=zero_grad, loss_src=b.loss, loss_ring=b.ring, norm_part=b.part if clip > 0 else None,
              **({} if guard is None else {"guard": guard}))
    tg = torch.tensor([t % 2 for t in range(len(NUMELS))], dtype=torch.int32, device=DEV)
    lr, wd, eps = GROUP_OPTS[0]
    if kind.startswith("adamw_") and kind != "adamw_grouped":  # [1:]: off the 16-byte alignment → the scalar kernel
        K.adamw(*b.flat(1 if kind == "adamw_scalar" else 0), _hyper(step), eps, wd, clip, GSCALE, **kw)
    elif kind == "adamw_grouped":
        K.adamw_grouped(*b.flat(), _hyper(step, True), case["chunk_tab"], tg, 2, clip, GSCALE, **kw)
    else:
        K.lamb(*b.flat(), _hyper(step, True), case["chunk_tab"], case["tensor_tab"], case["tensor_opt"], b.partials,
               b.trust, 1e-6, clip, GSCALE, tensor_group=tg, **kw)


def _same(a, b, what):
    for k, t in a.outputs().items():
        assert torch.equal(_bits(t), _bits(b.outputs()[k])), (what, k)


@pytest.mark.parametrize("clip,zero_grad", list(itertools.product((0.0, CLIP), (False, True))))
@pytest.mark.parametrize("kind", list(KINDS))
def test_guarded_update_kernels(case, kind, clip, zero_grad):
    K = _ext()
    ref, on, late = (_Bufs(K, case, KINDS[kind]) for _ in range(3))
    _launch(K, kind, case, ref, 3, clip, zero_grad, None)
    _launch(K, kind, case, on, 3, clip, zero_grad, _guard([0.0, 0.0, 0.0, 3.0, 1.0, 1.0, 0.0, 0.0]))
    _same(ref, on, "skip 0, total 0 is the launch without a guard")
    _launch(K, kind, case, late, 5, clip, zero_grad, _guard([0.0, 2.0, 0.0, 3.0, 1.0, 1.0, 4.0, 0.0]))
    _same(ref, late, "two skipped steps behind it, hyper[1] = 5 is the unguarded step 3")
    sk = _Bufs(K, case, KINDS[kind], poison=True)
    before = {k: t.clone() for k, t in sk.outputs().items()}
    _launch(K, kind, case, sk, 3, clip, zero_grad, _guard([1.0, 1.0, 1.0, 3.0, INF, 1.0, 3.0, 0.0]))
    torch.cuda.synchronize()
    for k in ("p", "m", "v", "shadow", "trust", "partials"):
        assert torch.equal(_bits(before[k]), _bits(sk.outputs()[k])), k
    assert sk.ring.tolist() == [0.0, 0.0, 1.25, 0.0]
    lo = 1 if kind == "adamw_scalar" else 0
    if zero_grad:
        assert not sk.g[lo:][case["valid"][lo:]].any()
        assert torch.equal(_bits(before["g"][:lo]), _bits(sk.g[:lo]))  # outside the slice
    else:
        assert torch.equal(_bits(before["g"]), _bits(sk.g))


# ---- the GradScaler invariant inside a captured graph --------------------------------------------
def _optimizer(cls, **kw):
    from perceiver_io_amd.ops import optim

    gen = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen).to(DEV)) for n in NUMELS[3:]]
    return getattr(optim, cls)(params, lr=1e-2, weight_decay=0.01, **kw)


def _captured_run(opt, grads, poison_at):
    """Capture ``device_update`` once, replay it once per gradient (the one at ``poison_at`` with an inf)."""
    graph = torch.cuda.CUDAGraph()
    opt.stage_hyper()
    with torch.cuda.graph(graph):
        opt.device_update(zero_grad=True)
    for i, g in enumerate(grads):
        opt.flat.grad.copy_(g)
        if i == poison_at:
            opt.flat.grad[opt.flat.offsets[2] + 7] = INF
        opt.stage_hyper()
        graph.replay()
        opt._step += 1
    torch.cuda.synchronize()


@pytest.mark.parametrize("cls", ["FusedAdamW", "FusedLamb"])
def test_poisoned_replay_equals_the_run_without_it(cls):
    for kw in ({}, {"skip_nonfinite": True}):  # the kernels' modules load outside any capture
        warm = _optimizer(cls, **kw)
        warm.step()
    torch.cuda.synchronize()
    clean, guarded = _optimizer(cls), _optimizer(cls, skip_nonfinite=True)
    gen = torch.Generator().manual_seed(5)
    valid = torch.zeros(clean.flat.numel, dtype=torch.bool)
    for o, p in zip(clean.flat.offsets, clean.flat.params):
        valid[o:o + p.numel()] = True
    grads = [torch.where(valid, torch.randn(clean.flat.numel, generator=gen), torch.zeros(())).to(DEV) for _ in range(5)]
    _captured_run(clean, [g for i, g in enumerate(grads) if i != 2], None)
    _captured_run(guarded, grads, 2)
    assert torch.equal(clean.flat.data, guarded.flat.data)
    assert torch.equal(clean.exp_avg, guarded.exp_avg) and torch.equal(clean.exp_avg_sq, guarded.exp_avg_sq)
    assert torch.equal(_bits(clean.flat.shadow), _bits(guarded.flat.shadow))
    assert not guarded.flat.grad.any()  # cleared on the skipped replay too
    h = guarded.health()
    assert h["skipped"] == 1 and h["consecutive"] == 0 and h["last_skipped_step"] == 3 and math.isfinite(h["last_norm"])
    assert guarded.state_dict()["state"][0]["step"].item() == 4


# ---- tensor_stats ------------------------------------------------------------------------------
def test_tensor_stats_kernels_against_fp64(case):
    K = _ext()
    g, w = case["g"].clone(), case["p"].clone()
    g[case["offsets"][2] + 1] = NAN
    g[case["offsets"][9] + 5000] = INF
    g[case["offsets"][7] + 4095] = -77.0  # the largest magnitude sits in a chunk's last element
    T, C = len(NUMELS), case["chunk_tab"].shape[0]
    part = torch.zeros(4 * C, device=DEV)
    stats, again = torch.full((T, 4), -1.0, device=DEV), torch.full((T, 4), -1.0, device=DEV)
    skip_stats = torch.full((T, 4), -2.0, device=DEV)
    args = (case["chunk_tab"], case["tensor_tab"], part)
    K.tensor_stats(g, w, _hyper(3), *args, stats, GSCALE)
    assert (stats == -1.0).all()  # not due: untouched
    K.tensor_stats(g, w, _hyper(3, due=1.0), *args, stats, GSCALE)
    K.tensor_stats(g, w, _hyper(3, due=1.0), *args, again, GSCALE)
    want = _stats_reference(case, g.cpu(), w.cpu(), GSCALE)
    print("kernel", stats.cpu().tolist(), "fp64", want.tolist())
    _check_stats(stats, want)
    assert torch.equal(_bits(stats), _bits(again))  # bitwise repeatable
    assert want[:, 3].tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0, 1] and want[7, 2].item() == 77.0 * GSCALE
    stats.fill_(-1.0)
    K.tensor_stats(g, w, _hyper(3), *args, stats, GSCALE, guard=_guard([0.0, 0.0, 0.0, 3.0, 1.0, 1.0, 0.0, 0.0]),
                   skip_stats=skip_stats)
    assert (stats == -1.0).all() and (skip_stats == -2.0).all()  # neither due nor skipped
    K.tensor_stats(g, w, _hyper(3), *args, stats, GSCALE, guard=_guard([1.0, 1.0, 1.0, 3.0, NAN, 1.0, 3.0, 0.0]),
                   skip_stats=skip_stats)
    assert (stats == -1.0).all()  # a skipped step fills the second buffer and leaves the first
    _check_stats(skip_stats, want)


def test_tensor_stats_skips_a_chunk_entry_that_does_not_fit(case):
    """An entry that fails the chunk validation is not read (its tensor's row then covers the other
    chunks only); the checked build flags kErrOptTable (64)."""
    K = _ext()
    g, w = case["g"].clone(), case["p"].clone()
    tab = case["chunk_tab"].clone()
    last = tab.shape[0] - 1  # tensor 9's last chunk (1 element): a length past the buffer's end
    tab[last, 1] = 4096
    T = len(NUMELS)
    part, stats = torch.zeros(4 * tab.shape[0], device=DEV), torch.zeros(T, 4, device=DEV)
    K.check_errors(True)
    K.tensor_stats(g, w, _hyper(3, due=1.0), tab, case["tensor_tab"], part, stats, 1.0)
    torch.cuda.synchronize()
    o = case["offsets"][9]
    assert stats[9, 0].item() == pytest.approx(float(g[o:o + 8192].double().norm()), rel=1e-5)
    assert K.check_errors(True) == (64 if K.checked_build() else 0)


# ---- the Trainer on the graph path ---------------------------------------------------------------
@pytest.mark.timeout(180)
def test_trainer_skips_a_poisoned_step_on_the_graph_path(tmp_path):
    from perceiver_io_amd import ops

    cli = run_mlm(tmp_path, poisoned_mlm((5,)), "--data.synthetic_size=80", "--data.max_seq_len=64", "--data.pad_to_max=true", "--model.num_latents=32",
                  "--trainer.accelerator=gpu", "--trainer.devices=1", "--trainer.max_steps=8", "--trainer.log_every_n_steps=2",
                  "--trainer.val_check_interval=6", "--trainer.skip_nonfinite_steps=true", "--trainer.track_grad_norm=2")
    tr = cli.trainer
    opt = tr.optimizers[0]
    assert tr.fused and tr._engine.graph_enabled and tr._engine.replays >= 5 and type(opt).__name__ == "FusedAdamW"
    assert tr.global_step == 8 and tr.callback_metrics["skipped_steps"] == 1
    assert opt.health()["skipped"] == 1 and opt.health()["last_skipped_step"] == 5
    assert torch.isfinite(opt.flat.data).all() and torch.isfinite(opt.flat.shadow.float()).all()
    assert torch.isfinite(opt.exp_avg).all() and torch.isfinite(opt.exp_avg_sq).all()
    assert tr.skip_report.startswith("step 5:") and "tensors with non-finite gradients: " in tr.skip_report
    assert math.isfinite(tr.callback_metrics["grad_2.0_norm_total"])
    assert opt.state_dict()["state"][0]["step"].item() == 7
    ops.check_device_errors()
