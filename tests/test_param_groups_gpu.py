"""Parameter groups on the GPU: the ``adamw_grouped`` kernel (csrc/optim.hip) against its
emulation and, bit for bit, against the single-group ``adamw`` launch; ``lamb`` with a tensor → group
table; a captured step that reads the group words on the device; the checked build."""
import os
import subprocess
import sys

import pytest
import torch

from optim_cases import NUMELS, close
from optim_cases import flat_case as _case

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (lr, weight decay, eps) per group; tensor t sits in group t % G
GROUP_OPTS = [(2e-3, 0.01, 1e-8), (5e-4, 0.0, 1e-8), (1e-3, 0.1, 1e-6), (3e-3, 0.05, 1e-7)]
GSCALE = 0.5
CLIP = 5.0  # active: ‖g‖ · GSCALE ≈ sqrt(20686) / 2 ≈ 72


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


@pytest.fixture(scope="module")
def case():
    return _case()


def _hyper(opts):
    words = [opts[0][0], 3.0, 0.0, 0.9, 0.999, 0.0, 0.0, 2.0]
    for lr, wd, eps in opts:
        words += [lr, wd, eps, 0.0]
    return torch.tensor(words, dtype=torch.float32, device=DEV)


def _tensor_group(G):
    return torch.tensor([t % G for t in range(len(NUMELS))], dtype=torch.int32, device=DEV)


def _buffers(case, shadow):
    p, g, m, v = (case[k].clone() for k in ("p", "g", "m", "v"))
    sh = torch.zeros(p.numel(), dtype=torch.bfloat16, device=DEV) if shadow else None
    return p, g, m, v, sh


def _norm_part(K, g, clip):
    if clip <= 0:
        return None
    part = torch.full((512,), float("nan"), device=DEV)
    K.sumsq(g, part)
    return part


def _run_grouped(K, case, opts, clip=CLIP, zero_grad=True, shadow=True, l2=False):
    p, g, m, v, sh = _buffers(case, shadow)
    loss, ring = torch.tensor(1.25, device=DEV), torch.zeros(4, device=DEV)
    K.adamw_grouped(p, g, m, v, sh, _hyper(opts), case["chunk_tab"], _tensor_group(len(opts)), len(opts), clip, GSCALE,
                    l2=l2, zero_grad=zero_grad, loss_src=loss, loss_ring=ring, norm_part=_norm_part(K, g, clip))
    torch.cuda.synchronize()
    return dict(p=p, g=g, m=m, v=v, shadow=sh, ring=ring)


def _run_single(K, case, lr, wd, eps, clip=CLIP, zero_grad=True, shadow=True, l2=False):
    p, g, m, v, sh = _buffers(case, shadow)
    K.adamw(p, g, m, v, sh, _hyper([(lr, wd, eps)])[:8].contiguous(), eps, wd, clip, GSCALE, l2=l2, zero_grad=zero_grad,
            norm_part=_norm_part(K, g, clip))
    torch.cuda.synchronize()
    return dict(p=p, g=g, m=m, v=v, shadow=sh)


def _bits(t):
    return t.view(torch.uint8) if t.dtype != torch.bfloat16 else t.view(torch.int16)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("clip", [0.0, CLIP])
@pytest.mark.parametrize("zero_grad", [False, True])
@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("l2", [False, True])
def test_adamw_grouped_matches_emulation(case, G, clip, zero_grad, shadow, l2):
    from perceiver_io_amd.ops import emulation

    opts = GROUP_OPTS[:G]
    k = _run_grouped(_ext(), case, opts, clip, zero_grad, shadow, l2)
    e = _run_grouped(emulation, case, opts, clip, zero_grad, shadow, l2)
    valid, pad = case["valid"], ~case["valid"]
    for name in ("p", "m", "v"):
        close(k[name][valid], e[name][valid], 1e-5, name)
    if shadow:
        assert torch.equal(k["shadow"][valid], k["p"][valid].to(torch.bfloat16))  # the bf16 of THIS update
        assert not k["shadow"][pad].view(torch.int16).any()
    if zero_grad:
        assert not k["g"].any()
    else:
        assert torch.equal(k["g"], case["g"])
    assert k["ring"].tolist() == [0.0, 0.0, 1.25, 0.0]  # hyper[7] = 2
    for name in ("p", "m", "v"):  # the padding (NaN in m and v) is bitwise untouched
        assert torch.equal(_bits(k[name][pad]), _bits(case[name][pad])), name
    assert not torch.equal(k["p"][valid], case["p"][valid])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("l2", [False, True])
def test_equal_groups_are_bitwise_the_single_group_launch(case, l2):
    lr, wd, eps = GROUP_OPTS[0]
    valid = case["valid"]
    for shadow in (True, False):
        one = _run_single(_ext(), case, lr, wd, eps, shadow=shadow, l2=l2)
        for G in (2, 4):
            k = _run_grouped(_ext(), case, [(lr, wd, eps)] * G, shadow=shadow, l2=l2)
            for name in ("p", "m", "v", "g") + (("shadow",) if shadow else ()):
                assert torch.equal(_bits(k[name][valid]), _bits(one[name][valid])), (name, G, shadow)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("clip", [0.0, CLIP])
@pytest.mark.parametrize("l2", [False, True])
def test_groups_are_bitwise_separate_single_group_launches(case, G, clip, l2):
    opts = GROUP_OPTS[:G]
    k = _run_grouped(_ext(), case, opts, clip=clip, l2=l2)
    singles = [_run_single(_ext(), case, lr, wd, eps, clip=clip, l2=l2) for lr, wd, eps in opts]
    for t, (o, n) in enumerate(zip(case["offsets"], NUMELS)):
        for name in ("p", "m", "v", "shadow"):
            assert torch.equal(_bits(k[name][o:o + n]), _bits(singles[t % G][name][o:o + n])), (name, t)
    # distinct options did give distinct results
    assert not torch.equal(singles[0]["p"][case["valid"]], singles[1]["p"][case["valid"]])


@pytest.mark.timeout(120)
def test_adamw_grouped_is_bitwise_repeatable(case):
    a, b = _run_grouped(_ext(), case, GROUP_OPTS), _run_grouped(_ext(), case, GROUP_OPTS)
    for name in ("p", "m", "v", "shadow", "g"):
        assert torch.equal(_bits(a[name]), _bits(b[name])), name


def _run_lamb(K, case, opts, tensor_group):
    p, g, m, v, sh = _buffers(case, True)
    m, v = torch.nan_to_num(m), torch.nan_to_num(v)  # the LAMB test's padding: zero
    chunk_tab, tensor_tab, tensor_opt = case["chunk_tab"], case["tensor_tab"], case["tensor_opt"]
    partials = torch.full((2 * chunk_tab.shape[0],), float("nan"), device=DEV)
    trust = torch.full((tensor_tab.shape[0],), float("nan"), device=DEV)
    K.lamb(p, g, m, v, sh, _hyper(opts), chunk_tab, tensor_tab, tensor_opt, partials, trust, 1e-6, CLIP, GSCALE,
           zero_grad=True, norm_part=_norm_part(K, g, CLIP), tensor_group=tensor_group)
    torch.cuda.synchronize()
    return dict(p=p, m=m, v=v, shadow=sh, trust=trust)


@pytest.mark.timeout(120)
def test_lamb_with_tensor_groups_matches_emulation(case):
    from perceiver_io_amd.ops import emulation

    opts = GROUP_OPTS[:2]
    k, e = _run_lamb(_ext(), case, opts, _tensor_group(2)), _run_lamb(emulation, case, opts, _tensor_group(2))
    for name in ("p", "m", "v", "trust"):
        close(k[name], e[name], 1e-5, name)
    assert torch.equal(k["shadow"], k["p"].to(torch.bfloat16))
    # without the table every tensor takes hyper[0]: group 0's tensors agree bitwise, group 1's moved differently
    plain = _run_lamb(_ext(), case, opts, None)
    for t, (o, n) in enumerate(zip(case["offsets"], NUMELS)):
        assert torch.equal(k["p"][o:o + n], plain["p"][o:o + n]) == (t % 2 == 0), t
    all0 = _run_lamb(_ext(), case, opts, torch.zeros(len(NUMELS), dtype=torch.int32, device=DEV))
    assert torch.equal(all0["p"], plain["p"]) and torch.equal(all0["shadow"], plain["shadow"])


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@pytest.mark.timeout(300)
def test_captured_step_with_groups_matches_eager_and_reads_the_group_words_on_the_device():
    """Three replayed steps of a tiny MLM with two groups under OneCycleLR(max_lr=[…]) against the
    same engine without graphs, within the tolerance of tests/test_lamb_gpu.py
    test_captured_lamb_step_matches_eager_and_reads_hyper_on_the_device (losses 5e-3 relative, all
    parameters together 1e-2 relative Frobenius); then a replay with one group's lr forced to 0."""
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops.optim import FusedAdamW, param_groups, scale_group_lrs
    from perceiver_io_amd.tasks import LitMaskedLanguageModel
    from perceiver_io_amd.train.engine import StepEngine

    torch.manual_seed(2)
    ids = torch.randint(3, 200, (4, 64), device=DEV)
    pad = torch.zeros(4, 64, dtype=torch.bool, device=DEV)
    pad[1, 50:] = True
    states = []
    for graph in (False, True):
        torch.manual_seed(3)
        lit = LitMaskedLanguageModel(vocab_size=200, max_seq_len=64,
                                     optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3}},
                                     num_latents=8, num_latent_channels=64, num_encoder_layers=1,
                                     num_encoder_self_attention_layers_per_block=1).to(DEV)
        m = lit.model
        with torch.no_grad():  # one fixed masking: no RNG inside the step
            xm, lab = m.masking(ids, pad, generator=torch.Generator(device=DEV).manual_seed(7))
        groups = scale_group_lrs(param_groups(m, 0.01, no_decay_1d=True), 1e-3)
        assert len(groups) == 2 and groups[1]["weight_decay"] == 0.0 and all(p.dim() <= 1 for p in groups[1]["params"])
        opt = FusedAdamW(groups, max_grad_norm=1.0)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=[2e-3, 4e-3], total_steps=10, cycle_momentum=False)
        eng = StepEngine(lambda b: m.loss(b[1], b[2], labels=lab, x_masked=xm), opt, sched, device=DEV, graph=graph,
                         warmup_eager=0)
        losses = [eng.step((None, ids, pad)).item() for _ in range(3)]
        states.append((losses, opt.flat.data.clone()))
        if graph:
            assert eng.num_graphs == 1 and eng.replays == 3
            assert opt.param_groups[0]["lr"] != opt.param_groups[1]["lr"]
            # the replayed kernel reads every group's words from device memory: group 1 at lr 0
            # stands still bit for bit, group 0 goes on at its scheduled lr
            before, shadow = opt.flat.data.clone(), opt.flat.shadow.clone()
            opt.param_groups[1]["lr"] = 0.0
            eng.step((None, ids, pad))
            assert eng.replays == 4 and opt._step == 4
            torch.cuda.synchronize()
            still = {id(p) for p in opt.param_groups[1]["params"]}
            moved = 0
            for p, o in zip(opt.flat.params, opt.flat.offsets):
                n = p.numel()
                same = torch.equal(opt.flat.data[o:o + n], before[o:o + n])
                if id(p) in still:
                    assert same and torch.equal(opt.flat.shadow[o:o + n], shadow[o:o + n])
                else:
                    moved += int(not same)
            assert len(still) > 0 and moved > 0
    (la, pa), (lb, pb) = states
    assert all(torch.isfinite(torch.tensor(la + lb)))
    for a, b in zip(la, lb):
        assert abs(a - b) <= 5e-3 * abs(a), (la, lb)
    assert _rel(pb, pa) < 1e-2
    ops.check_device_errors()


_CHECKED_PROBE = r"""
import sys
import torch
sys.path.insert(0, "tests")
import test_param_groups_gpu as T
from perceiver_io_amd import ops
from perceiver_io_amd.ops import ext
K = ext.require()
assert K.checked_build() and K.__name__.endswith("_C_check"), K.__name__
case = T._case()
opts = T.GROUP_OPTS[:2]
good = T._run_grouped(K, case, opts)
assert K.check_errors(False) == 0  # group ids inside [0, G) raise nothing
p, g, m, v, sh = T._buffers(case, True)
tg = T._tensor_group(2)
tg[7] = 2  # the 4096-element tensor: a group id == G
K.adamw_grouped(p, g, m, v, sh, T._hyper(opts), case["chunk_tab"], tg, 2, 0.0, T.GSCALE, zero_grad=True)
torch.cuda.synchronize()
assert K.check_errors(False) == 64
good0 = T._run_grouped(K, case, opts, clip=0.0)
for t, (o, n) in enumerate(zip(case["offsets"], T.NUMELS)):
    for name, buf in (("p", p), ("g", g), ("m", m), ("v", v)):
        want = case[name] if t == 7 else good0[name]  # the flagged tensor's chunk is skipped
        assert torch.equal(buf[o:o + n], want[o:o + n]), (name, t)
assert not sh[case["offsets"][7]:case["offsets"][7] + 4096].view(torch.int16).any()
try:
    ops.check_device_errors()
    raise SystemExit("check_device_errors did not raise")
except RuntimeError as e:
    assert "group id" in str(e), e
assert K.check_errors(True) == 0  # cleared
print("CHECKED_OK")
"""


@pytest.mark.timeout(300)
def test_checked_build_flags_a_group_id_outside_the_groups():
    from perceiver_io_amd.csrc.build import ext_path

    assert ext_path("_C_check").exists(), "the checked extension is not built"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PERCEIVER_CHECKED="1", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", _CHECKED_PROBE], env=env, capture_output=True, text=True, timeout=240,
                       cwd=root)
    assert r.returncode == 0 and "CHECKED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("scale", [0.1, 0.0])
def test_trainer_fit_on_the_graph_path_keeps_the_groups(tmp_path, scale):
    """``--model.no_decay_1d --model.encoder_lr_scale`` through ``Trainer.fit`` on the GPU: the fused
    optimizer that replaces AdamW has its four groups, OneCycleLR is re-bound with per-group ``max_lr``,
    the ``pg`` learning rates are logged, and with the scale at 0 the encoder's two groups (lr 0 on
    every replay) stay bitwise unchanged while the decoder trains."""
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops.optim import FusedAdamW
    from perceiver_io_amd.tasks import LitMaskedLanguageModel
    from perceiver_io_amd.train.callbacks import LearningRateMonitor
    from perceiver_io_amd.train.trainer import Trainer

    torch.manual_seed(0)
    lit = LitMaskedLanguageModel(
        vocab_size=1000, max_seq_len=128, num_latents=64, num_latent_channels=64, num_encoder_layers=2,
        num_encoder_self_attention_layers_per_block=2, no_decay_1d=True, encoder_lr_scale=scale,
        optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3, "weight_decay": 0.01}},
        scheduler_init={"class_path": "torch.optim.lr_scheduler.OneCycleLR",
                        "init_args": {"max_lr": 2e-3, "total_steps": 10, "cycle_momentum": False}})
    before = {n: p.detach().clone() for n, p in lit.model.named_parameters()}
    g = torch.Generator().manual_seed(5)
    data = [(torch.zeros(4, dtype=torch.long), torch.randint(3, 1000, (4, 128), generator=g),
             torch.zeros(4, 128, dtype=torch.bool)) for _ in range(4)]
    tr = Trainer(logger=False, enable_checkpointing=False, callbacks=[LearningRateMonitor(logging_interval="step")],
                 default_root_dir=str(tmp_path), accelerator="gpu", devices=1, max_steps=4, num_sanity_val_steps=0,
                 limit_val_batches=0, enable_progress_bar=False, log_every_n_steps=1)
    seen = {}
    tr.log_scalars = seen.update
    tr.fit(lit, train_dataloaders=data)
    torch.cuda.synchronize()
    assert tr.fused and tr.global_step == 4 and tr._engine.graph_enabled and tr._engine.replays > 0
    opt = tr.optimizers[0]
    assert type(opt) is FusedAdamW and len(opt.param_groups) == 4 and opt.hyper.numel() == 8 + 4 * 4
    assert sorted((g["lr_scale"], g["weight_decay"]) for g in opt.param_groups) == [
        (scale, 0.0), (scale, 0.01), (1.0, 0.0), (1.0, 0.01)]
    enc = {id(p) for p in lit.model.encoder.parameters()}
    for g in opt.param_groups:
        assert all((id(p) in enc) == (g["lr_scale"] == scale) for p in g["params"])
        assert all((p.dim() <= 1) == (g["weight_decay"] == 0.0) for p in g["params"])
    assert {id(p) for p in opt.flat.params} == {id(p) for p in lit.parameters() if p.requires_grad}
    assert tr.lr_schedulers[0].optimizer is opt
    assert [g["max_lr"] for g in opt.param_groups] == pytest.approx([2e-3 * g["lr_scale"] for g in opt.param_groups])
    assert [g["lr"] for g in opt.param_groups] == pytest.approx(
        [opt.param_groups[2]["lr"] * g["lr_scale"] for g in opt.param_groups])
    assert {f"lr-FusedAdamW/pg{j}" for j in range(1, 5)} <= set(seen)
    assert len(opt.hyper_values()) == 24
    still = moved = 0
    for name, p in lit.model.named_parameters():
        same = torch.equal(p.detach().cpu(), before[name])
        if scale == 0.0 and name.startswith("encoder."):
            assert same, name
            still += 1
        else:
            moved += int(not same)
    assert moved > 0 and (still > 0) == (scale == 0.0)
    if scale != 0.0:  # the encoder trains too
        assert any(not torch.equal(p.detach().cpu(), before[n]) for n, p in lit.model.named_parameters()
                   if n.startswith("encoder."))
    ops.check_device_errors()
