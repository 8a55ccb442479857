"""Fused LAMB on the GPU (csrc/lamb.hip): the kernels against their emulation over one flat
buffer of awkward tensor sizes, bitwise repeatability, the captured step and the command line."""
import os

import pytest
import torch

from optim_cases import close

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


def _case():
    """One flat buffer: sizes around the 64-element alignment and the chunk length, a long
    partial chain, an all-zero-weight tensor and a zero-gradient tensor without decay.
    (numel, weight decay, adapt) per tensor; adapted and non-adapted tensors alternate."""
    from perceiver_io_amd.ops.optim import ALIGN, LAMB_CHUNK, lamb_tables

    CH = LAMB_CHUNK
    spec = [(1, 0.0, False), (63, 0.01, True), (64, 0.0, False), (65, 0.01, True), (CH - 1, 0.01, True),
            (CH, 0.0, False), (CH + 1, 0.01, True), (3 * CH + 5, 0.01, True), (64, 0.01, True),  # [8]: zero weights
            (64, 0.0, True),  # [9]: zero gradient, wd = 0, zero moments
            ((1 << 20) + 192, 0.01, True), (7, 0.02, False)]
    offsets, off = [], 0
    for n, _, _ in spec:
        offsets.append(off)
        off += (n + ALIGN - 1) // ALIGN * ALIGN
    g = torch.Generator().manual_seed(11)
    valid = torch.zeros(off, dtype=torch.bool)
    for o, (n, _, _) in zip(offsets, spec):
        valid[o:o + n] = True
    zero = torch.zeros(off)  # padding is +0.0 bitwise, as FlatParameterSpace leaves it
    p = torch.where(valid, torch.randn(off, generator=g), zero)
    grad = torch.where(valid, torch.randn(off, generator=g), zero)
    m = torch.where(valid, torch.randn(off, generator=g) * 0.1, zero)
    v = torch.where(valid, torch.rand(off, generator=g) * 0.01, zero)
    o8, o9 = offsets[8], offsets[9]
    p[o8:o8 + 64] = 0
    grad[o9:o9 + 64] = 0
    m[o9:o9 + 64] = 0
    v[o9:o9 + 64] = 0
    tabs = lamb_tables(offsets, [s[0] for s in spec], [s[1] for s in spec], [s[2] for s in spec], DEV)
    return dict(spec=spec, offsets=offsets, valid=valid.to(DEV), p=p.to(DEV), g=grad.to(DEV), m=m.to(DEV), v=v.to(DEV),
                tabs=tabs)


@pytest.fixture(scope="module")
def case():
    return _case()


def _run(K, case, clip, zero_grad, shadow):
    p, g, m, v = (case[k].clone() for k in ("p", "g", "m", "v"))
    sh = torch.zeros(p.numel(), dtype=torch.bfloat16, device=DEV) if shadow else None
    chunk_tab, tensor_tab, tensor_opt = case["tabs"]
    partials = torch.full((2 * chunk_tab.shape[0],), float("nan"), device=DEV)
    trust = torch.full((tensor_tab.shape[0],), float("nan"), device=DEV)
    hyper = torch.tensor([2e-3, 3.0, 0.0, 0.9, 0.999, 0, 0, 2.0], device=DEV)
    part = torch.full((512,), float("nan"), device=DEV)
    loss, ring = torch.tensor(1.25, device=DEV), torch.zeros(4, device=DEV)
    if clip > 0:
        K.sumsq(g, part)
    K.lamb(p, g, m, v, sh, hyper, chunk_tab, tensor_tab, tensor_opt, partials, trust, 1e-6, clip, 0.5,
           zero_grad=zero_grad, loss_src=loss, loss_ring=ring, norm_part=part if clip > 0 else None)
    torch.cuda.synchronize()
    return dict(p=p, g=g, m=m, v=v, shadow=sh, trust=trust, ring=ring)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("clip", [0.0, 5.0])
@pytest.mark.parametrize("zero_grad", [False, True])
@pytest.mark.parametrize("shadow", [True, False])
def test_lamb_kernels_match_emulation(case, clip, zero_grad, shadow):
    from perceiver_io_amd.ops import emulation
    from perceiver_io_amd.ops.optim import LAMB_CHUNK

    assert _ext().LAMB_CHUNK == LAMB_CHUNK
    # the clip is active: ‖g‖ · gscale ≈ sqrt(1.07 M) / 2 ≈ 517 > 5
    k, e = _run(_ext(), case, clip, zero_grad, shadow), _run(emulation, case, clip, zero_grad, shadow)
    for name in ("p", "m", "v", "trust") + (("shadow",) if shadow else ()):
        close(k[name], e[name], 1e-5, name)
    if shadow:
        assert torch.equal(k["shadow"], k["p"].to(torch.bfloat16))  # the shadow is the bf16 of THIS update
    if zero_grad:
        assert not k["g"].any()
    else:
        assert torch.equal(k["g"], case["g"])
    assert k["ring"].tolist() == [0.0, 0.0, 1.25, 0.0]  # hyper[7] = 2
    pad = ~case["valid"]
    for name in ("p", "m", "v") + (("shadow",) if shadow else ()):
        assert not k[name][pad].view(torch.uint8).any(), name  # bitwise zero (no -0.0 either)
    spec, offs = case["spec"], case["offsets"]
    tr = k["trust"].tolist()
    assert all(tr[i] == 1.0 for i, s in enumerate(spec) if not s[2])
    assert tr[8] == 1.0 and tr[9] == 1.0  # ‖w‖ = 0; ‖u‖ = 0
    assert k["p"][offs[8]:offs[8] + 64].abs().max() > 0  # moved off zero
    assert torch.equal(k["p"][offs[9]:offs[9] + 64], case["p"][offs[9]:offs[9] + 64])  # bitwise unchanged
    assert all(t != 1.0 for i, t in enumerate(tr) if spec[i][2] and i not in (8, 9))


@pytest.mark.timeout(120)
def test_lamb_kernels_are_bitwise_repeatable(case):
    a, b = _run(_ext(), case, 5.0, True, True), _run(_ext(), case, 5.0, True, True)
    for name in ("p", "m", "v", "trust", "shadow"):
        assert torch.equal(a[name], b[name]), name


def _smoke_mlm():
    from perceiver_io_amd.tasks import LitMaskedLanguageModel

    # the model of __graft_entry__.smoke
    return LitMaskedLanguageModel(vocab_size=1000, max_seq_len=128,
                                  optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3}},
                                  num_latents=64, num_latent_channels=64, num_encoder_layers=2,
                                  num_encoder_self_attention_layers_per_block=2).to(DEV)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@pytest.mark.timeout(300)
def test_captured_lamb_step_matches_eager_and_reads_hyper_on_the_device():
    """Three replayed steps against the same engine without graphs, within the tolerance of
    tests/test_model_gpu.py test_graph_engine_matches_eager_steps (losses 5e-3 relative, all
    parameters together 1e-2 relative Frobenius); then a replay with lr forced to 0."""
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops.optim import FusedLamb
    from perceiver_io_amd.train.engine import StepEngine

    torch.manual_seed(2)
    ids = torch.randint(3, 1000, (4, 128), device=DEV)
    pad = torch.zeros(4, 128, dtype=torch.bool, device=DEV)
    pad[1, 100:] = True
    states = []
    for graph in (False, True):
        torch.manual_seed(3)
        lit = _smoke_mlm()
        m = lit.model
        with torch.no_grad():  # one fixed masking: no RNG inside the step
            xm, lab = m.masking(ids, pad, generator=torch.Generator(device=DEV).manual_seed(7))
        opt = FusedLamb(m.parameters(), lr=1e-3, max_grad_norm=1.0)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=2e-3, total_steps=10, cycle_momentum=False)
        eng = StepEngine(lambda b: m.loss(b[1], b[2], labels=lab, x_masked=xm), opt, sched, device=DEV, graph=graph,
                         warmup_eager=0)
        losses = [eng.step((None, ids, pad)).item() for _ in range(3)]
        states.append((losses, opt.flat.data.clone()))
        if graph:
            assert eng.num_graphs == 1 and eng.replays == 3
            tr = opt.last_trust()
            assert torch.isfinite(tr).all() and (tr > 0).all()
            assert all(tr[i].item() == 1.0 for i, p in enumerate(opt.flat.params) if p.dim() <= 1)
            assert any(tr[i].item() != 1.0 for i, p in enumerate(opt.flat.params) if p.dim() > 1)
            # the replayed kernels read lr from device memory: lr = 0 → nothing moves
            before, shadow = opt.flat.data.clone(), opt.flat.shadow.clone()
            opt.param_groups[0]["lr"] = 0.0
            eng.step((None, ids, pad))
            assert eng.replays == 4
            torch.cuda.synchronize()
            assert torch.equal(opt.flat.data, before) and torch.equal(opt.flat.shadow, shadow)
            assert opt._step == 4
    (la, pa), (lb, pb) = states
    assert all(torch.isfinite(torch.tensor(la + lb)))
    for a, b in zip(la, lb):
        assert abs(a - b) <= 5e-3 * abs(a), (la, lb)
    assert _rel(pb, pa) < 1e-2
    ops.check_device_errors()


@pytest.mark.timeout(300)
def test_mlm_cli_fit_with_lamb_on_the_graph_path(tmp_path):
    from perceiver_io_amd.cli.tasks import main

    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        cli = main("mlm", ["fit", "--data=IMDBDataModule", "--data.synthetic=true", "--data.synthetic_size=64",
                           "--data.vocab_size=500", "--data.max_seq_len=64", "--data.batch_size=8",
                           "--data.num_workers=0", "--data.pad_to_max=true", "--model.num_latents=32",
                           "--model.num_encoder_layers=2", "--model.num_encoder_self_attention_layers_per_block=2",
                           "--optimizer=Lamb", "--optimizer.lr=3e-3", "--trainer.accelerator=gpu",
                           "--trainer.devices=1", "--trainer.max_steps=6", "--trainer.val_check_interval=6",
                           "--trainer.limit_val_batches=2", "--trainer.log_every_n_steps=1",
                           "--model.masked_samples=null"])
    finally:
        os.chdir(old)
    tr = cli.trainer
    assert tr.fused and tr._engine.graph_enabled and tr._engine.num_graphs == 1 and tr._engine.replays > 0
    assert tr.global_step == 6
    assert type(tr.optimizers[0]).__name__ == "FusedLamb"
    assert tr.lr_schedulers[0].optimizer is tr.optimizers[0]
    assert torch.isfinite(torch.tensor(tr.callback_metrics["train_loss"]))
    assert cli.model.hparams["optimizer_init"]["class_path"] == "perceiver_io_amd.ops.optim.Lamb"
