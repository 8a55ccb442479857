"""Parameter groups in the fused optimizers on the CPU: ``FusedAdamW`` / ``FusedAdam`` /
``FusedLamb`` with per-group lr and weight decay (the emulation of ``adamw_grouped`` and of
``lamb(tensor_group=)``, the HIP kernels' oracles) against ``torch.optim.AdamW`` / ``Adam`` and
``ops.optim.Lamb`` built with the same groups, the chunk tables and the padding, torch-layout state
dicts, the ``param_groups`` helper, and the two ``LitModel`` options through the trainer."""
import pytest
import torch

from perceiver_io_amd.ops import emulation
from perceiver_io_amd.ops.optim import (ALIGN, LAMB_CHUNK, FlatParameterSpace, FusedAdam, FusedAdamW, FusedLamb, Lamb,
                                        group_tables, lamb_tables, param_groups, scale_scheduler_init)

NUMELS = [1, 3, 5, 63, 64, 65, 4095, 4096, 4097, 8193]
# tensor → group: every group holds small and multi-chunk tensors, and no group is contiguous
GROUP3 = [0, 1, 2, 0, 1, 2, 0, 1, 2, 1]
GROUP2 = [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
OPTS3 = [dict(lr=1e-3, weight_decay=0.01, eps=1e-8), dict(lr=3e-3, weight_decay=0.0, eps=1e-8),
         dict(lr=1e-4, weight_decay=0.1, eps=1e-6)]
MAX_LR3 = [3e-2, 1e-2, 3e-3]
TOL = dict(atol=1e-6, rtol=1e-5)  # the project's fused-optimizer tolerance (tests/test_lamb.py TOL)
CLIP = 0.5


def _shape(n):  # every other multi-element tensor 2-d, so LAMB's exclude_1d sees both kinds
    return (n,) if n < 64 or n % 2 else (n // 2, 2)


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*_shape(n), generator=g)) for n in NUMELS]


def _grads(step, seed=1):
    # step 0's gradient norm (≈ 5·sqrt(Σ numel) ≈ 780) is clipped at CLIP, the later ones (≈ 0.16) are not
    g = torch.Generator().manual_seed(100 * seed + step)
    return [torch.randn(*_shape(n), generator=g) * (5.0 if step == 0 else 1e-3) for n in NUMELS]


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)


def _groups(params, assign, opts):
    return [{"params": [p for p, a in zip(params, assign) if a == j], **o} for j, o in enumerate(opts)]


def _run(make, assign, opts, max_lr, steps=5, fused=True, seed=0):
    """``steps`` steps under ``OneCycleLR(max_lr=[…])`` with clipping at CLIP; a plain optimizer
    (``fused=False``) clips with ``clip_grad_norm_`` unless it clips itself."""
    params = _params(seed)
    opt = make(_groups(params, assign, opts))
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=max_lr, total_steps=10, cycle_momentum=False)
    for t in range(steps):
        opt.zero_grad()
        _set_grads(params, _grads(t))
        if not fused and not getattr(opt, "max_grad_norm", 0.0):
            torch.nn.utils.clip_grad_norm_(params, CLIP)
        opt.step()
        sched.step()
    return params, opt


def _assert_params_close(got, want):
    for a, b in zip(got, want):
        torch.testing.assert_close(a.detach(), b.detach(), **TOL)


def test_fused_adamw_groups_match_torch_adamw():
    fused, opt = _run(lambda gs: FusedAdamW(gs, max_grad_norm=CLIP), GROUP3, OPTS3, MAX_LR3)
    ref, ropt = _run(lambda gs: torch.optim.AdamW(gs), GROUP3, OPTS3, MAX_LR3, fused=False)
    assert len(opt.param_groups) == 3 and opt.hyper.numel() == 8 + 4 * 3 and len(opt.hyper_values()) == 20
    assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in ropt.param_groups]
    assert len({g["lr"] for g in opt.param_groups}) == 3
    _assert_params_close(fused, ref)
    # the group words of the NEXT update: behind the 8 global ones, hyper[0] still group 0's lr
    hv = opt.hyper_values()
    assert hv[0] == opt.param_groups[0]["lr"] and hv[1] == 6.0 and hv[5] == 0.0
    for j, g in enumerate(opt.param_groups):
        assert hv[8 + 4 * j:12 + 4 * j] == [g["lr"], g["weight_decay"], g["eps"], 0.0]
    assert opt.bucket_updates_ok() is False
    with pytest.raises(NotImplementedError):
        opt.range_update(0, 64)


def test_fused_adam_groups_match_torch_adam():
    fused, opt = _run(lambda gs: FusedAdam(gs, max_grad_norm=CLIP), GROUP3, OPTS3, MAX_LR3)
    ref, _ = _run(lambda gs: torch.optim.Adam(gs), GROUP3, OPTS3, MAX_LR3, fused=False)
    assert opt.l2 and len(opt.param_groups) == 3
    _assert_params_close(fused, ref)


def test_fused_lamb_groups_match_lamb():
    opts = [dict(lr=1e-3, weight_decay=0.01, exclude_1d=True), dict(lr=3e-3, weight_decay=0.1, exclude_1d=False)]
    fused, opt = _run(lambda gs: FusedLamb(gs, max_grad_norm=CLIP), GROUP2, opts, [3e-2, 1e-2])
    ref, _ = _run(lambda gs: Lamb(gs, max_grad_norm=CLIP), GROUP2, opts, [3e-2, 1e-2], fused=False)
    assert opt.tensor_opt.shape == (len(NUMELS), 2) and opt.tensor_group.tolist() == [
        GROUP2[NUMELS.index(p.numel())] for p in opt.flat.params]
    # group 0 leaves its 1-d tensors plain, group 1 decays and adapts them
    for p, (wd, adapt), j in zip(opt.flat.params, opt.tensor_opt.tolist(), opt.tensor_group.tolist()):
        plain = j == 0 and p.dim() <= 1
        assert wd == pytest.approx(0.0 if plain else opts[j]["weight_decay"]) and adapt == (0.0 if plain else 1.0)
    _assert_params_close(fused, ref)


@pytest.mark.parametrize("cls", [FusedAdamW, FusedAdam, FusedLamb])
def test_groups_with_equal_options_are_bitwise_one_group(cls):
    same = dict(lr=1e-3, weight_decay=0.01)
    grouped, gopt = _run(lambda gs: cls(gs, max_grad_norm=CLIP), GROUP3, [same] * 3, 3e-2, steps=3)
    params = _params()
    one = cls(params, max_grad_norm=CLIP, **same)
    sched = torch.optim.lr_scheduler.OneCycleLR(one, max_lr=3e-2, total_steps=10, cycle_momentum=False)
    for t in range(3):
        one.zero_grad()
        _set_grads(params, _grads(t))
        one.step()
        sched.step()
    assert len(gopt.param_groups) == 3 and len(one.param_groups) == 1 and one.hyper.numel() == 8
    assert len(one.hyper_values()) == 8
    for a, b in zip(grouped, params):
        assert torch.equal(a.detach(), b.detach())
    # the moments too, tensor by tensor (the grouped flat buffer is laid out in group order)
    at = {id(p): i for i, p in enumerate(gopt.flat.params)}
    for buf_g, buf_1 in ((gopt.exp_avg, one.exp_avg), (gopt.exp_avg_sq, one.exp_avg_sq)):
        vg, v1 = gopt.flat.views(buf_g), one.flat.views(buf_1)
        for k, (a, b) in enumerate(zip(grouped, params)):
            assert one.flat.params[k] is b and torch.equal(vg[at[id(a)]], v1[k])


def _padding_mask(flat):
    pad = torch.ones(flat.numel, dtype=torch.bool)
    for p, o in zip(flat.params, flat.offsets):
        pad[o:o + p.numel()] = False
    return pad


def test_padding_stays_bitwise_zero_and_tables_cover_tensors_exactly():
    params, opt = _run(lambda gs: FusedAdamW(gs, max_grad_norm=CLIP), GROUP3, OPTS3, MAX_LR3, steps=3)
    flat = opt.flat
    pad = _padding_mask(flat)
    assert pad.sum() > 0 and flat.shadow is not None
    for buf in (flat.data, opt.exp_avg, opt.exp_avg_sq, flat.shadow):
        assert torch.equal(buf[pad].view(torch.uint8), torch.zeros_like(buf[pad]).view(torch.uint8))
    chunks, tgroup = group_tables(flat, opt.param_groups)
    assert torch.equal(chunks, opt.chunk_tab) and torch.equal(tgroup, opt.tensor_group)
    assert chunks.dtype == torch.int64 and tgroup.dtype == torch.int32 and tgroup.shape == (len(NUMELS),)
    # the same cutting as the LAMB tables
    numels = [p.numel() for p in flat.params]
    assert torch.equal(chunks, lamb_tables(flat.offsets, numels, [0.0] * len(numels), [True] * len(numels), "cpu")[0])
    covered = torch.zeros(flat.numel, dtype=torch.int32)
    for start, length, t in chunks.tolist():
        assert 0 < length <= LAMB_CHUNK and start % 4 == 0
        assert flat.offsets[t] <= start and start + length <= flat.offsets[t] + numels[t]
        covered[start:start + length] += 1
    assert torch.equal(covered == 1, ~pad) and int(covered.max()) == 1
    assert all(o % ALIGN == 0 for o in flat.offsets)
    for p, j in zip(flat.params, tgroup.tolist()):
        assert any(p is q for q in opt.param_groups[j]["params"])


def test_group_order_differs_from_flat_order_and_state_dict_round_trips():
    params = _params()
    for i in (4, 7):  # replicated parameters go first in the flat buffer
        params[i]._pio_replicate = True
    opt = FusedAdamW(_groups(params, GROUP3, OPTS3), max_grad_norm=CLIP,
                     flat=FlatParameterSpace(params, with_shadow=True, replicate=True))
    ordered = [p for g in opt.param_groups for p in g["params"]]
    assert [id(p) for p in opt.flat.params] != [id(p) for p in ordered]
    assert opt.flat.params[0] is params[4] and opt.flat.params[1] is params[7]
    tparams = _params()
    topt = torch.optim.AdamW(_groups(tparams, GROUP3, OPTS3))
    for t in range(2):
        grads = _grads(t)
        opt.zero_grad()
        _set_grads(params, grads)
        opt.step()
        _set_grads(tparams, grads)
        torch.nn.utils.clip_grad_norm_(tparams, CLIP)
        topt.step()
    _assert_params_close(params, tparams)
    # fused → torch.optim.AdamW with the same groups: state keys number the parameters in group order
    sd = opt.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1, 2], [3, 4, 5, 6], [7, 8, 9]]
    assert sorted(sd["state"]) == list(range(len(NUMELS)))
    for k, p in enumerate(ordered):
        assert sd["state"][k]["exp_avg"].shape == p.shape
    mid_params = _params()
    with torch.no_grad():
        for a, b in zip(mid_params, params):
            a.copy_(b)
    mid = torch.optim.AdamW(_groups(mid_params, GROUP3, [dict(lr=1.0)] * 3))
    mid.load_state_dict(sd)
    assert [g["lr"] for g in mid.param_groups] == [o["lr"] for o in OPTS3]
    for p, q in zip(params, mid_params):  # the same tensor's moments, whatever the buffer order
        i = [id(x) for x in opt.flat.params].index(id(p))
        torch.testing.assert_close(mid.state[q]["exp_avg"], opt.flat.views(opt.exp_avg)[i], rtol=0, atol=0)
    # … and back into a fresh fused optimizer
    back_params = _params()
    with torch.no_grad():
        for a, b in zip(back_params, params):
            a.copy_(b)
    back = FusedAdamW(_groups(back_params, GROUP3, [dict(lr=1.0)] * 3), max_grad_norm=CLIP)
    back.load_state_dict(mid.state_dict())
    assert back._step == 2 and [g["weight_decay"] for g in back.param_groups] == [o["weight_decay"] for o in OPTS3]
    grads = _grads(2)
    for o, ps in ((opt, params), (back, back_params), (mid, mid_params)):
        o.zero_grad()
        _set_grads(ps, grads)
        if o is mid:
            torch.nn.utils.clip_grad_norm_(ps, CLIP)
        o.step()
    _assert_params_close(back_params, params)
    _assert_params_close(back_params, mid_params)


def test_single_group_state_dict_layout_is_unchanged():
    params = _params()
    opt = FusedAdamW(params, lr=1e-3)
    _set_grads(params, _grads(1))
    opt.step()
    sd = opt.state_dict()
    assert sd["param_groups"][0]["params"] == list(range(len(NUMELS))) and sorted(sd["state"]) == list(range(len(NUMELS)))
    for i, p in enumerate(opt.flat.params):
        assert sd["state"][i]["exp_avg"].shape == p.shape
    fresh = FusedAdamW(_params(), lr=1.0)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.exp_avg, opt.exp_avg) and fresh._step == 1 and fresh.param_groups[0]["lr"] == 1e-3


def test_error_cases():
    params = _params()
    with pytest.raises(ValueError, match="at most 8 parameter groups"):
        FusedAdamW([{"params": [p]} for p in params[:9]])
    with pytest.raises(ValueError, match="betas"):
        FusedAdamW([{"params": params[:2]}, {"params": params[2:], "betas": (0.8, 0.999)}])
    with pytest.raises(ValueError, match="betas"):
        FusedLamb([{"params": params[:2]}, {"params": params[2:], "betas": (0.9, 0.99)}])
    eight = FusedAdamW([{"params": [p], "lr": 1e-3 * (j + 1)} for j, p in enumerate(params[:8])])
    assert eight.hyper.numel() == 40 and len(eight.hyper_values()) == 40
    # the emulation refuses a group id outside [0, G), as the checked kernel flags it
    opt = FusedAdamW(_groups(params[8:], [0, 1], OPTS3[:2]))
    opt.stage_hyper()
    bad = opt.tensor_group.clone()
    bad[1] = 2
    with pytest.raises(ValueError):
        emulation.adamw_grouped(opt.flat.data, opt.flat.grad, opt.exp_avg, opt.exp_avg_sq, None, opt.hyper,
                                opt.chunk_tab, bad, 2, 0.0, 1.0)


# ---- the helper and the LitModel options -------------------------------------------------------------
def _lit(**kw):
    from perceiver_io_amd.tasks import LitImageClassifier

    torch.manual_seed(0)
    kw.setdefault("optimizer_init", {"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-2, "weight_decay": 0.05}})
    return LitImageClassifier(image_shape=(8, 8, 1), num_classes=4, num_frequency_bands=4, num_latents=8,
                              num_latent_channels=16, num_encoder_layers=1,
                              num_encoder_self_attention_layers_per_block=1, **kw)


def test_param_groups_helper_counts_and_membership():
    net = _lit().model  # a tiny PerceiverIO: children "0" (encoder) and "1" (decoder)
    named = dict(net.named_parameters())
    assert any(n.startswith("0.") for n in named) and any(n.startswith("1.") for n in named)
    one = param_groups(net, 0.05)
    assert len(one) == 1 and one[0]["weight_decay"] == 0.05 and one[0]["lr_scale"] == 1.0
    assert [id(p) for p in one[0]["params"]] == [id(p) for p in net.parameters()]
    two = param_groups(net, 0.05, no_decay_1d=True)
    assert sorted(g["weight_decay"] for g in two) == [0.0, 0.05]
    four = param_groups(net, 0.05, no_decay_1d=True, lr_scales={"0.": 0.1})
    assert len(four) == 4 and sorted((g["lr_scale"], g["weight_decay"]) for g in four) == [
        (0.1, 0.0), (0.1, 0.05), (1.0, 0.0), (1.0, 0.05)]
    where = {id(p): g for g in four for p in g["params"]}
    assert len(where) == len(named) == sum(len(g["params"]) for g in four)
    for name, p in named.items():
        g = where[id(p)]
        assert g["lr_scale"] == (0.1 if name.startswith("0.") else 1.0)
        assert g["weight_decay"] == (0.0 if p.dim() <= 1 else 0.05)
    # frozen parameters belong to no group; a group they leave empty is dropped
    for name, p in named.items():
        p.requires_grad_(not name.startswith("0."))
    assert sorted(g["lr_scale"] for g in param_groups(net, 0.05, no_decay_1d=True, lr_scales={"0.": 0.1})) == [1.0, 1.0]
    init = {"class_path": "torch.optim.lr_scheduler.OneCycleLR", "init_args": {"max_lr": 1e-2, "total_steps": 10}}
    assert scale_scheduler_init(init, four)["init_args"]["max_lr"] == [1e-2 * g["lr_scale"] for g in four]
    assert scale_scheduler_init(init, one) is init and init["init_args"]["max_lr"] == 1e-2


def test_default_hparams_configure_one_group_as_before():
    lit = _lit()
    assert lit.hparams["no_decay_1d"] is False and lit.hparams["encoder_lr_scale"] == 1.0
    opt = lit.configure_optimizers()
    assert type(opt) is torch.optim.AdamW and len(opt.param_groups) == 1
    ref = torch.optim.AdamW(lit.parameters(), lr=1e-2, weight_decay=0.05)
    assert {k: v for k, v in opt.param_groups[0].items() if k != "params"} == {
        k: v for k, v in ref.param_groups[0].items() if k != "params"}
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in lit.parameters()]
    # a checkpoint from before the two options lacks them
    old = _lit()
    del old.hparams["no_decay_1d"], old.hparams["encoder_lr_scale"]
    assert len(old.configure_optimizers().param_groups) == 1
    sched = _lit(no_decay_1d=True, encoder_lr_scale=0.1,
                 scheduler_init={"class_path": "torch.optim.lr_scheduler.OneCycleLR",
                                 "init_args": {"max_lr": 1e-2, "total_steps": 10}}).configure_optimizers()
    groups = sched["optimizer"].param_groups
    assert len(groups) == 4 and [g["max_lr"] for g in groups] == [1e-2 * g["lr_scale"] for g in groups]
    assert sorted({g["lr_scale"] for g in groups}) == [0.1, 1.0]


def test_trainer_fit_honours_the_groups(tmp_path):
    from perceiver_io_amd.tasks import LitImageClassifier
    from perceiver_io_amd.train.callbacks import LearningRateMonitor
    from perceiver_io_amd.train.trainer import Trainer

    class Lit(LitImageClassifier):
        def configure_optimizers(self):
            opt = super().configure_optimizers()
            for g in opt.param_groups:  # the encoder's undecayed group stands still
                if g["lr_scale"] == 0.1 and g["weight_decay"] == 0.0:
                    g["lr"] = 0.0
            return opt

    torch.manual_seed(0)
    lit = Lit(image_shape=(8, 8, 1), num_classes=4, num_frequency_bands=4, num_latents=8, num_latent_channels=16,
              num_encoder_layers=1, num_encoder_self_attention_layers_per_block=1, no_decay_1d=True,
              encoder_lr_scale=0.1,
              optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-2, "weight_decay": 0.05}})
    before = {n: p.detach().clone() for n, p in lit.model.named_parameters()}
    g = torch.Generator().manual_seed(11)
    data = [(torch.rand(4, 8, 8, 1, generator=g), torch.randint(0, 4, (4,), generator=g)) for _ in range(3)]
    tr = Trainer(logger=False, enable_checkpointing=False, callbacks=[LearningRateMonitor(logging_interval="step")],
                 default_root_dir=str(tmp_path), accelerator="cpu", max_epochs=1, limit_train_batches=3,
                 num_sanity_val_steps=0, enable_progress_bar=False, log_every_n_steps=1)
    seen = {}
    tr.log_scalars = seen.update
    tr.fit(lit, train_dataloaders=data)
    assert tr.global_step == 3
    groups = tr.optimizers[0].param_groups
    assert len(groups) == 4
    where = {id(p): g for g in groups for p in g["params"]}
    still = moved = 0
    for name, p in lit.model.named_parameters():
        g = where[id(p)]
        assert g["weight_decay"] == (0.0 if p.dim() <= 1 else 0.05)  # 1-d tensors are not decayed
        if name.startswith("0.") and p.dim() <= 1:
            assert g["lr"] == 0.0 and torch.equal(p.detach(), before[name]), name
            still += 1
        else:
            assert g["lr"] == pytest.approx(1e-2 * g["lr_scale"])
            moved += int(not torch.equal(p.detach(), before[name]))
    assert still > 0 and moved > 0
    name = type(tr.optimizers[0]).__name__
    assert {f"lr-{name}/pg{j}" for j in range(1, 5)} <= set(seen)
    assert sorted(seen[f"lr-{name}/pg{j}"] for j in range(1, 5)) == sorted(g["lr"] for g in groups)


def test_cli_flags_build_the_groups(tmp_path):
    import os

    from perceiver_io_amd.cli.tasks import main as cli_main

    flags = ["--data=IMDBDataModule", "--data.synthetic=true", "--data.synthetic_size=16", "--data.vocab_size=200",
             "--data.max_seq_len=32", "--data.batch_size=4", "--data.num_workers=0", "--model.num_latents=8",
             "--model.num_encoder_layers=1", "--model.num_encoder_self_attention_layers_per_block=1",
             "--model.masked_samples=null", "--trainer.max_steps=4", "--trainer.fast_dev_run=true", "--optimizer.lr=1e-3"]
    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        cli = cli_main("mlm", ["fit", *flags, "--model.no_decay_1d=true", "--model.encoder_lr_scale=0.1"])
    finally:
        os.chdir(old)
    assert cli.model.hparams["no_decay_1d"] is True and cli.model.hparams["encoder_lr_scale"] == 0.1
    groups = cli.trainer.optimizers[0].param_groups
    assert sorted((g["lr_scale"], g["weight_decay"]) for g in groups) == [(0.1, 0.0), (0.1, 0.01), (1.0, 0.0), (1.0, 0.01)]
    # OneCycleLR drives every group from its own max_lr
    assert [g["max_lr"] for g in groups] == pytest.approx([1e-3 * g["lr_scale"] for g in groups])
    assert cli.trainer.lr_schedulers[0].optimizer is cli.trainer.optimizers[0]
    enc = {id(p) for p in cli.model.model.encoder.parameters()}
    for g in groups:
        assert all((id(p) in enc) == (g["lr_scale"] == 0.1) for p in g["params"])


# ---- the Trainer's fused branch (forced on: on the CPU the fused optimizers run their emulation) ---------------
SCHED = {"class_path": "torch.optim.lr_scheduler.OneCycleLR", "init_args": {"max_lr": 1e-2, "total_steps": 10}}


def _fused_fit(tmp_path, fused, optimizer="torch.optim.AdamW", scale=0.1):
    from perceiver_io_amd.train.callbacks import LearningRateMonitor
    from perceiver_io_amd.train.trainer import Trainer

    class ForcedFused(Trainer):
        fused = True

    lit = _lit(no_decay_1d=True, encoder_lr_scale=scale, scheduler_init=SCHED,
               optimizer_init={"class_path": optimizer, "init_args": {"lr": 1e-2, "weight_decay": 0.05}})
    before = {n: p.detach().clone() for n, p in lit.model.named_parameters()}
    g = torch.Generator().manual_seed(11)
    data = [(torch.rand(4, 8, 8, 1, generator=g), torch.randint(0, 4, (4,), generator=g)) for _ in range(3)]
    tr = (ForcedFused if fused else Trainer)(
        logger=False, enable_checkpointing=False, callbacks=[LearningRateMonitor(logging_interval="step")],
        default_root_dir=str(tmp_path), accelerator="cpu", max_epochs=1, limit_train_batches=3, num_sanity_val_steps=0,
        enable_progress_bar=False, log_every_n_steps=1)
    seen = {}
    tr.log_scalars = seen.update
    tr.fit(lit, train_dataloaders=data)
    assert tr.global_step == 3
    return lit, tr, seen, before


@pytest.mark.parametrize("optimizer,fused_cls", [("torch.optim.AdamW", FusedAdamW), ("perceiver_io_amd.ops.optim.Lamb", FusedLamb)])
def test_trainer_fused_branch_keeps_the_groups(tmp_path, optimizer, fused_cls):
    lit, tr, seen, before = _fused_fit(tmp_path / "fused", True, optimizer)
    ref_lit, ref_tr, _, _ = _fused_fit(tmp_path / "plain", False, optimizer)
    opt, ref = tr.optimizers[0], ref_tr.optimizers[0]
    assert type(opt) is fused_cls and not isinstance(ref, FusedAdamW)
    # the groups of the optimizer it replaced: options and membership, group by group
    assert len(opt.param_groups) == len(ref.param_groups) == 4
    names = {id(p): n for n, p in lit.model.named_parameters()}
    ref_names = {id(p): n for n, p in ref_lit.model.named_parameters()}
    for g, r in zip(opt.param_groups, ref.param_groups):
        for k in ("lr", "weight_decay", "eps", "lr_scale", "max_lr", "initial_lr") + (
                ("exclude_1d",) if fused_cls is FusedLamb else ()):
            assert g[k] == r[k], k
        assert tuple(g["betas"]) == tuple(r["betas"])
        assert [names[id(p)] for p in g["params"]] == [ref_names[id(p)] for p in r["params"]]
    assert sorted((g["lr_scale"], g["weight_decay"]) for g in opt.param_groups) == [
        (0.1, 0.0), (0.1, 0.05), (1.0, 0.0), (1.0, 0.05)]
    # the scheduler is bound to the fused optimizer and drives every group from its own max_lr
    assert tr.lr_schedulers[0].optimizer is opt
    assert [g["max_lr"] for g in opt.param_groups] == pytest.approx([1e-2 * g["lr_scale"] for g in opt.param_groups])
    assert len({g["lr"] for g in opt.param_groups}) == 2
    assert {f"lr-{fused_cls.__name__}/pg{j}" for j in range(1, 5)} <= set(seen)
    # the flat buffer keeps model order whatever the groups
    assert [id(p) for p in opt.flat.params] == [id(p) for p in lit.parameters() if p.requires_grad]
    # the device words of the next update carry every group's scheduled lr and its weight decay
    hv = opt.hyper_values()
    for j, g in enumerate(opt.param_groups):
        assert hv[8 + 4 * j:10 + 4 * j] == [g["lr"], g["weight_decay"]]
    moved = [n for n, p in lit.model.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert len(moved) > 0 and opt._step == 3


def test_trainer_fused_branch_leaves_a_group_at_lr_zero_bitwise_unchanged(tmp_path):
    # --model.encoder_lr_scale=0: the encoder's two groups run at lr = max_lr = 0 under the scheduler
    lit, tr, seen, before = _fused_fit(tmp_path, True, scale=0.0)
    opt = tr.optimizers[0]
    assert type(opt) is FusedAdamW and len(opt.param_groups) == 4
    assert sorted(g["max_lr"] for g in opt.param_groups) == [0.0, 0.0, 1e-2, 1e-2]
    assert sorted(seen[f"lr-FusedAdamW/pg{j}"] for j in range(1, 5))[:2] == [0.0, 0.0]
    still = moved = 0
    for name, p in lit.model.named_parameters():
        if name.startswith("0."):  # the encoder: decayed or not, nothing moves at lr 0
            assert torch.equal(p.detach(), before[name]), name
            still += 1
        else:
            moved += int(not torch.equal(p.detach(), before[name]))
    assert still > 0 and moved > 0


def test_zero_encoder_lr_scale_and_unequal_lamb_eps():
    groups = _lit(encoder_lr_scale=0.0).configure_optimizers().param_groups
    assert sorted(g["lr"] for g in groups) == [0.0, 1e-2] and sorted(g["lr_scale"] for g in groups) == [0.0, 1.0]
    lit = _lit()
    lit.hparams["encoder_lr_scale"] = None
    assert len(lit.configure_optimizers().param_groups) == 1
    params = _params()
    with pytest.raises(ValueError, match="eps"):
        FusedLamb([{"params": params[:2]}, {"params": params[2:], "eps": 1e-8}])
    with pytest.raises(ValueError, match="missing from `flat`"):
        FusedAdamW(params, flat=FlatParameterSpace(params[:3], with_shadow=True))
