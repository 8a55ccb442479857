"""Weight EMA on the CPU: the schedule, the emulation of the update / swap kernels (the HIP
kernels' oracle, ops/emulation.py), the coupling to the fused optimizers and to the step engine's
replayed graphs, evaluation with the averaged weights, and ``--trainer.ema_*`` through the Trainer,
its checkpoints and the command line."""
import os
import warnings

import numpy as np
import pytest
import torch

from perceiver_io_amd.ops import emulation
from perceiver_io_amd.ops.optim import FlatParameterSpace, FusedAdamW, FusedLamb, WeightEMA

SHAPES = [(37, 5), (11,), (1,), (64, 64)]


def _params(seed=0, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]


def _grads(step, seed=1, shapes=SHAPES):
    g = torch.Generator().manual_seed(100 * seed + step)
    return [torch.randn(*s, generator=g) for s in shapes]


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad.copy_(g)


def _hyper(omd):
    h = torch.zeros(8)
    h[5] = omd
    return h


def _bits(t):
    return t.detach().contiguous().view(torch.uint8)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- schedule ----------------------------------------------------------------------------------
@pytest.mark.parametrize("decay,warmup,every", [(0.999, False, 1), (0.9999, True, 1), (0.99, True, 3)])
def test_schedule_follows_the_formula(decay, warmup, every):
    ema = WeightEMA(_params(), decay=decay, warmup=warmup, update_every=every)
    for t in range(1, 13):
        if t % every:
            want = 0.0
        else:
            u = t // every
            d = min(decay, (1 + u) / (10 + u)) if warmup else decay
            want = float(np.float32(1.0 - d))  # formed in double, rounded once
        got = ema.one_minus_decay(t)
        assert isinstance(got, float) and got == want, (t, got, want)
    # the warm-up really is in force early and gone late
    if warmup:
        assert ema.one_minus_decay(every) == float(np.float32(1.0 - 2.0 / 11.0))
        assert ema.one_minus_decay(10 ** 7 * every) == float(np.float32(1.0 - decay))


@pytest.mark.parametrize("decay", [-0.1, 1.0001, float("nan"), float("inf")])
def test_bad_decay_raises(decay):
    with pytest.raises(ValueError):
        WeightEMA(_params(), decay=decay)


# ---- emulation of the kernels -------------------------------------------------------------------
@pytest.mark.parametrize("omd", [0.25, float(np.float32(1.0 - 0.9999)), float(np.float32(1.0 - 2.0 / 11.0))])
def test_emulated_update_is_the_three_op_expression(omd):
    g = torch.Generator().manual_seed(3)
    e, w = torch.randn(1024 + 64, generator=g), torch.randn(1024 + 64, generator=g) * 3
    o = torch.tensor(omd, dtype=torch.float32)
    d = w - e
    p = o * d
    want = e + p
    got = e.clone()
    emulation.ema_update(got, w, _hyper(omd))
    assert _same(got, want)
    # and it is not the contracted form: some element differs from fma(omd, d, e) (a product by a
    # power of two is exact, so the two agree there)
    fused = (e.double() + o.double() * d.double()).float()
    assert torch.equal(fused, want) == (omd == 0.25)


def test_emulated_update_with_zero_and_one():
    g = torch.Generator().manual_seed(4)
    e, w = torch.randn(256, generator=g), torch.randn(256, generator=g) * 1e-3
    keep = e.clone()
    emulation.ema_update(e, w, _hyper(0.0))
    assert _same(e, keep)
    # decay = 0: the average is the weights themselves (e + (w − e) would not be, elementwise)
    assert not torch.equal(keep + (w - keep), w)
    emulation.ema_update(e, w, _hyper(1.0))
    assert _same(e, w)
    with pytest.raises(ValueError):
        emulation.ema_update(torch.zeros(6), torch.zeros(6), _hyper(0.5))


def test_emulated_update_tracks_a_float64_recurrence():
    """50 steps with a constant 1 − decay: three roundings per step, each at most half an ulp of a
    value bounded by max|w| (the difference by twice that, scaled down by omd ≤ 1/2), and the
    recurrence contracts errors by (1 − omd) — so 50 · 2⁻²³ · max|w| bounds the drift, with the
    same relative term on e itself."""
    g = torch.Generator().manual_seed(5)
    omd = float(np.float32(0.1))
    e = torch.randn(512, generator=g)
    ref = e.double()
    wmax = float(e.abs().max())
    for s in range(50):
        w = torch.randn(512, generator=g) * 2
        wmax = max(wmax, float(w.abs().max()))
        emulation.ema_update(e, w, _hyper(omd))
        ref = ref + omd * (w.double() - ref)
    bound = 50 * 2.0 ** -23 * wmax + 50 * 2.0 ** -23 * ref.abs()
    err = (e.double() - ref).abs()
    assert (err <= bound).all(), float((err / bound).max())


def test_emulated_swap():
    g = torch.Generator().manual_seed(6)
    w, e = torch.randn(128, generator=g), torch.randn(128, generator=g)
    s = torch.zeros(128, dtype=torch.bfloat16)
    w0, e0 = w.clone(), e.clone()
    emulation.ema_swap(w, e, s)
    assert _same(w, e0) and _same(e, w0) and _same(s, e0.to(torch.bfloat16))
    emulation.ema_swap(w, e, s)
    assert _same(w, w0) and _same(e, e0) and _same(s, w0.to(torch.bfloat16))
    emulation.ema_swap(w, e, None)
    assert _same(w, e0) and _same(e, w0)


# ---- optimizer coupling -----------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [FusedAdamW, FusedLamb])
def test_fused_optimizers_update_the_average_behind_every_step(cls):
    plain_params, params = _params(), _params()
    plain = cls(plain_params, lr=1e-2, weight_decay=0.01)
    opt = cls(params, lr=1e-2, weight_decay=0.01)
    assert opt.hyper_values()[5] == 0.0 and opt.bucket_updates_ok() == plain.bucket_updates_ok()
    ema = WeightEMA(opt.flat, decay=0.9, warmup=True, update_every=2)
    assert ema.avg.shape == (opt.flat.numel,) and ema.avg.dtype == torch.float32 and _same(ema.avg, opt.flat.data)
    assert ema.avg.data_ptr() != opt.flat.data.data_ptr()
    opt.attach_ema(ema)
    assert opt.bucket_updates_ok() is False
    moved = 0
    for t in range(1, 7):
        grads = _grads(t)
        for o, ps in ((plain, plain_params), (opt, params)):
            o.zero_grad()
            _set_grads(ps, grads)
        prev = ema.avg.clone()
        assert opt.hyper_values()[5] == ema.one_minus_decay(t)
        plain.step()
        opt.step()
        assert opt.hyper[5].item() == ema.one_minus_decay(t) and opt.hyper[2].item() == 0.0
        want = prev.clone()
        emulation.ema_update(want, opt.flat.data.clone(), _hyper(ema.one_minus_decay(t)))
        assert _same(ema.avg, want), t
        moved += int(not torch.equal(prev, ema.avg))
        assert (t % 2 == 0) == (not torch.equal(prev, ema.avg))
        # the weights are those of the run without an average
        assert _same(opt.flat.data, plain.flat.data) and _same(opt.flat.shadow, plain.flat.shadow)
    assert moved == 3
    pad = torch.ones(opt.flat.numel, dtype=torch.bool)
    for p, o in zip(opt.flat.params, opt.flat.offsets):
        pad[o:o + p.numel()] = False
    assert pad.any() and not ema.avg[pad].any()  # padding stays zero


def test_attach_needs_the_optimizers_own_flat_space():
    opt = FusedAdamW(_params(), lr=1e-2)
    with pytest.raises(ValueError):
        opt.attach_ema(WeightEMA(FlatParameterSpace(_params(1), with_shadow=True)))


# ---- step engine: eager warm-ups and replayed graphs ----------------------------------------------------
def _engine_run(with_ema, accumulate=1, steps=6):
    from perceiver_io_amd.train.engine import StepEngine

    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(6, 8), torch.nn.GELU(), torch.nn.Linear(8, 3))
    opt = FusedAdamW(net.parameters(), lr=1e-2, weight_decay=0.01)
    ema = None
    if with_ema:
        ema = WeightEMA(opt.flat, decay=0.9, warmup=False, update_every=2)
        opt.attach_ema(ema)
    ce = torch.nn.CrossEntropyLoss()
    eng = StepEngine(lambda b: ce(net(b[0]), b[1]), opt, graph=True, graph_impl="closure", warmup_eager=2,
                     accumulate=accumulate)
    g = torch.Generator().manual_seed(1)
    trace = []
    for t in range(1, steps + 1):
        micro = [(torch.randn(8, 6, generator=g), torch.randint(0, 3, (8,), generator=g)) for _ in range(accumulate)]
        prev = ema.avg.clone() if ema is not None else None
        eng.step(micro if accumulate > 1 else micro[0])
        if ema is not None:
            want = prev.clone()
            emulation.ema_update(want, opt.flat.data.clone(), _hyper(ema.one_minus_decay(t)))
            assert _same(ema.avg, want), t
            assert (t % 2 == 0) == (not torch.equal(prev, ema.avg)), t
        trace.append(opt.flat.data.clone())
    return eng, opt, ema, trace


@pytest.mark.parametrize("accumulate", [1, 2])
def test_replayed_steps_update_the_average_on_the_last_graph_only(monkeypatch, accumulate):
    eng, opt, ema, trace = _engine_run(True, accumulate)
    assert eng.replays == 4 * accumulate and eng.num_graphs == accumulate and opt._step == 6
    _, _, _, plain = _engine_run(False, accumulate)
    assert all(_same(a, b) for a, b in zip(trace, plain))
    if accumulate == 2:
        # replaying the "micro" graph alone moves neither the weights nor the average
        ent = [e for k, e in eng._graphs.items() if k[0] == "micro"][0]
        opt.stage_hyper()
        assert opt.hyper[5].item() == 0.0  # step 7: no update either way; force one to be seen
        opt.hyper[5] = 0.5
        before = ema.avg.clone()
        ent.graph.replay()
        assert _same(ema.avg, before)


# ---- evaluation with the averaged weights ------------------------------------------------------------
def _trained(cls=FusedAdamW):
    params = _params()
    opt = cls(params, lr=1e-2)
    ema = WeightEMA(opt.flat, decay=0.5, warmup=False)
    opt.attach_ema(ema)
    for t in range(1, 4):
        opt.zero_grad()
        _set_grads(params, _grads(t))
        opt.step()
    return params, opt, ema


def test_averaged_swaps_in_and_restores_bitwise():
    from perceiver_io_amd.ops.fused import weight_cache

    params, opt, ema = _trained()
    f = opt.flat
    data0, avg0, shadow0 = f.data.clone(), ema.avg.clone(), f.shadow.clone()
    assert not torch.equal(data0, avg0)
    ptrs = (f.data.data_ptr(), ema.avg.data_ptr(), f.shadow.data_ptr(), params[0].data_ptr())
    versions = [p._version for p in params]
    # the optimizer bound every parameter's cache entry to its slice of the flat shadow
    loose = weight_cache.get(params[0])
    assert loose.data_ptr() == f.views(f.shadow)[0].data_ptr()
    with ema.averaged() as inside:
        assert inside is ema and ema.swapped
        assert _same(f.data, avg0) and _same(ema.avg, data0) and _same(f.shadow, avg0.to(torch.bfloat16))
        for p, a in zip(params, f.views(avg0)):
            assert _same(p.detach(), a)
        assert all(p._version > v for p, v in zip(params, versions))
        # the bound entry still serves the (rewritten) shadow, no re-cast
        got = weight_cache.get(params[0])
        assert got.data_ptr() == loose.data_ptr() and _same(got, f.views(avg0)[0].to(torch.bfloat16))
        with pytest.raises(RuntimeError):
            opt.step()
        with pytest.raises(RuntimeError):
            ema.state_dict()
    assert not ema.swapped
    assert _same(f.data, data0) and _same(ema.avg, avg0) and _same(f.shadow, shadow0)
    assert ptrs == (f.data.data_ptr(), ema.avg.data_ptr(), f.shadow.data_ptr(), params[0].data_ptr())
    # the same when the body raises
    with pytest.raises(KeyError):
        with ema.averaged():
            assert _same(f.data, avg0)
            raise KeyError("body")
    assert not ema.swapped
    assert _same(f.data, data0) and _same(ema.avg, avg0) and _same(f.shadow, shadow0)


def test_version_keyed_caches_see_the_swap():
    """A weight-cache entry that is NOT the flat shadow (a flat space without one) is re-cast after
    the swap, and so is anything keyed on ``p._version``."""
    from perceiver_io_amd.ops.fused import WeightCache

    params = _params()
    flat = FlatParameterSpace(params, with_shadow=False)
    ema = WeightEMA(flat, decay=0.5)
    with torch.no_grad():
        ema.avg.mul_(2.0)
    cache = WeightCache()
    before = cache.get(params[0]).clone()
    ema.swap()
    after = cache.get(params[0])
    assert _same(after, params[0].detach().to(torch.bfloat16)) and not torch.equal(after, before)
    ema.swap()
    assert _same(cache.get(params[0]), before)


def test_parameter_list_form_and_state_dict():
    params = _params()
    ema = WeightEMA(params, decay=0.75, warmup=False, update_every=1)
    flat_params = _params()
    flat_ema = WeightEMA(FlatParameterSpace(flat_params, with_shadow=False), decay=0.75, warmup=False)
    for t in range(1, 4):
        with torch.no_grad():
            for p, q, g in zip(params, flat_params, _grads(t)):
                p.add_(g)
                q.add_(g)
        ema.update(t)
        flat_ema.update(t)
    sd = ema.state_dict()
    assert len(sd) == len(params) and all(_same(a, b) for a, b in zip(sd, flat_ema.state_dict()))
    assert all(a.shape == p.shape for a, p in zip(sd, params))
    w0 = [p.detach().clone() for p in params]
    v0 = [p._version for p in params]
    with ema.averaged():
        assert all(_same(p.detach(), a) for p, a in zip(params, sd))
        assert all(p._version > v for p, v in zip(params, v0))
    assert all(_same(p.detach(), w) for p, w in zip(params, w0)) and all(_same(a, b) for a, b in zip(ema.state_dict(), sd))
    fresh = WeightEMA(_params(), decay=0.75)
    fresh.load_state_dict(sd)
    assert all(_same(a, b) for a, b in zip(fresh.state_dict(), sd))
    with pytest.raises(ValueError):
        fresh.load_state_dict(sd[:-1])


# ---- Trainer -----------------------------------------------------------------------------------------
def _lit(lr=1e-2):
    from perceiver_io_amd.tasks import LitImageClassifier

    torch.manual_seed(0)
    return LitImageClassifier(image_shape=(8, 8, 1), num_classes=4, num_frequency_bands=4, num_latents=8,
                              num_latent_channels=16, num_encoder_layers=1,
                              num_encoder_self_attention_layers_per_block=1,
                              optimizer_init={"class_path": "torch.optim.AdamW",
                                              "init_args": {"lr": lr, "weight_decay": 0.0}})


def _data(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(4, 8, 8, 1, generator=g), torch.randint(0, 4, (4,), generator=g)) for _ in range(n)]


TRAIN, VAL = _data(6, 11), _data(2, 12)


def _fit(tmp_path, lr=1e-2, steps=3, callbacks=None, **flags):
    from perceiver_io_amd.train.trainer import Trainer

    lit = _lit(lr)
    tr = Trainer(logger=False, enable_checkpointing=bool(callbacks), callbacks=callbacks, default_root_dir=str(tmp_path),
                 accelerator="cpu", max_epochs=steps // 3, limit_train_batches=3, num_sanity_val_steps=1,
                 enable_progress_bar=False, **flags)
    # two epochs see the same three batches: a resumed run starts its epoch where this one does
    tr.fit(lit, train_dataloaders=TRAIN[:3], val_dataloaders=VAL)
    return lit, tr


@pytest.fixture(scope="module")
def plain_fit(tmp_path_factory):
    """Three steps without an average, and the same from a learning rate of zero (the freshly
    initialised model's validation loss on the same batches)."""
    lit, tr = _fit(tmp_path_factory.mktemp("plain"))
    lit0, tr0 = _fit(tmp_path_factory.mktemp("init"), lr=0.0)
    out = {"val": tr.callback_metrics["val_loss"], "init_val": tr0.callback_metrics["val_loss"],
           "weights": [p.detach().clone() for p in lit.parameters()],
           "init_weights": [p.detach().clone() for p in lit0.parameters()]}
    assert out["val"] != out["init_val"]
    assert all(_same(a, b.detach()) for a, b in zip(out["init_weights"], _lit().parameters()))
    return out


def test_trainer_decay_zero_evaluates_the_weights(tmp_path, plain_fit):
    lit, tr = _fit(tmp_path, ema_decay=0.0, ema_warmup=False)
    assert tr.ema is not None and tr.global_step == 3 and not tr.ema.swapped
    assert all(_same(a, p.detach()) for a, p in zip(tr.ema.state_dict(), tr.ema.params))
    assert all(_same(p.detach(), w) for p, w in zip(lit.parameters(), plain_fit["weights"]))
    assert tr.callback_metrics["val_loss"] == plain_fit["val"]


def test_trainer_decay_one_evaluates_the_initial_weights(tmp_path, plain_fit):
    lit, tr = _fit(tmp_path, ema_decay=1.0, ema_warmup=False)
    names = {id(p): i for i, p in enumerate(lit.parameters())}
    for a, p in zip(tr.ema.state_dict(), tr.ema.params):
        assert _same(a, plain_fit["init_weights"][names[id(p)]])
    assert tr.callback_metrics["val_loss"] == plain_fit["init_val"]
    # training itself went on with the raw weights
    assert all(_same(p.detach(), w) for p, w in zip(lit.parameters(), plain_fit["weights"]))
    # validate() after the fit evaluates the average as well
    assert tr.validate(lit, dataloaders=VAL, verbose=False)[0]["val_loss"] == plain_fit["init_val"]


def test_trainer_ema_eval_off_evaluates_the_raw_weights(tmp_path, plain_fit):
    lit, tr = _fit(tmp_path, ema_decay=1.0, ema_warmup=False, ema_eval=False)
    assert tr.ema is not None and tr.callback_metrics["val_loss"] == plain_fit["val"]


def test_trainer_without_ema_is_unchanged(tmp_path):
    lit, tr = _fit(tmp_path)
    assert tr.ema is None and getattr(tr.optimizers[0], "ema", None) is None
    with pytest.raises(ValueError):
        _fit(tmp_path, ema_decay=1.5)


# ---- checkpoints -----------------------------------------------------------------------------------------
EMA_FLAGS = dict(ema_decay=0.9, ema_warmup=True, ema_update_every=2)


def _ckpt_fit(tmp_path, steps, **flags):
    from perceiver_io_amd.train.callbacks import ModelCheckpoint

    ck = ModelCheckpoint(dirpath=str(tmp_path / "ck"), monitor=None, filename="{step}")
    lit, tr = _fit(tmp_path, steps=steps, callbacks=[ck], **EMA_FLAGS, **flags)
    return lit, tr, ck


def test_checkpoint_keys_and_averaged_state_dict(tmp_path):
    from perceiver_io_amd.train.checkpoint import averaged_state_dict

    lit, tr, ck = _ckpt_fit(tmp_path, 3)
    ckpt = torch.load(ck.last_model_path, map_location="cpu", weights_only=True)
    assert ckpt["ema"] == {"decay": 0.9, "warmup": True, "update_every": 2} and ckpt["global_step"] == 3
    esd, sd = ckpt["ema_state_dict"], ckpt["state_dict"]
    named = dict(lit.named_parameters())
    assert set(esd) == {n for n, p in named.items() if p.requires_grad} and set(esd) <= set(sd)
    # the checkpoint was written after the swap back: raw weights in state_dict, the average beside
    assert all(_same(sd[n], named[n].detach()) for n in esd)
    want = dict(zip([n for p in tr.ema.params for n, q in named.items() if q is p], tr.ema.state_dict()))
    assert all(_same(esd[n], want[n]) for n in esd) and any(not torch.equal(esd[n], sd[n]) for n in esd)
    avg = averaged_state_dict(ckpt)
    assert list(avg) == list(sd)
    assert all(_same(avg[k], esd[k] if k in esd else sd[k]) for k in sd)
    with pytest.raises(KeyError):
        averaged_state_dict({"state_dict": sd})
    # validate(ckpt_path=) evaluates the averaged tensors of the file
    from perceiver_io_amd.train.trainer import Trainer

    fresh = _lit()
    fresh.load_state_dict(avg)
    ref = Trainer(logger=False, enable_checkpointing=False, accelerator="cpu", enable_progress_bar=False)
    want_val = ref.validate(fresh, dataloaders=VAL, verbose=False)[0]["val_loss"]
    got_val = ref.validate(_lit(), dataloaders=VAL, ckpt_path=ck.last_model_path, verbose=False)[0]["val_loss"]
    assert got_val == want_val == tr.callback_metrics["val_loss"]
    raw = Trainer(logger=False, enable_checkpointing=False, accelerator="cpu", enable_progress_bar=False,
                  ema_eval=False)
    assert raw.validate(_lit(), dataloaders=VAL, ckpt_path=ck.last_model_path, verbose=False)[0]["val_loss"] != want_val


def test_resume_continues_the_average_bitwise(tmp_path):
    _, full, _ = _ckpt_fit(tmp_path / "full", 6)
    _, _, ck = _ckpt_fit(tmp_path / "half", 3)
    assert ck.last_model_path.endswith("step=3.ckpt")
    lit, res, _ = _ckpt_fit(tmp_path / "rest", 6, resume_from_checkpoint=ck.last_model_path)
    assert res.global_step == full.global_step == 6
    assert all(_same(a, b) for a, b in zip(res.ema.state_dict(), full.ema.state_dict()))
    assert all(_same(p.detach(), q.detach()) for p, q in zip(res.ema.params, full.ema.params))
    # a checkpoint without an average: a warning, and the average restarts from its weights
    _, plain = _fit(tmp_path / "noema", callbacks=None)
    plain.save_checkpoint(str(tmp_path / "noema.ckpt"))
    with pytest.warns(UserWarning, match="no weight EMA"):
        _fit(tmp_path / "warn", steps=6, resume_from_checkpoint=str(tmp_path / "noema.ckpt"), **EMA_FLAGS)


# ---- command line ---------------------------------------------------------------------------------------
def _parse(*flags):
    from perceiver_io_amd.cli import CLIParser
    from perceiver_io_amd.cli.tasks import task_cli

    cls = task_cli("img_clf")
    cli = cls.__new__(cls)
    cli.parser = CLIParser()
    cli.add_default_arguments_to_parser(cli.parser)
    cli.add_arguments_to_parser(cli.parser)
    return cli.parse(list(flags))[1]


def test_cli_flags_reach_the_trainer(tmp_path, capsys):
    from perceiver_io_amd.cli.tasks import main as cli_main

    cfg = _parse("fit")
    assert cfg["trainer"]["ema_decay"] is None and cfg["trainer"]["ema_warmup"] is True
    assert cfg["trainer"]["ema_update_every"] == 1 and cfg["trainer"]["ema_eval"] is True
    flags = ["--data=MNISTDataModule", "--data.synthetic=true", "--data.synthetic_size=24", "--data.batch_size=8",
             "--data.num_workers=0", "--data.val_split=8", "--model.num_encoder_layers=1", "--model.num_latents=8",
             "--model.num_encoder_self_attention_layers_per_block=1", "--trainer.limit_val_batches=1",
             "--trainer.accelerator=cpu", "--trainer.max_epochs=1", "--trainer.ema_decay=0.999",
             "--trainer.ema_update_every=2"]
    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        with pytest.raises(SystemExit) as e:
            cli_main("img_clf", ["fit", *flags, "--print_config"])
        assert e.value.code == 0
        out = capsys.readouterr().out
        assert "ema_decay: 0.999" in out and "ema_update_every: 2" in out and "ema_warmup: true" in out
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            cli = cli_main("img_clf", ["fit", *flags])
    finally:
        os.chdir(old)
    assert not [w for w in rec if "has no effect" in str(w.message)]
    tr = cli.trainer
    assert tr.ema_decay == 0.999 and tr.ema_update_every == 2 and tr.ema_warmup is True and tr.ema_eval is True
    assert tr.ema is not None and (tr.ema.decay, tr.ema.update_every) == (0.999, 2) and tr.global_step == 2
    ck = [c for c in tr.callbacks if type(c).__name__ == "ModelCheckpoint"][0]
    assert "ema_state_dict" in torch.load(ck.best_model_path, map_location="cpu", weights_only=True)
