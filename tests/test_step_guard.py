"""The step guard and the per-tensor gradient statistics on the CPU (ops/emulation.py, ops/optim.py,
the Trainer's eager path): the guard words, the guarded updates, the GradScaler invariant (a run with
one poisoned step ends bit for bit where the run without that step ends), ``tensor_stats`` against fp64
torch, the trainer flags ``skip_nonfinite_steps`` / ``max_skipped_steps`` / ``track_grad_norm``, and a
2-rank gloo run through the step engine in which only one rank's gradient is poisoned."""
import math
import os

import pytest
import torch
import torch.multiprocessing as mp

from optim_cases import NUMELS, flat_case
from perceiver_io_amd.ops import emulation as E

INF, NAN = float("inf"), float("nan")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _hyper(step, groups=0, due=0.0, slot=2.0):
    words = [2e-3, float(step), 0.0, 0.9, 0.999, 0.0, due, slot]
    for j in range(groups):
        words += [1e-3 * (j + 1), 0.01 * j, 1e-8, 0.0]
    return torch.tensor(words, dtype=torch.float32)


# ---- guard words -------------------------------------------------------------------------------
def test_guard_words_follow_the_partials():
    gscale = 0.5
    guard = torch.zeros(8)
    part = torch.rand(512, generator=torch.Generator().manual_seed(0))
    norm = math.sqrt(float(part.sum())) * gscale
    E.step_guard(part, _hyper(1), guard, gscale)
    assert guard[:4].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert guard[4].item() == pytest.approx(norm, rel=1e-6) and guard[5].item() == guard[4].item()
    assert guard[6].item() == 0.0
    for step, poison in ((2, INF), (3, NAN)):
        bad = part.clone()
        bad[17] = poison
        E.step_guard(bad, _hyper(step), guard, gscale)
        assert guard[0].item() == 1.0 and guard[1].item() == step - 1 and guard[2].item() == step - 1
        assert not math.isfinite(guard[4].item()) and guard[5].item() == pytest.approx(norm, rel=1e-6)
        assert guard[6].item() == step
    E.step_guard(part, _hyper(4), guard, gscale)  # a finite step: consecutive resets, total stays
    assert guard[:4].tolist() == [0.0, 2.0, 0.0, 2.0]  # effective step = hyper[1] − total
    assert guard[6].item() == 3.0
    # a finite gradient whose Σ g² overflows fp32 counts as non-finite
    big = torch.zeros(512)
    big[0] = big[1] = 2.5e38
    E.step_guard(big, _hyper(5), guard, gscale)
    assert guard[0].item() == 1.0 and guard[1].item() == 3.0 and guard[3].item() == 3.0


# ---- guarded updates ---------------------------------------------------------------------------
class _Bufs:
    def __init__(self, case):
        self.p, self.g, self.m, self.v = (case[k].clone() for k in "pgmv")
        self.shadow = torch.zeros(self.p.numel(), dtype=torch.bfloat16)
        self.loss, self.ring = torch.tensor(1.25), torch.zeros(4)
        self.trust = torch.full((len(NUMELS),), 7.0)
        self.partials = torch.zeros(2 * case["chunk_tab"].shape[0])

    def flat(self):
        return [self.p, self.g, self.m, self.v, self.shadow]

    def outputs(self):
        return dict(p=self.p, g=self.g, m=self.m, v=self.v, shadow=self.shadow, ring=self.ring, trust=self.trust)


def _launch(kind, case, b, step, zero_grad, guard):
    kw = dict(zero_grad=zero_grad, loss_src=b.loss, loss_ring=b.ring, **({} if guard is None else {"guard": guard}))
    tg = torch.tensor([t % 2 for t in range(len(NUMELS))], dtype=torch.int32)
    if kind == "adamw":
        E.adamw(*b.flat(), _hyper(step), 1e-8, 0.01, 0.0, 0.5, **kw)
    elif kind == "adamw_grouped":
        E.adamw_grouped(*b.flat(), _hyper(step, 2), case["chunk_tab"], tg, 2, 0.0, 0.5, **kw)
    else:
        E.lamb(*b.flat(), _hyper(step, 2), case["chunk_tab"], case["tensor_tab"], case["tensor_opt"], b.partials,
               b.trust, 1e-6, 0.0, 0.5, tensor_group=tg, **kw)


@pytest.mark.parametrize("zero_grad", [False, True])
@pytest.mark.parametrize("kind", ["adamw", "adamw_grouped", "lamb"])
def test_guarded_update_emulation(kind, zero_grad):
    case = flat_case("cpu")
    if kind == "adamw":  # the whole-buffer kernel walks the padding too: finite moments there
        case["m"], case["v"] = torch.nan_to_num(case["m"]), torch.nan_to_num(case["v"])
    ref, on = _Bufs(case), _Bufs(case)
    _launch(kind, case, ref, 3, zero_grad, None)
    _launch(kind, case, on, 3, zero_grad, torch.tensor([0.0, 0.0, 0.0, 3.0, 1.0, 1.0, 0.0, 0.0]))
    for k, t in ref.outputs().items():
        assert torch.equal(_bits(t), _bits(on.outputs()[k])), k  # skip 0, total 0: the unguarded call
    late = _Bufs(case)  # two skipped steps behind it: hyper[1] = 5 is effective step 3
    _launch(kind, case, late, 5, zero_grad, torch.tensor([0.0, 2.0, 0.0, 3.0, 1.0, 1.0, 4.0, 0.0]))
    for k, t in ref.outputs().items():
        assert torch.equal(_bits(t), _bits(late.outputs()[k])), k
    sk = _Bufs(case)
    sk.g[case["offsets"][2]] = NAN
    before = {k: t.clone() for k, t in sk.outputs().items()}
    _launch(kind, case, sk, 3, zero_grad, torch.tensor([1.0, 1.0, 1.0, 3.0, NAN, 1.0, 3.0, 0.0]))
    for k in ("p", "m", "v", "shadow", "trust"):
        assert torch.equal(_bits(before[k]), _bits(sk.outputs()[k])), k  # NaN padding compared by bits
    assert sk.ring[2].item() == 1.25
    if zero_grad:
        assert not sk.g[case["valid"]].any()
    else:
        assert torch.equal(_bits(before["g"]), _bits(sk.g))


# ---- the GradScaler invariant ------------------------------------------------------------------
def _net(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(6, 8), torch.nn.GELU(), torch.nn.Linear(8, 3))


@pytest.mark.parametrize("cls", ["FusedAdamW", "FusedLamb"])
def test_poisoned_step_equals_the_run_without_it(cls):
    from perceiver_io_amd.ops import optim

    C = getattr(optim, cls)
    a, b = _net(), _net()
    oa, ob = C(a.parameters(), lr=1e-2, weight_decay=0.01), C(b.parameters(), lr=1e-2, weight_decay=0.01, skip_nonfinite=True)
    assert oa.norm_part is None and oa.guard is None and ob.norm_part is not None
    xs = torch.randn(5, 4, 6, generator=torch.Generator().manual_seed(1))
    for i in range(5):
        if i != 2:
            oa.zero_grad()
            a(xs[i]).pow(2).mean().backward()
            oa.step()
        ob.zero_grad()
        (b(xs[i]).pow(2).mean() * (INF if i == 2 else 1.0)).backward()
        ob.step()
    assert torch.equal(oa.flat.data, ob.flat.data) and torch.equal(oa.exp_avg, ob.exp_avg)
    assert torch.equal(oa.exp_avg_sq, ob.exp_avg_sq) and torch.equal(_bits(oa.flat.shadow), _bits(ob.flat.shadow))
    h = ob.health()
    assert h["skipped"] == 1 and h["consecutive"] == 0 and h["last_skipped_step"] == 3
    assert math.isfinite(h["last_norm"]) and h["last_norm"] == h["last_finite_norm"]
    assert ob._step == 5 and ob.state_dict()["state"][0]["step"].item() == 4  # the effective step
    assert not ob.bucket_updates_ok()
    with pytest.raises(NotImplementedError):
        ob.range_update(0, 64)
    oc = C(_net().parameters(), lr=1e-2, skip_nonfinite=True)
    oc.load_state_dict(ob.state_dict())
    assert oc._step == 4 and oc.health()["skipped"] == 0


# ---- tensor_stats ------------------------------------------------------------------------------
def _stats_reference(case, g, w, gscale):
    rows = []
    for o, n in zip(case["offsets"], NUMELS):
        gt, wt = g[o:o + n].double(), w[o:o + n].double()
        mx = torch.where(torch.isnan(gt), torch.zeros_like(gt), gt.abs()).max()
        rows.append([float(gt.pow(2).sum().sqrt()) * gscale, float(wt.pow(2).sum().sqrt()), float(mx.float()) * gscale,
                     float((~torch.isfinite(gt)).sum())])
    return torch.tensor(rows, dtype=torch.float64)


def _check_stats(got, want):
    got, want = got.double().cpu(), want
    for col in (0, 1):
        fin = torch.isfinite(want[:, col])
        assert torch.equal(torch.isfinite(got[:, col]), fin)
        assert ((got[fin, col] - want[fin, col]).abs() <= 1e-5 * want[fin, col].abs()).all(), col
    assert torch.equal(got[:, 2].float(), want[:, 2].float()) and torch.equal(got[:, 3], want[:, 3])  # max, counts exact


def test_tensor_stats_emulation_against_fp64():
    case = flat_case("cpu")
    g, w = case["g"].clone(), case["p"].clone()
    g[case["offsets"][2] + 1] = NAN
    g[case["offsets"][9] + 5000] = INF
    T, C = len(NUMELS), case["chunk_tab"].shape[0]
    part, stats = torch.zeros(4 * C), torch.full((T, 4), -1.0)
    skip_stats = torch.full((T, 4), -2.0)
    E.tensor_stats(g, w, _hyper(3, due=0.0), case["chunk_tab"], case["tensor_tab"], part, stats, 0.5)
    assert (stats == -1.0).all()  # not due: untouched
    E.tensor_stats(g, w, _hyper(3, due=1.0), case["chunk_tab"], case["tensor_tab"], part, stats, 0.5)
    want = _stats_reference(case, g, w, 0.5)
    _check_stats(stats, want)
    assert want[:, 3].tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0, 1]  # the NaN padding of m / v and zero padding never counted
    assert want[9, 2].item() == INF and math.isnan(want[2, 0].item())
    stats.fill_(-1.0)  # a skipped step that is not due: the second buffer only
    guard = torch.tensor([1.0, 1.0, 1.0, 3.0, NAN, 1.0, 3.0, 0.0])
    E.tensor_stats(g, w, _hyper(3), case["chunk_tab"], case["tensor_tab"], part, stats, 0.5, guard=guard, skip_stats=skip_stats)
    assert (stats == -1.0).all()
    _check_stats(skip_stats, want)


def test_optimizer_statistics_requests():
    from perceiver_io_amd.ops.optim import FusedAdamW

    net = _net()
    plain = FusedAdamW(net.parameters(), lr=1e-2)
    assert plain.chunk_tab is None and plain.hyper.numel() == 8 and plain.hyper_values()[6] == 0.0
    with pytest.raises(RuntimeError):
        plain.request_stats()
    net = _net()
    opt = FusedAdamW(net.parameters(), lr=1e-2, tensor_stats=True, skip_nonfinite=True)
    x = torch.randn(4, 6, generator=torch.Generator().manual_seed(3))
    net(x).pow(2).mean().backward()
    grads = [p.grad.clone() for p in opt.flat.params]
    opt.step()
    assert not opt.tensor_stats().any()  # never requested
    opt.zero_grad()
    net(x).pow(2).mean().backward()
    grads = [p.grad.clone() for p in opt.flat.params]
    weights = [p.detach().clone() for p in opt.flat.params]
    opt.request_stats()
    opt.step()
    st = opt.tensor_stats()
    for row, gr, wt in zip(st.tolist(), grads, weights):
        assert row[0] == pytest.approx(float(gr.double().norm()), rel=1e-5)
        assert row[1] == pytest.approx(float(wt.double().norm()), rel=1e-5)
        assert row[2] == float(gr.abs().max()) and row[3] == 0
    assert opt.hyper_values()[6] == 0.0  # one request, one step
    opt.zero_grad()
    (net(x).pow(2).mean() * INF).backward()
    opt.step()
    assert opt.health()["skipped"] == 1 and (opt.skipped_tensor_stats()[:, 3] > 0).any()
    assert torch.equal(opt.tensor_stats(), st)


# ---- the Trainer on the CPU path ---------------------------------------------------------------
MLM_FLAGS = ["fit", "--data=IMDBDataModule", "--data.synthetic=true", "--data.synthetic_size=48", "--data.vocab_size=400",
             "--data.max_seq_len=48", "--data.batch_size=8", "--data.num_workers=0", "--model.num_latents=16",
             "--model.num_encoder_layers=1", "--model.num_encoder_self_attention_layers_per_block=1",
             "--model.masked_samples=null", "--optimizer.lr=0.003", "--trainer.limit_val_batches=1",
             "--trainer.max_steps=5", "--trainer.max_epochs=1", "--trainer.log_every_n_steps=1",
             "--trainer.num_sanity_val_steps=0"]


def poisoned_mlm(steps):
    """A test-local LitMaskedLanguageModel whose training loss is multiplied by a tensor that is inf on
    the attempted steps ``steps`` (1-based) and 1 otherwise.  The tensor is filled outside the
    (captured) step: in ``graph_batch`` on the graph path, at the top of ``training_step`` otherwise."""
    from perceiver_io_amd.tasks import LitMaskedLanguageModel

    class Poisoned(LitMaskedLanguageModel):
        _factor, _count = None, 0

        def _arm(self):
            self._count += 1
            if self._factor is None:
                self._factor = torch.ones((), device=next(self.parameters()).device)
            self._factor.fill_(INF if self._count in steps else 1.0)

        def graph_batch(self, batch):
            self._arm()
            return super().graph_batch(batch)

        def training_step(self, batch, batch_idx):
            if not self.trainer._engine.graph_enabled:
                self._arm()
            return super().training_step(batch, batch_idx) * self._factor

    Poisoned.__name__ = "LitMaskedLanguageModel"  # the checkpoint's hparams_name
    return Poisoned


def run_mlm(tmp_path, model_class, *flags):
    import perceiver_io_amd.data  # noqa: F401  (registers the data modules)
    from perceiver_io_amd.cli.tasks import task_cli

    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        return task_cli("mlm")(model_class, description="mlm", run=True,
                               args=MLM_FLAGS + ["--data.data_dir=" + str(tmp_path / "cache"), *flags])
    finally:
        os.chdir(old)


def _trainable_names(model):
    return [n for n, p in model.named_parameters() if p.requires_grad]


def test_trainer_defaults_add_nothing(tmp_path):
    from perceiver_io_amd.ops.optim import FusedAdamW

    tr = run_mlm(tmp_path, poisoned_mlm(())).trainer
    assert not any(k.startswith("grad_") or k == "skipped_steps" for k in tr.callback_metrics)
    assert tr.skip_nonfinite_steps is False and tr.track_grad_norm is None and tr.max_skipped_steps == 25
    opt = FusedAdamW(_net().parameters(), **tr._health_options())
    assert opt.norm_part is None and opt.guard is None and opt.chunk_tab is None and not opt.track_stats


@pytest.mark.parametrize("kind,prefix", [("2", "grad_2.0_norm"), ("inf", "grad_inf_norm")])
def test_trainer_track_grad_norm_keys(tmp_path, kind, prefix):
    cli = run_mlm(tmp_path, poisoned_mlm(()), f"--trainer.track_grad_norm={kind}", "--trainer.max_steps=2")
    m = cli.trainer.callback_metrics
    names = _trainable_names(cli.model)
    assert math.isfinite(m[prefix + "_total"]) and m[prefix + "_total"] > 0
    assert sorted(k for k in m if k.startswith(prefix + "/")) == sorted(f"{prefix}/{n}" for n in names)
    per = [m[f"{prefix}/{n}"] for n in names]
    total = math.sqrt(sum(v * v for v in per)) if kind == "2" else max(per)
    assert m[prefix + "_total"] == pytest.approx(total, rel=1e-5)


def test_trainer_track_grad_norm_refuses_other_norms(tmp_path):
    with pytest.raises(ValueError, match="track_grad_norm"):
        run_mlm(tmp_path, poisoned_mlm(()), "--trainer.track_grad_norm=3")


def test_trainer_skips_a_poisoned_step(tmp_path, capsys):
    from perceiver_io_amd.train.checkpoint import load_checkpoint

    cli = run_mlm(tmp_path, poisoned_mlm((3,)), "--trainer.skip_nonfinite_steps=true", "--trainer.track_grad_norm=2",
                  "--trainer.val_check_interval=5")
    tr = cli.trainer
    assert tr.global_step == 5 and tr.callback_metrics["skipped_steps"] == 1
    assert all(torch.isfinite(p).all() for p in cli.model.parameters())
    assert tr.skip_report.startswith("step 3:") and "tensors with non-finite gradients: " in tr.skip_report
    assert "step 3:" in capsys.readouterr().err
    ck = [c for c in tr.callbacks if type(c).__name__ == "ModelCheckpoint"][0]
    ckpt = load_checkpoint(ck.best_model_path)
    assert ckpt["global_step"] == 5  # attempted steps; the optimizer's step is the effective one
    assert {int(float(st["step"])) for st in ckpt["optimizer_states"][0]["state"].values()} == {4}
    assert not any("guard" in k or "skip" in k for k in ckpt)


def test_trainer_raises_past_max_skipped_steps(tmp_path):
    with pytest.raises(RuntimeError, match=r"max_skipped_steps=1 consecutive skipped steps at step 3: step 3:"):
        run_mlm(tmp_path, poisoned_mlm((2, 3)), "--trainer.skip_nonfinite_steps=true", "--trainer.max_skipped_steps=1")


# ---- data parallel: one rank's poison, every rank's skip -----------------------------------------
def _ddp_worker(rank, world, port, out):
    import test_ddp_engine as D

    D._env(rank, world, port)
    D._fused_on_cpu()
    from perceiver_io_amd.ops.optim import FusedAdamW
    from perceiver_io_amd.parallel import FlatGradReducer, dist
    from perceiver_io_amd.parallel.reducer import params_in_sync
    from perceiver_io_amd.train.engine import StepEngine

    dist.init(device_type="cpu")
    model = D._model()
    opt = FusedAdamW(model.parameters(), lr=1e-2, eps=0.1, weight_decay=0.01, skip_nonfinite=True)
    red = FlatGradReducer(opt.flat, bucket_bytes=16 << 10, overlap=True, in_graph=True)
    red.plan(model)
    red.broadcast_parameters(model)
    factor = torch.ones(())
    loss = D._loss_fn(model)
    eng = StepEngine(lambda b: loss(b) * factor, opt, reducer=red, graph=True, warmup_eager=1, graph_impl="closure")
    data, sync, kept = D._batches(rank, 4, 1), [], None
    for s in range(4):
        factor.fill_(INF if (s == 2 and rank == 1) else 1.0)  # a replayed step, rank 1 only
        before = opt.flat.data.clone()
        eng.step(data[s][0])
        sync.append(params_in_sync(opt.flat))
        if s == 2:
            kept = torch.equal(before, opt.flat.data)
    out[rank] = dict(sync=sync, kept=kept, health=opt.health(), finite=bool(torch.isfinite(opt.flat.data).all()),
                     bucket=eng.bucket_update, replays=eng.replays)
    red.close()
    dist.shutdown()


@pytest.mark.timeout(300)
def test_two_ranks_skip_together():
    import test_ddp_engine as D

    out = mp.Manager().dict()
    mp.spawn(_ddp_worker, args=(2, D._port(), out), nprocs=2, join=True)
    for rank in (0, 1):
        r = out[rank]
        assert r["sync"] == [0.0] * 4, r["sync"]  # the largest difference between the ranks' parameters
        assert r["kept"] and r["finite"] and not r["bucket"] and r["replays"] >= 2
        assert r["health"]["skipped"] == 1 and r["health"]["last_skipped_step"] == 3
