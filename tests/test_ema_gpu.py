"""Weight EMA on the GPU (csrc/ema.hip): the update and swap kernels against their emulation, bit
for bit; the update inside captured steps (``hyper[5]`` restaged on every replay); and a Trainer
run whose validation swaps the average in and out between replayed steps."""
import numpy as np
import pytest
import torch

from perceiver_io_amd.train.callbacks import Callback

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


def _bits(t):
    return t.detach().contiguous().view(torch.uint8)


def _same(a, b):
    a, b = a.cpu(), b.cpu()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _hyper(omd, device="cpu"):
    # the optimizer's block: lr, step, 0, betas, 1 − decay, 0, loss-ring slot
    return torch.tensor([1e-3, 3.0, 0.0, 0.9, 0.999, omd, 0.0, 2.0], dtype=torch.float32, device=device)


# one pass of the launcher's capped grid covers EMA_PASS_ELEMS = 2048 blocks · 256 threads · 4 =
# 2,097,152 elements; 2 passes and a partial third one, with a partial last block
N_STRIDE = 2 * 2097152 + 1024 + 64
SIZES = [64, 1024 + 64, N_STRIDE]


@pytest.fixture(scope="module")
def operands():
    """Normal-range fp32 values (|x| in [2⁻²⁰, 2²⁰), both signs, no subnormals) per size."""
    out = {}
    for n in SIZES:
        g = torch.Generator().manual_seed(n)
        def draw():
            mag = torch.exp2(torch.rand(n, generator=g) * 40 - 20)
            sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
            return (mag * sign).float()
        e, w = draw(), draw()
        w[::7] = e[::7] * 1.0001  # close pairs too: the differences that cancel
        assert torch.isfinite(e).all() and (e.abs() >= 2.0 ** -126).all() and (w.abs() >= 2.0 ** -126).all()
        out[n] = (e, w)
    return out


@pytest.mark.parametrize("omd", [0.25, float(np.float32(1.0 - 0.9999)), 1.0])
@pytest.mark.parametrize("n", SIZES)
def test_ema_update_kernel_is_the_emulation_bitwise(operands, n, omd):
    from perceiver_io_amd.ops import emulation

    assert _ext().EMA_PASS_ELEMS == 2097152 and N_STRIDE > 2 * _ext().EMA_PASS_ELEMS
    e, w = operands[n]
    want = e.clone()
    emulation.ema_update(want, w, _hyper(omd))
    assert not torch.equal(want, e)
    got, wd = e.to(DEV), w.to(DEV)
    _ext().ema_update(got, wd, _hyper(omd, DEV))
    torch.cuda.synchronize()
    assert _same(got, want)
    assert _same(wd, w)  # the weights are only read
    if omd == 1.0:
        assert _same(got, w)


@pytest.mark.parametrize("n", SIZES)
def test_ema_update_with_zero_leaves_the_buffer_untouched(operands, n):
    e, w = operands[n]
    got = e.to(DEV)
    got[:4] = torch.tensor([float("nan"), float("inf"), -0.0, 1e-42], device=DEV)  # anything at all stays
    keep = got.clone()
    _ext().ema_update(got, w.to(DEV), _hyper(0.0, DEV))
    torch.cuda.synchronize()
    assert _same(got, keep)


def test_launchers_refuse_what_they_cannot_vectorise():
    K = _ext()
    h = _hyper(0.5, DEV)
    for n in (6, 63, 1025):
        e, w = torch.ones(n, device=DEV), torch.zeros(n, device=DEV)
        with pytest.raises(RuntimeError, match="multiple of 4"):
            K.ema_update(e, w, h)
        with pytest.raises(RuntimeError, match="multiple of 4"):
            K.ema_swap(w, e, None)
        torch.cuda.synchronize()
        assert (e == 1).all() and (w == 0).all()  # refused, not launched
    buf = torch.zeros(72, device=DEV)
    with pytest.raises(RuntimeError, match="aligned"):
        K.ema_update(buf[1:65], buf[4:68].clone(), h)
    with pytest.raises(RuntimeError):
        K.ema_update(torch.zeros(64, device=DEV), torch.zeros(128, device=DEV), h)
    with pytest.raises(RuntimeError):
        K.ema_update(torch.zeros(64, device=DEV), torch.zeros(64, device=DEV), h[:4])
    with pytest.raises(RuntimeError):
        K.ema_swap(torch.zeros(64, device=DEV), torch.zeros(64, device=DEV), torch.zeros(64, device=DEV))  # fp32 shadow


def _swap_operands(n):
    g = torch.Generator().manual_seed(n + 1)
    w, e = torch.randn(n, generator=g), torch.randn(n, generator=g) * 100
    # ±0, ±inf, and bf16 rounding ties: fp32 values whose low 16 bits are exactly 0x8000, on an
    # even and on an odd bf16 mantissa, both signs (round to nearest even goes down / up)
    ties = torch.tensor([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x7F7F8000, 0x00808000],
                        dtype=torch.int64).to(torch.int32).view(torch.float32)
    special = torch.cat([torch.tensor([0.0, -0.0, float("inf"), float("-inf")]), ties])
    e[:special.numel()] = special
    w[-special.numel():] = special.flip(0)
    return w, e


@pytest.mark.parametrize("n", SIZES)
def test_ema_swap_exchanges_and_writes_the_shadow(n):
    K = _ext()
    w0, e0 = _swap_operands(n)
    w, e = w0.to(DEV), e0.to(DEV)
    s = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
    K.ema_swap(w, e, s)
    torch.cuda.synchronize()
    assert _same(w, e0) and _same(e, w0)
    assert _same(s, e0.to(torch.bfloat16)) and _same(s, w.to(torch.bfloat16))
    # the tie cases really are ties, rounded to even
    assert s[4:8].view(torch.int16).tolist() == [0x3F80, 0x3F82, 0xBF80 - 0x10000, 0xBF82 - 0x10000]
    K.ema_swap(w, e, s)
    torch.cuda.synchronize()
    assert _same(w, w0) and _same(e, e0) and _same(s, w0.to(torch.bfloat16))
    # without a shadow
    K.ema_swap(w, e, None)
    torch.cuda.synchronize()
    assert _same(w, e0) and _same(e, w0) and _same(s, w0.to(torch.bfloat16))


def test_swap_emulation_is_the_kernel():
    from perceiver_io_amd.ops import emulation

    w0, e0 = _swap_operands(1024 + 64)
    w, e, s = w0.clone(), e0.clone(), torch.zeros(1024 + 64, dtype=torch.bfloat16)
    emulation.ema_swap(w, e, s)
    wg, eg, sg = w0.to(DEV), e0.to(DEV), torch.zeros(1024 + 64, dtype=torch.bfloat16, device=DEV)
    _ext().ema_swap(wg, eg, sg)
    torch.cuda.synchronize()
    assert _same(wg, w) and _same(eg, e) and _same(sg, s)


# ---- the captured step ---------------------------------------------------------------------------------
def _smoke_mlm():
    from perceiver_io_amd.tasks import LitMaskedLanguageModel

    # the model of __graft_entry__.smoke
    return LitMaskedLanguageModel(vocab_size=1000, max_seq_len=128,
                                  optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3}},
                                  num_latents=64, num_latent_channels=64, num_encoder_layers=2,
                                  num_encoder_self_attention_layers_per_block=2).to(DEV)


def _captured_run(cls, with_ema):
    from perceiver_io_amd.ops import emulation
    from perceiver_io_amd.ops.optim import WeightEMA
    from perceiver_io_amd.train.engine import StepEngine

    torch.manual_seed(2)
    ids = torch.randint(3, 1000, (4, 128), device=DEV)
    pad = torch.zeros(4, 128, dtype=torch.bool, device=DEV)
    pad[1, 100:] = True
    torch.manual_seed(3)
    m = _smoke_mlm().model
    with torch.no_grad():  # one fixed masking: no RNG inside the step
        xm, lab = m.masking(ids, pad, generator=torch.Generator(device=DEV).manual_seed(7))
    opt = cls(m.parameters(), lr=1e-3)
    ema = None
    if with_ema:
        ema = WeightEMA(opt.flat, decay=0.9, warmup=True, update_every=2)
        opt.attach_ema(ema)
    eng = StepEngine(lambda b: m.loss(b[1], b[2], labels=lab, x_masked=xm), opt, device=DEV, graph=True,
                     warmup_eager=2)
    for t in range(1, 7):
        prev = ema.avg.clone() if with_ema else None
        eng.step((None, ids, pad))
        torch.cuda.synchronize()
        if with_ema:
            want = prev.cpu()
            emulation.ema_update(want, opt.flat.data.clone().cpu(), _hyper(ema.one_minus_decay(t)))
            assert _same(ema.avg, want), t
            assert (t % 2 == 0) == (not torch.equal(prev, ema.avg)), t
    assert eng.replays == 4 and eng.num_graphs == 1 and opt._step == 6
    return opt.flat.data.clone(), opt.flat.shadow.clone()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["FusedAdamW", "FusedLamb"])
def test_captured_step_updates_the_average_and_leaves_the_weights_alone(name):
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops import optim

    ops.set_deterministic(True)  # put back by the autouse fixture
    cls = getattr(optim, name)
    data, shadow = _captured_run(cls, True)
    plain_data, plain_shadow = _captured_run(cls, False)  # bitwise the run without an average
    assert _same(data, plain_data) and _same(shadow, plain_shadow)
    assert _same(shadow, data.to(torch.bfloat16))
    ops.check_device_errors()


# ---- Trainer ---------------------------------------------------------------------------------------------
class _Probe(Callback):
    """Records, around every validation, what the swap has to put back."""

    def __init__(self):
        self.last, self.at_val, self.val_losses = None, [], []

    def on_train_batch_end(self, trainer, module):
        f = trainer.optimizers[0].flat
        self.last = (f.data.clone(), f.shadow.clone())  # as the optimizer's own kernel wrote them

    def on_validation_end(self, trainer, module):
        if trainer.sanity_checking:
            return
        f = trainer.optimizers[0].flat
        self.at_val.append((trainer.global_step, trainer._engine.replays, f.data.clone(), f.shadow.clone(), self.last))
        self.val_losses.append(trainer.callback_metrics["val_loss"])


def _trainer_run(**flags):
    from perceiver_io_amd.ops import masking
    from perceiver_io_amd.train.trainer import Trainer

    torch.manual_seed(0)
    masking.reset_mask_state()  # the device's masking stream restarts from this seed in every run
    lit = _smoke_mlm()
    g = torch.Generator().manual_seed(5)
    data = [(torch.zeros(4, dtype=torch.long), torch.randint(3, 1000, (4, 128), generator=g),
             torch.zeros(4, 128, dtype=torch.bool)) for _ in range(7)]
    probe = _Probe()
    tr = Trainer(logger=False, enable_checkpointing=False, callbacks=[probe], accelerator="gpu", devices=1,
                 max_steps=6, val_check_interval=3, limit_val_batches=1, num_sanity_val_steps=1, deterministic=True,
                 enable_progress_bar=False, **flags)
    tr.fit(lit, train_dataloaders=data[:6], val_dataloaders=data[6:])
    torch.cuda.synchronize()
    return tr, probe


@pytest.fixture(scope="module")
def plain_run():
    try:
        return _trainer_run()
    finally:
        torch.use_deterministic_algorithms(False)


def _check_training_went_on(tr, probe, plain):
    f, pf = tr.optimizers[0].flat, plain.optimizers[0].flat
    assert tr.fused and tr._engine.graph_enabled and tr.ema is not None and tr.optimizers[0].ema is tr.ema
    assert [s for s, *_ in probe.at_val] == [3, 6] and not tr.ema.swapped
    for step, replays, data, shadow, last in probe.at_val:
        # after the swap back: the weights and the shadow the optimizer wrote before validation
        assert _same(data, last[0]) and _same(shadow, last[1]), step
        assert _same(shadow, data.to(torch.bfloat16)), step
    # training went on through the same graph: replays kept rising, and the shadow the optimizer
    # wrote in the steps after the swap back is the bf16 of its weights, as in the plain run
    assert probe.at_val[0][1] >= 1 and probe.at_val[1][1] == probe.at_val[0][1] + 3 == tr._engine.replays
    assert tr._engine.num_graphs == 1 and tr.global_step == 6
    assert _same(f.shadow, f.data.to(torch.bfloat16))
    assert _same(f.data, pf.data) and _same(f.shadow, pf.shadow)


@pytest.mark.timeout(300)
def test_trainer_validates_with_the_average_between_replayed_steps(plain_run):
    plain, pp = plain_run
    try:
        tr, probe = _trainer_run(ema_decay=0.0, ema_warmup=False)
    finally:
        torch.use_deterministic_algorithms(False)
    assert plain.ema is None and plain.optimizers[0].hyper[5].item() == 0.0
    assert tr.optimizers[0].hyper[5].item() == 1.0
    # decay = 0: the average is the weights, so validation sees what the plain run sees
    assert len(probe.val_losses) == 2 and probe.val_losses == pp.val_losses
    assert _same(tr.ema.avg, tr.optimizers[0].flat.data)
    _check_training_went_on(tr, probe, plain)


@pytest.mark.timeout(300)
def test_trainer_swaps_a_different_average_in_and_back(plain_run):
    plain, pp = plain_run
    try:
        tr, probe = _trainer_run(ema_decay=0.9, ema_warmup=False)
    finally:
        torch.use_deterministic_algorithms(False)
    assert not torch.equal(tr.ema.avg, tr.optimizers[0].flat.data)
    assert probe.val_losses != pp.val_losses  # other weights were evaluated
    _check_training_went_on(tr, probe, plain)
