"""Soft-target classifier head, batch mixing and the MixUp / CutMix draw on CPU: the kernels'
emulation against fp64 autograd and the formulas written out, the host draw's statistics, and the
options through the CLI and the Trainer."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _head_case(M=45, V=37, C=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    h = _bf(torch.randn(M, C, generator=g))
    w = (torch.randn(V, C, generator=g) * 0.3).to(torch.bfloat16)
    bias = _bf(torch.randn(V, generator=g) * 0.1)
    a = torch.randint(0, V, (M,), generator=g)
    b = torch.randint(0, V, (M,), generator=g)
    b[::5] = a[::5]  # rows with b == a
    return h, w, bias, a, b, g


def _oracle(h, w, bias, a, b, lam, eps, gout):
    """fp64 autograd of F.cross_entropy with explicit probability targets, mean over the labelled rows"""
    hd = h.double().requires_grad_()
    wd = w.double().requires_grad_()
    bd = bias.double().requires_grad_()
    z = hd @ wd.t() + bd
    V = z.shape[1]
    valid = a != -100
    ac, bc = a.clamp(min=0), b.clamp(min=0)
    lm = lam.double()[:, None]
    t = (1 - eps) * (lm * F.one_hot(ac, V).double() + (1 - lm) * F.one_hot(bc, V).double()) + eps / V
    rows = F.cross_entropy(z, t, reduction="none")
    loss = (rows * valid.double()).sum() / max(int(valid.sum()), 1)
    (loss * gout).backward()
    return loss.detach(), hd.grad, wd.grad, bd.grad, z.detach()


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("lam_kind", ["zero", "one", "random"])
@pytest.mark.parametrize("labels", ["every7", "none"])
def test_emulation_matches_fp64_autograd(eps, lam_kind, labels):
    from perceiver_io_amd.ops import emulation

    h, w, bias, a, b, g = _head_case()
    M, V = h.shape[0], w.shape[0]
    lam = {"zero": torch.zeros(M), "one": torch.ones(M), "random": torch.rand(M, generator=g)}[lam_kind]
    if labels == "every7":
        a[::7] = -100
    else:
        a[:] = -100
    gout = 0.37
    loss, lse, pred, hs, cnt = emulation.soft_ce_fwd(h, a, b, lam, w, bias, eps)
    dH = torch.full((M, h.shape[1]), 3.0)
    dW, db = torch.full((V, h.shape[1]), 7.0), torch.full((V,), 7.0)
    emulation.soft_ce_bwd(hs, a, b, lam, w, bias, eps, lse, torch.tensor([gout]), cnt, dH, dW, db, False)
    rl, rh, rw, rb, z = _oracle(h, w.float(), bias, a, b, lam, eps, gout)
    assert cnt.item() == float((a != -100).sum())
    assert hs.dtype == torch.bfloat16 and torch.equal(hs.float(), h)
    assert torch.equal(pred.long(), z.float().argmax(-1)) and pred.dtype == torch.int32
    if labels == "none":  # loss 0, zero gradients, no NaN
        assert loss.item() == 0.0
        assert all(torch.equal(t, torch.zeros_like(t)) for t in (dH, dW, db))
        return
    errs = {"loss": abs(loss.item() - rl.item()) / abs(rl.item()), "dH": _rel(dH, rh), "dW": _rel(dW, rw),
            "db": _rel(db, rb)}
    print(errs)
    assert all(e < 1e-5 for e in errs.values()), errs
    assert torch.equal(dH[::7], torch.zeros_like(dH[::7]))  # rows without a label
    if lam_kind == "one":  # hard labels: label smoothing of F.cross_entropy
        valid = a != -100
        ref = F.cross_entropy(z[valid], a[valid], label_smoothing=eps)
        assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
    # accumulate adds to what the gradient tensors hold
    dW2, db2 = torch.full_like(dW, 2.0), torch.full_like(db, -1.0)
    emulation.soft_ce_bwd(hs, a, b, lam, w, bias, eps, lse, torch.tensor([gout]), cnt, torch.empty_like(dH), dW2, db2,
                          True)
    assert torch.allclose(dW2 - 2.0, dW, atol=1e-6) and torch.allclose(db2 + 1.0, db, atol=1e-6)


def test_emulation_pred_tie_rule():
    """h = 0: the logits are the bias; two equal maxima → the lower index"""
    from perceiver_io_amd.ops import emulation

    V, C, M = 40, 64, 5
    w = torch.randn(V, C).to(torch.bfloat16)
    bias = torch.zeros(V)
    bias[33] = bias[17] = 2.5
    a = torch.zeros(M, dtype=torch.int64)
    pred = emulation.soft_ce_fwd(torch.zeros(M, C), a, a, torch.ones(M), w, bias, 0.0)[2]
    assert pred.tolist() == [17] * M


def _mix_words(mode, lam=1.0, box=(0, 0, 0, 0)):
    return torch.tensor([float(mode), lam, *map(float, box)], dtype=torch.float32)


@pytest.mark.parametrize("B", [1, 4, 5])
@pytest.mark.parametrize("shape", [(8, 8, 1), (6, 10, 3)])
def test_emulation_batch_mix(B, shape):
    from perceiver_io_amd.ops import emulation

    H, W, Ch = shape
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, H, W, Ch, generator=g)
    y = torch.randint(0, 10, (B,), generator=g)
    x0, y0 = x.clone(), y.clone()
    # mode 0
    out, yb, lam = emulation.batch_mix(x, y, _mix_words(0, 0.3, (1, 2, 3, 4)))
    assert torch.equal(out, x) and out.data_ptr() != x.data_ptr()
    assert torch.equal(yb, y) and torch.equal(lam, torch.ones(B))
    # MixUp
    lm = 0.3
    out, yb, lam = emulation.batch_mix(x, y, _mix_words(1, lm))
    for i in range(B):
        j = B - 1 - i
        want = x[i] if i == j else torch.tensor(lm) * x[i] + (1.0 - torch.tensor(lm)) * x[j]
        assert torch.equal(out[i], want), i
        assert yb[i] == y[j]
    assert torch.equal(lam, torch.full((B,), lm))
    # CutMix with a box clipped at the border (rows 3..H, columns 0..2)
    out, yb, lam = emulation.batch_mix(x, y, _mix_words(2, 0.75, (3, H, 0, 2)))
    for i in range(B):
        j = B - 1 - i
        want = x[i].clone()
        want[3:H, 0:2] = x[j][3:H, 0:2]
        assert torch.equal(out[i], want), i
        assert yb[i] == y[j]
    if B % 2:  # the middle sample pairs with itself: unchanged
        assert torch.equal(out[B // 2], x[B // 2])
    assert torch.equal(lam, torch.full((B,), 0.75))
    assert torch.equal(x, x0) and torch.equal(y, y0)  # inputs unmodified


def test_draw_box_area_equals_one_minus_lambda():
    from perceiver_io_amd.tasks import draw_mix

    rng = np.random.default_rng(7)
    H, W = 28, 20
    seen_clipped = False
    for _ in range(300):
        mode, lam, y0, y1, x0, x1 = draw_mix(rng, (H, W), cutmix_alpha=1.0)
        assert mode == 2.0
        assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W
        assert all(float(v).is_integer() for v in (y0, y1, x0, x1))
        area = (y1 - y0) * (x1 - x0)
        assert lam == 1.0 - area / (H * W)  # λ reset to the clipped box, exactly
        assert abs(area / (H * W) - (1.0 - lam)) < 1e-15
        seen_clipped |= y0 == 0 or x0 == 0 or y1 == H or x1 == W
    assert seen_clipped


def test_draw_mode_frequencies():
    from perceiver_io_amd.tasks import draw_mix

    n, p_mix, p_cut = 2000, 0.7, 0.3
    rng = np.random.default_rng(11)
    modes = np.array([draw_mix(rng, (16, 16), 0.8, 1.0, p_mix, p_cut)[0] for _ in range(n)])
    for mode, p in ((0.0, 1 - p_mix), (1.0, p_mix * (1 - p_cut)), (2.0, p_mix * p_cut)):
        k = int((modes == mode).sum())
        assert abs(k - n * p) <= 4 * math.sqrt(n * p * (1 - p)), (mode, k, n * p)
    # one alpha only: that mode whenever the batch is mixed
    assert {draw_mix(rng, (16, 16), 0.8, 0.0)[0] for _ in range(50)} == {1.0}
    assert {draw_mix(rng, (16, 16), 0.0, 1.0)[0] for _ in range(50)} == {2.0}
    # both alphas zero: never mixed
    assert all(draw_mix(rng, (16, 16), 0.0, 0.0) == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0] for _ in range(50))
    lams = [draw_mix(rng, (16, 16), 0.8, 0.0)[1] for _ in range(50)]
    assert all(0.0 <= v <= 1.0 for v in lams) and len(set(lams)) > 40


def _tiny_img(**kw):
    from perceiver_io_amd.tasks import LitImageClassifier

    return LitImageClassifier(image_shape=(28, 28, 1), num_classes=10,
                              optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3}},
                              num_latents=8, num_latent_channels=64, num_encoder_layers=1,
                              num_encoder_self_attention_layers_per_block=1, num_frequency_bands=4, **kw)


def test_model_soft_loss_matches_cross_entropy_on_cpu():
    torch.manual_seed(3)
    lit = _tiny_img()
    x = torch.randn(6, 28, 28, 1)
    a = torch.randint(0, 10, (6,))
    b = a.flip(0)
    lam = torch.rand(6)
    logits = lit.model(x).float()
    # hard labels with smoothing = nn.CrossEntropyLoss(label_smoothing)
    loss, pred = lit.model.soft_loss(x, a, label_smoothing=0.1)
    assert torch.allclose(loss, F.cross_entropy(logits, a, label_smoothing=0.1), rtol=1e-5, atol=1e-6)
    assert torch.equal(pred, logits.argmax(-1))
    # a label pair
    loss, _ = lit.model.soft_loss(x, a, b, lam, label_smoothing=0.1)
    t = 0.9 * (lam[:, None] * F.one_hot(a, 10) + (1 - lam[:, None]) * F.one_hot(b, 10)) + 0.01
    assert torch.allclose(loss, F.cross_entropy(logits, t), rtol=1e-5, atol=1e-6)
    # options off: the step is the hard-label step
    assert not lit.soft_targets
    l0, _ = lit.step((x, a))
    assert torch.allclose(l0, F.cross_entropy(logits, a), rtol=1e-6)


def _run_cli(task, tmp_path, *flags):
    from perceiver_io_amd.cli.tasks import main as cli_main

    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        return cli_main(task, list(flags))
    finally:
        os.chdir(old)


def test_cli_fit_with_mixing_and_smoothing(tmp_path, monkeypatch):
    """4 CPU steps of the smallest MNIST-shape classifier with MixUp, CutMix and label smoothing on:
    the flags land in the checkpoint's hyper-parameters, the metrics are sane, and validation
    never mixes."""
    from perceiver_io_amd import ops
    from perceiver_io_amd.train.checkpoint import load_checkpoint

    calls = {"train": 0, "eval": 0}
    real = ops.batch_mix
    holder = {}

    def counted(x, y, mix):
        lit = holder.get("lit")
        calls["train" if lit is None or lit.training else "eval"] += 1
        return real(x, y, mix)

    monkeypatch.setattr(ops, "batch_mix", counted)
    from perceiver_io_amd.tasks import LitImageClassifier

    init = LitImageClassifier.__init__

    def spy(self, *a, **k):
        holder["lit"] = self
        init(self, *a, **k)

    monkeypatch.setattr(LitImageClassifier, "__init__", spy)
    cli = _run_cli("img_clf", tmp_path, "fit", "--data=MNISTDataModule", "--data.synthetic=true",
                   "--data.synthetic_size=48", "--data.batch_size=8", "--data.num_workers=0", "--data.val_split=16",
                   "--optimizer.lr=0.001", "--trainer.accelerator=cpu", "--trainer.max_epochs=1",
                   "--trainer.limit_train_batches=4", "--trainer.limit_val_batches=2", "--trainer.log_every_n_steps=1",
                   "--trainer.num_sanity_val_steps=1", "--trainer.seed=5",
                   "--model.num_latents=8", "--model.num_latent_channels=64", "--model.num_encoder_layers=1",
                   "--model.num_encoder_self_attention_layers_per_block=1", "--model.num_frequency_bands=4",
                   "--model.label_smoothing=0.1", "--model.mixup_alpha=0.8", "--model.cutmix_alpha=1.0")
    tr = cli.trainer
    assert tr.global_step == 4
    m = tr.callback_metrics
    assert math.isfinite(m["train_loss"]) and 0.0 <= m["train_acc"] <= 1.0
    assert math.isfinite(m["val_loss"]) and 0.0 <= m["val_acc"] <= 1.0
    assert calls == {"train": 4, "eval": 0}, calls  # one mix per training micro-batch, none in validation
    ck = [c for c in tr.callbacks if type(c).__name__ == "ModelCheckpoint"][0]
    hp = load_checkpoint(ck.best_model_path)["hyper_parameters"]
    assert hp["label_smoothing"] == 0.1 and hp["mixup_alpha"] == 0.8 and hp["cutmix_alpha"] == 1.0
    assert hp["mix_prob"] == 1.0 and hp["mix_switch_prob"] == 0.5
    # a validation run of the trained module: the soft head with hard labels, no mixing
    before = dict(calls)
    res = tr.validate(cli.model, datamodule=cli.datamodule, verbose=False)[0]
    assert calls == before and math.isfinite(res["val_loss"])
