"""Soft-target classifier head and batch mixing on the GPU: the HIP kernels against their
emulation, launch-to-launch bit equality, consistency with the hard-label head, the model's
soft_loss against eager fp32, and a replayed step graph reading the staged mix words."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [(5, 3, 64),      # V < one class tile, M < one row tile
         (33, 10, 128),   # one row past a 32-row tile
         (130, 257, 64),  # one class past a tile multiple, more than 4 row tiles
         (64, 1000, 128),  # the ImageNet head
         (7, 1024, 64)]   # the largest V


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


def _emu():
    from perceiver_io_amd.ops import emulation

    return emulation


def bf(x):
    return x.to(torch.bfloat16)


def rel_fro(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@functools.lru_cache(maxsize=None)
def _case(M, V, C):
    """bf16-exact rows, the bf16 weight, labels with b == a rows and every 7th row unlabelled, and
    the three λ patterns (shared, never modified)"""
    g = torch.Generator(device=DEV).manual_seed(1000 * M + V)
    h = bf(torch.randn(M, C, device=DEV, generator=g)).float()
    w = bf(torch.randn(V, C, device=DEV, generator=g) * 0.3)
    bias = torch.randn(V, device=DEV, generator=g) * 0.1
    a = torch.randint(0, V, (M,), device=DEV, generator=g)
    b = torch.randint(0, V, (M,), device=DEV, generator=g)
    b[::5] = a[::5]
    a[::7] = -100
    lams = {"zero": torch.zeros(M, device=DEV), "one": torch.ones(M, device=DEV),
            "random": torch.rand(M, device=DEV, generator=g)}
    ref = h @ w.float().t() + bias
    return h, w, bias, a, b, lams, ref


def _run_head(K, h, w, bias, a, b, lam, eps, gout):
    M, C = h.shape
    V = w.shape[0]
    loss, lse, pred, hs, cnt = K.soft_ce_fwd(h, a, b, lam, w, bias, eps)
    dH = torch.full((M, C), 5.0, device=DEV)
    dW, db = torch.full((V, C), 7.0, device=DEV), torch.full((V,), 7.0, device=DEV)  # overwritten
    K.soft_ce_bwd(hs, a, b, lam, w, bias, eps, lse, gout, cnt, dH, dW, db, False)
    dW2, db2 = torch.full((V, C), 0.5, device=DEV), torch.full((V,), -0.25, device=DEV)  # added to
    K.soft_ce_bwd(hs, a, b, lam, w, bias, eps, lse, gout, cnt, torch.empty_like(dH), dW2, db2, True)
    return dict(loss=loss, lse=lse, pred=pred, hs=hs, cnt=cnt, dH=dH, dW=dW, db=db, dW_acc=dW2, db_acc=db2)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("M,V,C", CASES)
def test_soft_ce_matches_emulation(M, V, C, eps):
    h, w, bias, a, b, lams, ref = _case(M, V, C)
    gout = torch.tensor([0.37], device=DEV)
    for kind, lam in lams.items():
        e = _run_head(_emu(), h, w, bias, a, b, lam, eps, gout)
        runs = [_run_head(_ext(), h, w, bias, a, b, lam, eps, gout) for _ in range(3)]
        k = runs[0]
        for r in runs[1:]:  # no atomics: every launch gives the same bits
            assert all(torch.equal(k[n], r[n]) for n in k), kind
        errs = {n: rel_fro(k[n], e[n]) for n in ("loss", "lse", "dH", "dW", "db", "dW_acc", "db_acc")}
        print(kind, errs)
        assert errs["loss"] < 1e-3 and errs["lse"] < 1e-3, (kind, errs)
        assert all(errs[n] < 1e-2 for n in ("dH", "dW", "db", "dW_acc", "db_acc")), (kind, errs)
        assert torch.equal(k["hs"], e["hs"]) and k["cnt"].item() == e["cnt"].item() == float((a >= 0).sum())
        assert torch.equal(k["dH"][::7], torch.zeros_like(k["dH"][::7]))  # rows without a label
        # pred: the reference logit at pred is the row's maximum to 1e-4 of the logits' scale
        # (fp32 accumulation-order error over C ≤ 128 bf16-exact products); every row, unlabelled too
        pred = k["pred"].long()
        assert k["pred"].dtype == torch.int32 and (pred >= 0).all() and (pred < V).all()
        gap = (ref.max(-1).values - ref.gather(1, pred[:, None])[:, 0]).abs().max().item()
        assert gap <= 1e-4 * ref.abs().max().item(), (kind, gap)


@pytest.mark.parametrize("M,V,C", [CASES[0], CASES[3]])
def test_soft_ce_all_rows_unlabelled(M, V, C):
    h, w, bias, _, b, lams, _ = _case(M, V, C)
    a = torch.full((M,), -100, device=DEV)
    k = _run_head(_ext(), h, w, bias, a, b, lams["random"], 0.1, torch.ones(1, device=DEV))
    assert k["loss"].item() == 0.0 and k["cnt"].item() == 0.0
    assert all(torch.equal(k[n], torch.zeros_like(k[n])) for n in ("dH", "dW", "db"))
    assert torch.isfinite(k["lse"]).all()


@pytest.mark.parametrize("lo,hi", [(17, 33), (3, 7), (2, 3), (5, 133), (0, 1023)])
def test_soft_ce_pred_tie_rule(lo, hi):
    """h = 0: the logits are the bias, two exactly equal maxima → the lower class.  The pairs sit
    in the tiles of two different waves, in the two lane halves of one tile, in one lane, in two
    tiles of one wave (0 and 4), and at the first and last class."""
    V, C, M = 1024, 64, 3
    w = bf(torch.randn(V, C, device=DEV))
    bias = torch.zeros(V, device=DEV)
    bias[lo] = bias[hi] = 2.5
    a = torch.zeros(M, dtype=torch.int64, device=DEV)
    pred = _ext().soft_ce_fwd(torch.zeros(M, C, device=DEV), a, a, torch.ones(M, device=DEV), w, bias, 0.0)[2]
    assert pred.tolist() == [lo] * M


@pytest.mark.parametrize("M,V,C", [CASES[1], CASES[2], CASES[3]])
def test_soft_ce_consistent_with_hard_label_head(M, V, C):
    """ε = 0, λ = 1: the loss and the gradients of ce_fwd / ce_bwd on the same rows"""
    h, w, bias, a, b, lams, _ = _case(M, V, C)
    gout = torch.tensor([0.37], device=DEV)
    k = _run_head(_ext(), h, w, bias, a, b, lams["one"], 0.0, gout)
    cnt = torch.empty(1, device=DEV)
    dh = torch.empty(M, C, device=DEV)
    o = _ext().ce_fwd(h, None, a, w, bias, cnt, dh, True)
    loss, lse, hs = o[:3]
    u = dict(u=o[3], u_ml=o[4]) if len(o) > 4 else {}
    dW, db = torch.zeros(V, C, device=DEV), torch.zeros(V, device=DEV)
    _ext().ce_bwd(hs, a, w, bias, lse, gout, cnt, dh, dW, db, False, None, **u)
    errs = dict(loss=rel_fro(k["loss"], loss), lse=rel_fro(k["lse"], lse), dH=rel_fro(k["dH"], dh),
                dW=rel_fro(k["dW"], dW), db=rel_fro(k["db"], db))
    print(errs)
    assert errs["loss"] < 1e-3 and errs["lse"] < 1e-3 and all(errs[n] < 1e-2 for n in ("dH", "dW", "db")), errs


def _words(mode, lam=1.0, box=(0, 0, 0, 0)):
    return torch.tensor([float(mode), lam, *map(float, box)], dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("B", [1, 4, 5])
@pytest.mark.parametrize("shape", [(8, 8, 1), (6, 10, 3), (5, 7, 3)])  # 5·7·3: the one-element-per-thread path
def test_batch_mix_matches_emulation(B, shape):
    H, W, _ = shape
    g = torch.Generator(device=DEV).manual_seed(B)
    x = torch.randn(B, *shape, device=DEV, generator=g).clamp(-1, 1)
    y = torch.randint(0, 10, (B,), device=DEV, generator=g)
    x0 = x.clone()
    for mix in (_words(0, 0.4, (1, 3, 2, 5)), _words(2, 0.8, (2, H, 0, 3)), _words(2, 1.0), _words(1, 0.3)):
        out, yb, lam = _ext().batch_mix(x, y, mix)
        eo, eyb, elam = _emu().batch_mix(x, y, mix)
        assert torch.equal(yb, eyb) and torch.equal(lam, elam)
        if int(mix[0]) == 1:  # the kernel may contract the multiply-add
            assert (out - eo).abs().max().item() <= 1e-6
            if B % 2:
                assert torch.equal(out[B // 2], x[B // 2])
        else:
            assert torch.equal(out, eo)
        assert torch.equal(x, x0) and out.data_ptr() != x.data_ptr()


def _img_lit(**kw):
    from perceiver_io_amd.tasks import LitImageClassifier

    return LitImageClassifier(image_shape=(28, 28, 1), num_classes=10,
                              optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3}},
                              num_latents=32, num_latent_channels=128, num_encoder_layers=2,
                              num_encoder_self_attention_layers_per_block=2, num_decoder_cross_attention_heads=1,
                              **kw).cuda()


@pytest.mark.parametrize("mode", ["mixup", "cutmix"])
def test_model_soft_loss_fused_matches_eager(mode):
    """PerceiverIO.soft_loss on a mixed batch with ε = 0.1: fused bf16 path vs eager fp32 and vs
    the emulation, loss to 1e-2 and every gradient tensor to 2e-2 (the tolerances of the
    hard-label classifier checks)."""
    from test_model_gpu import _three_way

    from perceiver_io_amd import ops

    torch.manual_seed(4)
    lit = _img_lit()
    x = torch.randn(6, 28, 28, 1, device=DEV)
    y = torch.randint(0, 10, (6,), device=DEV)
    mix = _words(1, 0.35) if mode == "mixup" else _words(2, 1.0 - 8 * 12 / 784.0, (5, 13, 10, 22))

    def run(xx=x):
        xm, yb, lam = ops.batch_mix(xx, y, mix)
        loss, pred = lit.model.soft_loss(xm, y, yb, lam, label_smoothing=0.1)
        assert pred.shape == (6,)
        loss.backward()
        return loss

    xj = x * (1 + 1e-6 * torch.randn_like(x))
    _three_way(lit, run, jitter_run=lambda: run(xj))


def test_graph_replay_reads_staged_mix_words():
    """A captured step with mixing on (lr = 0, weight decay = 0), replayed with two different
    staged mix tensors — mode 0, then a CutMix box — returns the losses the uncaptured fused path
    gives on those inputs."""
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops.optim import FusedAdamW
    from perceiver_io_amd.train.engine import StepEngine

    torch.manual_seed(6)
    lit = _img_lit(label_smoothing=0.1, mixup_alpha=0.8, cutmix_alpha=1.0)
    lit.train()
    with torch.no_grad():  # a freshly initialised head is near uniform: make the loss depend on the rows
        lit.model.decoder.output_adapter.linear.weight.normal_(0.0, 1.0)
    x = torch.randn(8, 28, 28, 1, device=DEV) * torch.arange(1, 9, device=DEV).view(8, 1, 1, 1)
    y = torch.randint(0, 10, (8,), device=DEV)
    mixes = [_words(0), _words(2, 1.0 - 10 * 14 / 784.0, (4, 14, 7, 21))]
    with ops.backend("hip"):
        with torch.no_grad():
            want = [lit.step((x, y, m))[0].item() for m in mixes]
        assert abs(want[0] - want[1]) > 1e-4 * abs(want[0])  # told apart at ten times the tolerance below
        opt = FusedAdamW(lit.parameters(), lr=0.0, weight_decay=0.0)
        eng = StepEngine(lambda b: lit.step(b)[0], opt, device=DEV, graph=True, warmup_eager=1)
        eng.step((x, y, _words(1, 0.5)))  # eager warm-up
        got = [eng.step((x, y, m)).item() for m in mixes]  # capture + replay, then a replay
        torch.cuda.synchronize()
    assert eng.num_graphs == 1 and eng.replays == 2
    print(want, got)
    assert all(abs(g - w) <= 1e-5 * abs(w) for g, w in zip(got, want)), (want, got)
    ops.check_device_errors()
