"""Focal cross-entropy + soft Dice on the GPU: the ``pixel_seg_fwd`` / ``pixel_seg_bwd`` kernels
(csrc/pixel_head.hip) against their emulation, and the loss through ``LArPerceiver`` on the fused
path, eagerly and inside a captured training step."""
import functools

import pytest
import torch

from perceiver_io_amd.data.lartpc import DenseCollator, sparse_collate
from perceiver_io_amd.data.synthetic import lartpc_event
from test_kernels_gpu import close
from test_seg_loss import saturated_operands

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (γ, ce_weight, dice_weight): today's loss through the new kernels, the common setting, and a
# general exponent with the cross-entropy term switched off
PARAMS = [(0.0, 1.0, 0.0), (2.0, 1.0, 0.5), (0.5, 0.0, 1.0)]
EPS = 1.0


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


def _emu():
    from perceiver_io_amd.ops import emulation

    return emulation


@functools.lru_cache(maxsize=None)
def _operands(R, C, K):
    """As ``test_pixel_ce_kernels`` builds them: every fifth label -100, weights[0] = 0."""
    torch.manual_seed(12)
    h = torch.randn(R, C, device=DEV)
    W = torch.randn(K, C, device=DEV) * 0.3
    b = torch.randn(K, device=DEV) * 0.1
    lab = torch.randint(0, K, (R,), device=DEV)
    lab[::5] = -100
    wts = torch.rand(K, device=DEV) + 0.5
    wts[0] = 0.0
    return h, W, b, lab, wts


def _backward(Kx, ops, params, stats, fill=1.0):
    h, W, b = ops[:3]
    K, C = W.shape
    d = torch.empty_like(h)
    dW, db = torch.full((K, C), fill, device=DEV), torch.full((K,), fill, device=DEV)  # accumulated onto
    Kx.pixel_seg_bwd(*ops, *params, torch.tensor([0.7], device=DEV), stats, d, dW, db)
    return d, dW, db


def _compare_forward(t1, l1, t2, l2, K):
    n, ns = 4 + 2 * K, 4 + 5 * K
    assert t1.shape == t2.shape == (6 + 7 * K,)
    close(t1[:2], t2[:2], 1e-4, "loss sums")
    assert torch.equal(t1[2:n], t2[2:n]), (t1[2:n], t2[2:n])  # counts / hits exact
    close(t1[n:n + 2 * K], t2[n:n + 2 * K], 1e-4, "I_c, P_c")
    assert torch.equal(t1[n + 2 * K:ns], t2[n + 2 * K:ns])  # T_c exact
    close(t1[ns:ns + K], t2[ns:ns + K], 1e-6, "accuracies")
    close(t1[ns + K:], t2[ns + K:], 1e-4, "F, D, per-class dice")
    close(l1, l2, 1e-4, "loss")


# 17: one partial block; 333 × 32: the float2 row path; 1000 × 128 × 4: the 24-column finalize;
# 8209: more than 512 blocks × 16 rows, so the grid-stride row loop takes a second trip
@pytest.mark.parametrize("gamma,cew,dcw", PARAMS)
@pytest.mark.parametrize("R,C,K", [(17, 64, 3), (333, 32, 2), (1000, 128, 4), (8209, 64, 3)])
def test_pixel_seg_kernels(R, C, K, gamma, cew, dcw):
    ops = _operands(R, C, K)
    params = (gamma, cew, dcw, EPS)
    (t1, l1), (t2, l2) = _ext().pixel_seg_fwd(*ops, *params), _emu().pixel_seg_fwd(*ops, *params)
    print(f"pixel_seg {R, C, K} {params}: loss {l1.item():.6f} vs {l2.item():.6f}, "
          f"stats max err {(t1 - t2).abs().max().item():.3e}")
    _compare_forward(t1, l1, t2, l2, K)
    got, want = _backward(_ext(), ops, params, t2), _backward(_emu(), ops, params, t2)
    for a, c, n in zip(got, want, ("dH", "dW", "db")):
        print(f"  {n}: max err {(a - c).abs().max().item():.3e} of {c.abs().max().item():.3e}")
        close(a, c, 1e-4, n)
    # onto zeros the same bound is relative to the gradients themselves, not to the ones
    for a, c, n in zip(_backward(_ext(), ops, params, t2, 0.0), _backward(_emu(), ops, params, t2, 0.0), ("dH", "dW", "db")):
        close(a, c, 1e-4, n + " onto 0")
    # fixed-order sums, no atomics: a second identical call is bitwise equal
    t3, l3 = _ext().pixel_seg_fwd(*ops, *params)
    assert torch.equal(t1, t3) and torch.equal(l1, l3)
    for a, c in zip(got, _backward(_ext(), ops, params, t2)):
        assert torch.equal(a, c)


def test_gamma0_without_dice_repeats_pixel_ce_sums():
    """γ = 0 does not touch q and a weight-0 term is not evaluated: the columns shared with
    ``pixel_ce_fwd`` hold the same sums (same row arithmetic, same summation order)."""
    ops = _operands(8209, 64, 3)
    t1, l1 = _ext().pixel_seg_fwd(*ops, 0.0, 1.0, 0.0, EPS)
    t0, l0 = _ext().pixel_ce_fwd(*ops)
    assert torch.equal(t1[1:10], t0[1:10])  # Σw, counts, hits
    close(t1[:1], t0[:1], 1e-6, "Σ w·ce")
    close(l1, l0, 1e-6, "loss")
    assert float(t1[10:19].abs().max()) == 0.0  # I_c, P_c, T_c are not evaluated


@pytest.mark.parametrize("gamma,cew,dcw", PARAMS[1:])
def test_empty_input_returns_the_finalize_values(gamma, cew, dcw):
    K, C = 3, 64
    h, W, b, lab, wts = _operands(17, C, K)
    ops = (h[:0].contiguous(), W, b, lab[:0].contiguous(), wts)
    params = (gamma, cew, dcw, EPS)
    (t1, l1), (t2, l2) = _ext().pixel_seg_fwd(*ops, *params), _emu().pixel_seg_fwd(*ops, *params)
    _compare_forward(t1, l1, t2, l2, K)  # identical NaN pattern: F = 0 / 0 where it is evaluated
    assert float(t1[:4 + 5 * K].abs().max()) == 0.0
    assert float(t1[4 + 6 * K + 1]) == 0.0  # D: every coefficient is ε / ε
    d, dW, db = _backward(_ext(), ops, params, t2)
    assert d.shape == (0, C) and torch.equal(dW, torch.ones_like(dW)) and torch.equal(db, torch.ones_like(db))


@pytest.mark.parametrize("gamma", [0.5, 2.0])
def test_saturated_row_on_the_device(gamma):
    ops = tuple(t.to(DEV) for t in saturated_operands())
    for dcw in (0.0, 0.5):
        params = (gamma, 1.0, dcw, EPS)
        (t1, l1), (t2, l2) = _ext().pixel_seg_fwd(*ops, *params), _emu().pixel_seg_fwd(*ops, *params)
        _compare_forward(t1, l1, t2, l2, 3)
        got, want = _backward(_ext(), ops, params, t2), _backward(_emu(), ops, params, t2)
        for a, c, n in zip(got, want, ("dH", "dW", "db")):
            assert torch.isfinite(a).all(), n
            close(a, c, 1e-4, n)
        assert torch.isfinite(t1).all() and torch.isfinite(l1)
        if dcw == 0.0:
            assert float(got[0][0].abs().max()) == 0.0  # q = 0: no focal gradient on that row


def test_invalid_parameter_raises_on_the_host():
    ops = _operands(17, 64, 3)
    for params in ((-0.5, 1.0, 0.0, 1.0), (2.0, 0.0, 0.0, 1.0), (2.0, 1.0, -0.1, 1.0), (2.0, 1.0, 0.5, 0.0)):
        with pytest.raises(RuntimeError):
            _ext().pixel_seg_fwd(*ops, *params)


def _lartpc(seed):
    from perceiver_io_amd.models.lartpc import LArPerceiver

    torch.manual_seed(seed)
    return LArPerceiver(64).to(DEV)


def test_sparse_seg_loss_fused_matches_eager():
    """``sparse_loss(loss=SegLoss(...))`` on the fused kernels against eager fp32 and against the
    kernels' emulation: the value and the head's gradients, at the tolerances of
    ``test_model_gpu`` (kernel vs emulation at 2 %, and vs fp32 with the emulation's own bf16 error
    added: the decoder output that feeds the head went through bf16 kernels)."""
    from perceiver_io_amd import ops
    from perceiver_io_amd.models.lartpc import SegLoss, class_weights
    from test_model_gpu import _check_grads, _emulated, _rel

    model = _lartpc(4)
    batch = tuple(t.to(DEV) for t in sparse_collate([lartpc_event(i, 64) for i in range(3)], bucket=256))
    w = class_weights(DEV, (0.0, 1.0, 2.0))
    cfg = SegLoss(2.0, 1.0, 0.5, 1.0)
    head = model.perceiver.decoder.output_adapter.linear
    res = {}
    for name in ("torch", "hip", "emu"):
        model.zero_grad()
        if name == "emu":
            with ops.backend("hip"), _emulated():
                loss, metrics = model.sparse_loss(batch, w, loss=cfg)
                loss.backward()
        else:
            with ops.backend(name):
                loss, metrics = model.sparse_loss(batch, w, loss=cfg)
                loss.backward()
        res[name] = (loss.item(), {"weight": head.weight.grad.clone(), "bias": head.bias.grad.clone()},
                     {k: float(v) for k, v in metrics.items()})
    (l0, g0, m0), (l1, g1, m1), (l2, g2, _) = res["torch"], res["hip"], res["emu"]
    print(f"seg loss eager {l0:.6f} fused {l1:.6f} emulated {l2:.6f}; metrics {m1}")
    assert abs(l1 - l0) < 1e-2 * abs(l0), (l0, l1)
    assert abs(l1 - l2) < 1e-3 * abs(l2), (l1, l2)
    assert sorted(m1) == sorted(m0) == ["acc", "acc1", "acc2", "dice", "dice1", "dice2", "focal"]
    assert abs(cfg.ce_weight * m1["focal"] + cfg.dice_weight * m1["dice"] - l1) < 1e-5 * abs(l1)
    floor = {n: _rel(g2[n], g) for n, g in g0.items()}
    _check_grads(g1, g2, floor=floor)
    _check_grads(g1, g0, floor=floor)


def test_event_loss_with_seg_loss_under_graph_capture():
    """One captured and replayed training step over ``event_loss(loss=SegLoss(...))`` gives the loss of
    the eager fused call on the same events and parameters.  The two run the same forward kernels
    on the same operands, so only an order of fp32 additions may differ: 1e-5 relative."""
    from perceiver_io_amd import ops
    from perceiver_io_amd.models.lartpc import SegLoss, class_weights
    from perceiver_io_amd.ops.optim import FusedAdam
    from perceiver_io_amd.train.engine import StepEngine

    events = [lartpc_event(90 + i, 64) for i in range(3)]
    shapes = sparse_collate(events, bucket=256)
    kcap, qcap = shapes[0].shape[1], shapes[3].shape[1]
    img, lab = DenseCollator()(events)
    batch = (img.to(DEV), lab.to(DEV), torch.tensor([0, 5, 3], dtype=torch.int32, device=DEV))
    w = class_weights(DEV)
    cfg = SegLoss(2.0, 1.0, 0.5, 1.0)
    model = _lartpc(6)
    with ops.backend("hip"), torch.no_grad():
        eager, metrics, _ = model.event_loss(batch, w, kcap, qcap, loss=cfg)
        plain = model.event_loss(batch, w, kcap, qcap)[0]
    assert float(eager) != float(plain)  # the configuration reaches the head
    opt = FusedAdam(model.trained_parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=10.0)
    eng = StepEngine(lambda b: model.event_loss(b, w, kcap, qcap, loss=cfg)[0], opt, device=DEV, graph=True,
                     warmup_eager=0)
    first = float(eng.step(batch))
    second = float(eng.step(batch))
    print(f"event_loss eager {float(eager):.6f}, captured step {first:.6f}, next step {second:.6f}")
    assert eng.num_graphs == 1 and eng.captures == 1 and eng.replays == 2
    assert abs(first - float(eager)) <= 1e-5 * abs(float(eager)), (first, float(eager))
    assert second == second and second != first  # the update happened and the replay recomputed the loss
