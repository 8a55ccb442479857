"""LArTPC sparse inference (``LArPerceiver.segment`` / ``segment_sparse``, ``ops.pixel_head.
pixel_predict``, the ``pixel_predict`` / ``nonzero_compact`` emulations, ``iou`` and ``run.py
--segment``) on the CPU, against the dense model and ``sparse_collate``."""
import os

import numpy as np
import pytest
import torch

from perceiver_io_amd.data.lartpc import sparse_collate
from perceiver_io_amd.data.synthetic import SyntheticLArTPC, lartpc_event
from perceiver_io_amd.models.lartpc import LArPerceiver, Segmentation, iou
from perceiver_io_amd.ops import emulation

SIZE = 32


def _model(size=SIZE, seed=1):
    """Random init gives every pixel the same class: a random output-query table and head weight
    (generator 7) spread the lit pixels over all three classes."""
    torch.manual_seed(seed)
    model = LArPerceiver(size).eval()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        out = model.decoder.output
        out.copy_(torch.randn(out.shape, generator=g))
        w = model.decoder.output_adapter.linear.weight
        w.copy_(0.5 * torch.randn(w.shape, generator=g))
    return model


@pytest.fixture(scope="module")
def case():
    model = _model()
    ev = [lartpc_event(10 + i, SIZE) for i in range(2)]
    img = torch.stack([e[0] for e in ev])
    lab = torch.stack([e[1] for e in ev])
    with torch.no_grad():
        dense = model(img)  # (B, 3, npix)
    return model, ev, img, lab, dense


def test_segment_matches_dense_argmax_at_lit_pixels(case):
    model, ev, img, lab, dense = case
    seg = model.segment(img)
    assert isinstance(seg, Segmentation)
    lit = img.reshape(2, -1) != 0
    want = torch.where(lit, dense.argmax(1), torch.zeros(1, dtype=torch.long)).to(torch.uint8)
    assert seg.class_map.dtype == torch.uint8 and seg.class_map.shape == (2, SIZE * SIZE)
    assert torch.equal(seg.class_map, want)
    assert set(seg.class_map[lit].tolist()) == {0, 1, 2}
    assert torch.equal(seg.count, lit.sum(1).to(torch.int32))
    assert seg.confusion is None
    # (B, H·W) input and an explicit capacity give the same answer
    seg2 = model.segment(img.reshape(2, -1), capacity=int(seg.count.max()))
    assert torch.equal(seg2.class_map, seg.class_map) and torch.equal(seg2.count, seg.count)


def test_segment_classes_and_confidence_match_softmax_of_sparse_logits(case):
    model, ev, img, lab, dense = case
    seg = model.segment(img, labels=lab)
    values, index, kmask = sparse_collate(ev)[:3]
    with torch.no_grad():
        p = torch.softmax(model.sparse_logits(values, index, kmask, index), -1)
    valid = ~kmask
    assert seg.classes.shape == index.shape and seg.confidence.shape == index.shape
    assert torch.allclose(seg.confidence[valid], p.max(-1).values[valid], atol=1e-5)
    chosen = p.gather(2, seg.classes.long()[..., None])[..., 0]
    assert torch.allclose(chosen[valid], p.max(-1).values[valid], atol=1e-5)
    assert (seg.classes[kmask] == 0).all() and (seg.confidence[kmask] == 0).all()
    # dense labels are gathered at the lit pixels
    ql = lab.gather(1, index)[valid]
    want = torch.bincount(ql * 3 + seg.classes.long()[valid], minlength=9).view(3, 3)
    assert seg.confusion.dtype == torch.int64 and torch.equal(seg.confusion, want)


def test_segment_sparse_on_collated_input(case):
    model, ev, img, lab, dense = case
    seg = model.segment(img)
    values, index, kmask, qidx, qlab = sparse_collate(ev)
    sp = model.segment_sparse(values, index, kmask)
    for a, b in zip(sp, seg):
        assert (a is None and b is None) or torch.equal(a, b)
    # an explicit, strictly smaller query set: only those pixels reach the map
    n = int((~kmask).sum(1).min())
    sub = index[:, 0:n:2].contiguous()
    qmask = torch.zeros_like(sub, dtype=torch.bool)
    qmask[:, -3:] = True  # and three padding slots among them
    part = model.segment_sparse(values, index, kmask, qidx=sub, qmask=qmask)
    want = torch.zeros_like(seg.class_map)
    for i in range(2):
        keep = sub[i][~qmask[i]]
        want[i, keep] = seg.class_map[i, keep]
    assert torch.equal(part.class_map, want)
    assert int((part.class_map != 0).sum()) < int((seg.class_map != 0).sum())
    assert (part.classes[qmask] == 0).all() and (part.confidence[qmask] == 0).all()


def test_emulation_pixel_predict_tie_invalid_and_out_of_range():
    C, K, Q, npix = 32, 3, 4, 10
    h = torch.zeros(2 * Q, C)
    h[:, 0] = 1.0
    w = torch.zeros(K, C)
    b = torch.zeros(K)
    # the logits of every row are w[:, 0]: classes 1 and 2 tie exactly
    w[:, 0] = torch.tensor([0.0, 2.0, 2.0])
    qidx = torch.tensor([3, 5, -1, 10, 0, 1, 2, 9])
    valid = torch.tensor([True, False, True, True, True, True, False, True])
    classes, conf, cmap = emulation.pixel_predict(h, w, b, qidx, valid, Q, npix)
    assert classes.dtype == torch.uint8 and cmap.dtype == torch.uint8 and cmap.shape == (2, npix)
    assert classes.tolist() == [1, 0, 1, 1, 1, 1, 0, 1]  # the lowest tied class; 0 on invalid rows
    p = 1.0 / (2.0 + float(torch.exp(torch.tensor(-2.0))))
    assert torch.allclose(conf, torch.tensor([p, 0, p, p, p, p, 0, p]), atol=1e-6)
    want = torch.zeros(2, npix, dtype=torch.uint8)
    want[0, 3] = 1  # row 1 invalid; rows 2 and 3 out of range: skipped, classes / conf kept
    want[1, 0] = want[1, 1] = want[1, 9] = 1
    assert torch.equal(cmap, want)
    w[:, 0] = 0.0  # every class ties: class 0, confidence 1/3
    classes, conf, cmap = emulation.pixel_predict(h, w, b, qidx, valid, Q, npix)
    assert (classes == 0).all() and torch.allclose(conf[valid], torch.full((6,), 1 / 3))


def test_emulation_pixel_predict_confusion_is_bincount():
    torch.manual_seed(4)
    B, Q, C, K, npix = 2, 25, 64, 3, 40
    h, w, b = torch.randn(B * Q, C), torch.randn(K, C) * 0.2, torch.randn(K) * 0.1
    qidx = torch.cat([torch.randperm(npix)[:Q] for _ in range(B)])
    valid = torch.ones(B * Q, dtype=torch.bool)
    valid[::7] = False
    lab = torch.randint(0, K, (B * Q,))
    lab[::5] = -100
    classes, conf, cmap, part = emulation.pixel_predict(h, w, b, qidx, valid, Q, npix, lab)
    pred = (h @ w.t() + b).argmax(-1)
    assert torch.equal(classes[valid].long(), pred[valid])
    ok = valid & (lab != -100)
    want = torch.bincount(lab[ok] * K + pred[ok], minlength=K * K)
    assert part.dtype == torch.int32 and torch.equal(part.sum(0).long(), want)
    assert int(want.sum()) == int(ok.sum())
    rows = torch.arange(B * Q) // Q
    assert torch.equal(cmap[rows[valid], qidx[valid]], classes[valid])
    assert int((cmap != 0).sum()) == int((classes[valid] != 0).sum())


def test_emulation_nonzero_compact_equals_sparse_collate():
    ev = [lartpc_event(20 + i, SIZE) for i in range(3)]
    values, index, kmask = sparse_collate(ev, bucket=64)[:3]
    img = torch.stack([e[0] for e in ev]).reshape(3, -1)
    v, i, m, count = emulation.nonzero_compact(img, values.shape[1])
    assert v.dtype == values.dtype and i.dtype == index.dtype and m.dtype == kmask.dtype
    assert torch.equal(v, values) and torch.equal(i, index) and torch.equal(m, kmask)
    assert count.dtype == torch.int32 and torch.equal(count.long(), (img != 0).sum(1))


def test_emulation_nonzero_compact_edge_cases():
    img = torch.zeros(2, 50)
    img[1, 7], img[1, 9], img[1, 30] = -0.0, float("nan"), 2.5
    v, i, m, count = emulation.nonzero_compact(img, 4)
    assert count.tolist() == [0, 2] and m[0].all()  # all-zero sample; -0.0 is zero, NaN is not
    assert (v[0] == 0).all() and (i[0] == 0).all()
    assert i[1].tolist() == [9, 30, 0, 0] and m[1].tolist() == [False, False, True, True]
    assert torch.isnan(v[1, 0, 0]) and v[1, 1:, 0].tolist() == [2.5, 0.0, 0.0]
    # overflow: the true count, the first cap pixels in order
    g = torch.Generator().manual_seed(0)
    img = torch.zeros(1, 1024)
    where = torch.randperm(1024, generator=g)[:700].sort().values
    img[0, where] = torch.rand(700, generator=g) + 0.5
    v, i, m, count = emulation.nonzero_compact(img, 512)
    assert count.tolist() == [700] and not m.any()
    assert torch.equal(i[0], where[:512]) and torch.equal(v[0, :, 0], img[0, where[:512]])
    assert emulation.nonzero_compact(img, 0)[3].tolist() == [700]  # counting pass


def test_iou_hand_written():
    conf = torch.tensor([[0, 0, 0], [0, 6, 2], [0, 1, 3]])  # class 0 in neither labels nor predictions
    per, mean = iou(conf)
    assert torch.isnan(per[0])
    assert float(per[1]) == pytest.approx(6 / 9) and float(per[2]) == pytest.approx(3 / 6)
    assert float(mean) == pytest.approx((6 / 9 + 3 / 6) / 2)
    per, mean = iou(torch.tensor([[5, 0, 0], [1, 0, 0], [0, 0, 4]]))  # labelled 1, never predicted: IoU 0
    assert per.tolist() == pytest.approx([5 / 6, 0.0, 1.0]) and float(mean) == pytest.approx((5 / 6 + 1) / 3)


def test_run_segment_writes_class_maps(tmp_path, capsys):
    import run

    ck, out = tmp_path / "ckpt", tmp_path / "maps"
    common = ["--val-events", "3", "--size", str(SIZE), "--batch-size", "2", "--device", "cpu"]
    run.main(["--epochs", "1", "--events", "2", "--max-steps", "1", "--log-dir", str(tmp_path / "runs"),
              "--ckpt-dir", str(ck), *common])
    capsys.readouterr()
    run.main(["--segment", str(ck / "model_0.ckpt"), "--out", str(out), "--ckpt-dir", str(tmp_path / "unused"), *common])
    assert "IoU" in capsys.readouterr().out
    assert sorted(os.listdir(out)) == [f"event_{i}.npy" for i in range(3)]
    assert not (tmp_path / "unused").exists()  # no training, no checkpoint
    data = SyntheticLArTPC(3, SIZE, seed=1)
    for i in range(3):
        m = np.load(out / f"event_{i}.npy")
        assert m.shape == (SIZE, SIZE) and m.dtype == np.uint8
        assert (m[data[i][0].numpy() == 0] == 0).all() and m.max() <= 2
