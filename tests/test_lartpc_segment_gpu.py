"""LArTPC sparse inference on the GPU: the ``pixel_predict`` and ``nonzero_compact`` kernels
(``csrc/pixel_head.hip``) against their emulations / ``sparse_collate``, and
``LArPerceiver.segment`` on the fused backend against the eager fp32 model."""
import pytest
import torch

from perceiver_io_amd.data.lartpc import sparse_collate
from perceiver_io_amd.data.synthetic import lartpc_event

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


def _emu():
    from perceiver_io_amd.ops import emulation

    return emulation


# ---- pixel_predict ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,Q,C,K", [
    (1, 1, 64, 3),       # a single row
    (1, 17, 64, 3),      # one row past a 16-row block iteration
    (3, 111, 32, 2),     # row -> sample mapping; map rows (npix odd) start at odd byte offsets
    (2, 4100, 128, 4),   # 8,200 rows > 512 blocks x 16 rows: the grid-stride loop runs twice
])
def test_pixel_predict_kernel(B, Q, C, K):
    torch.manual_seed(12)
    R, npix = B * Q, 2 * Q + 3
    h = torch.randn(R, C, device=DEV)
    W = torch.randn(K, C, device=DEV) * 0.3
    b = torch.randn(K, device=DEV) * 0.1
    lab = torch.randint(0, K, (R,), device=DEV)
    lab[::5] = -100
    valid = torch.ones(R, dtype=torch.bool, device=DEV)
    valid[3::7] = False
    qidx = torch.cat([torch.randperm(npix)[:Q] for _ in range(B)]).to(DEV)  # distinct per sample, in range
    classes, conf, cmap, part = _ext().pixel_predict(h, W, b, qidx, valid, Q, npix, lab)
    torch.cuda.synchronize()
    assert classes.dtype == torch.uint8 and classes.shape == (R,) and conf.shape == (R,)
    assert cmap.dtype == torch.uint8 and cmap.shape == (B, npix) and part.dtype == torch.int32
    e_classes, e_conf = _emu().pixel_predict(h, W, b, qidx, valid, Q, npix)[:2]
    # confidence: the 1e-4 relative bound of test_pixel_ce_kernels on the same logit arithmetic
    err = (conf - e_conf).abs().max().item()
    print(f"pixel_predict {B, Q, C, K}: conf max err {err:.3e}, classes differing from emulation "
          f"{int((classes != e_classes).sum())}")
    assert err <= 1e-4 * e_conf.max().item()
    assert ((conf - e_conf).double().norm() / e_conf.double().norm()).item() <= 1e-4
    assert (conf[~valid] == 0).all() and (classes[~valid] == 0).all()
    # classes: the fp32 reference logit at the returned class is the row maximum up to rounding
    z = _emu()._pixel_logits(h, W, b)
    got = z.gather(1, classes.long()[:, None])[:, 0]
    assert (classes < K).all()
    assert (got[valid] >= z.max(-1).values[valid] - 1e-4 * z.abs().max()).all()
    # the map is the scatter of the kernel's own classes; everything else stays 0
    rows = torch.arange(R, device=DEV) // Q
    want = torch.zeros(B, npix, dtype=torch.uint8, device=DEV)
    want[rows[valid], qidx[valid]] = classes[valid]
    assert torch.equal(cmap, want)
    # confusion: exact bincount of the kernel's own classes over valid, labelled rows
    ok = valid & (lab >= 0)
    cnt = torch.bincount(lab[ok] * K + classes[ok].long(), minlength=K * K)
    assert torch.equal(part.sum(0, dtype=torch.int64), cnt) and int(cnt.sum()) == int(ok.sum())
    # without labels: three outputs, the same values; and a second run is bitwise identical
    again = _ext().pixel_predict(h, W, b, qidx, valid, Q, npix, lab)
    for a, c in zip(again, (classes, conf, cmap, part)):
        assert torch.equal(a, c)
    nolab = _ext().pixel_predict(h, W, b, qidx, valid, Q, npix)
    assert len(nolab) == 3 and all(torch.equal(a, c) for a, c in zip(nolab, (classes, conf, cmap)))


# ---- nonzero_compact -------------------------------------------------------------------------
def _ref_compact(img, cap):
    """values / index / kmask / count from torch.nonzero per sample (CPU)."""
    B = img.shape[0]
    values, index = torch.zeros(B, cap, 1), torch.zeros(B, cap, dtype=torch.long)
    kmask, count = torch.ones(B, cap, dtype=torch.bool), torch.zeros(B, dtype=torch.int32)
    for i in range(B):
        nz = torch.nonzero(img[i] != 0).squeeze(1)
        n = min(len(nz), cap)
        values[i, :n, 0], index[i, :n], kmask[i, :n], count[i] = img[i, nz[:n]], nz[:n], False, len(nz)
    return values, index, kmask, count


def _same(a, b):
    """Bitwise: NaN payloads included."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# (segments per sample, loads per thread and tile): the default, one workgroup per sample, and
# an odd split with the larger tile
CONFIGS = [(0, 0), (1, 4), (7, 8)]


def _check_compact(img, cap, collated=None):
    ref = _ref_compact(img, cap)
    if collated is not None:  # the collator's own tensors at this capacity
        assert collated[0].shape[1] == cap
        assert all(_same(a, b) for a, b in zip(collated[:3], ref[:3]))
    dimg = img.to(DEV)
    for segs, tile in CONFIGS:
        out = _ext().nonzero_compact(dimg, cap, segs, tile)
        torch.cuda.synchronize()
        for name, a, b in zip(("values", "index", "kmask", "count"), out, ref):
            assert _same(a.cpu(), b), (name, segs, tile)
    assert _same(_ext().nonzero_compact(dimg, 0)[3].cpu(), ref[3])  # counting pass


def test_nonzero_compact_small_events():
    ev = [lartpc_event(20 + i, 32) for i in range(3)]
    _check_compact(torch.stack([e[0] for e in ev]).reshape(3, -1), 512, sparse_collate(ev, bucket=512))


def test_nonzero_compact_unaligned_rows():
    g = torch.Generator().manual_seed(3)
    img = torch.rand(2, 1089, generator=g)  # 33 x 33: rows not 16-byte aligned, tail not a multiple of 4
    img[torch.rand(2, 1089, generator=g) < 0.9] = 0
    img[0, 0], img[0, 1088], img[1, 1088] = 1.0, 2.0, 3.0
    _check_compact(img, 1152)


def test_nonzero_compact_real_shape():
    ev = [lartpc_event(30 + i, 512) for i in range(2)]
    _check_compact(torch.stack([e[0] for e in ev]).reshape(2, -1), 8192, sparse_collate(ev, bucket=8192))


def test_nonzero_compact_all_zero_sample():
    img = torch.stack([lartpc_event(20, 32)[0].reshape(-1), torch.zeros(1024), lartpc_event(21, 32)[0].reshape(-1)])
    _check_compact(img, 512)
    assert int(_ext().nonzero_compact(img.to(DEV), 512)[3][1]) == 0


def test_nonzero_compact_overflow():
    g = torch.Generator().manual_seed(0)
    img = torch.zeros(1, 1024)
    where = torch.randperm(1024, generator=g)[:700].sort().values
    img[0, where] = torch.rand(700, generator=g) + 0.5
    _check_compact(img, 512)
    v, i, m, count = _ext().nonzero_compact(img.to(DEV), 512)
    assert count.tolist() == [700] and torch.equal(i[0].cpu(), where[:512]) and not m.any()


def test_nonzero_compact_negative_zero_and_nan():
    img = torch.zeros(2, 1024)
    img[0, 5], img[0, 6], img[0, 700] = -0.0, float("nan"), 1.5
    img[1, 1023] = float("nan")
    _check_compact(img, 512)
    assert _ext().nonzero_compact(img.to(DEV), 512)[3].tolist() == [2, 1]


# ---- the model: fused segment against eager fp32 ---------------------------------------------
@pytest.fixture(scope="module")
def seg_case():
    from perceiver_io_amd import ops
    from perceiver_io_amd.models.lartpc import LArPerceiver

    torch.manual_seed(5)
    model = LArPerceiver(64).eval()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():  # spread the pixels over the three classes (random init predicts one)
        out = model.decoder.output
        out.copy_(torch.randn(out.shape, generator=g))
        w = model.decoder.output_adapter.linear.weight
        w.copy_(0.5 * torch.randn(w.shape, generator=g))
    model = model.cuda()
    ev = [lartpc_event(10 + i, 64) for i in range(2)]
    img = torch.stack([e[0] for e in ev]).cuda()
    lab = torch.stack([e[1] for e in ev]).cuda()
    coll = tuple(t.cuda() for t in sparse_collate(ev)[:3])
    with torch.no_grad(), ops.backend("torch"):
        eager = model.sparse_logits(*coll, coll[1]).float()  # (B, K, 3) fp32 logits at the lit pixels
    with ops.backend("hip"):
        seg = model.segment(img, labels=lab)
    torch.cuda.synchronize()
    return model, ev, img, lab, coll, eager, seg


def test_segment_fused_matches_eager(seg_case):
    model, ev, img, lab, coll, eager, seg = seg_case
    valid = ~coll[2]
    z = eager[valid]  # (n, 3)
    cls = seg.classes[valid].long()
    bound = 2e-2 * z.abs().max()  # what test_lartpc_dense_inference_fused_matches_eager allows these two paths
    top = z.topk(2, -1).values
    at = z.gather(1, cls[:, None])[:, 0]
    decided = (top[:, 0] - top[:, 1]) > bound
    share = decided.float().mean().item()
    rot = z.gather(1, ((cls + 1) % 3)[:, None])[:, 0]
    broken = (rot < top[:, 0] - bound).float().mean().item()
    print(f"segment vs eager: {len(z)} lit pixels, classes {torch.bincount(cls, minlength=3).tolist()}, decided "
          f"{share:.3f}, worst shortfall / bound {((top[:, 0] - at).max() / bound).item():.3f}, rotated broken {broken:.3f}")
    assert (at >= top[:, 0] - bound).all()
    assert share >= 0.90
    assert torch.equal(cls[decided], z.argmax(-1)[decided])
    assert set(cls.tolist()) == {0, 1, 2}
    assert broken >= 0.90  # the bound is not vacuous
    flat = img.reshape(2, -1)
    assert (seg.class_map[flat == 0] == 0).all()
    assert torch.equal(seg.class_map[flat != 0], cls)  # lit pixels in flat order = the keys in slot order
    assert torch.equal(seg.count, (flat != 0).sum(1).to(torch.int32))
    ql = lab.gather(1, coll[1])[valid]
    assert torch.equal(seg.confusion, torch.bincount(ql * 3 + cls, minlength=9).view(3, 3))


def test_segment_device_compaction_equals_collated(seg_case):
    from perceiver_io_amd import ops

    model, ev, img, lab, coll, eager, seg = seg_case
    with ops.backend("hip"):
        sp = model.segment_sparse(*coll)
        fixed = model.segment(img, capacity=coll[1].shape[1])
        wide = model.segment(img.reshape(2, -1), capacity=coll[1].shape[1] + 1024)
    for name in ("classes", "confidence", "class_map", "count"):  # same operands, same kernels: bitwise
        assert torch.equal(getattr(sp, name), getattr(seg, name)), name
        assert torch.equal(getattr(fixed, name), getattr(seg, name)), name
    assert sp.confusion is None and fixed.confusion is None
    # a larger capacity: the same count; the map agrees wherever the eager margin decides the class.
    # Not bitwise: with more (masked) key slots the cross-attention may split the keys differently,
    # which reorders its fp32 sums, so a pixel within rounding of a tie may flip.  The equal-capacity
    # call above is the bitwise check.
    assert torch.equal(wide.count, seg.count) and wide.classes.shape[1] == coll[1].shape[1] + 1024
    flat = img.reshape(2, -1)
    assert (wide.class_map[flat == 0] == 0).all()
    valid = ~coll[2]
    z = eager[valid]
    top = z.topk(2, -1).values
    decided = (top[:, 0] - top[:, 1]) > 2e-2 * z.abs().max()
    assert torch.equal(wide.class_map[flat != 0][decided], seg.class_map[flat != 0][decided])
