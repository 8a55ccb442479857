"""Device-side LArTPC batch building on the CPU: ``emulation.event_compact`` against
``sparse_collate`` on host-transformed events, ``DihedralAugment``, ``DenseCollator``,
``LArPerceiver.event_loss`` and the ``run.py`` flags."""
import numpy as np
import pytest
import torch

from perceiver_io_amd import ops
from perceiver_io_amd.data.lartpc import DenseCollator, DihedralAugment, SparseCollator, sparse_collate
from perceiver_io_amd.data.synthetic import lartpc_event
from perceiver_io_amd.models.lartpc import CLASS_WEIGHTS, LArPerceiver, class_weights
from perceiver_io_amd.ops import emulation

WMASK = 0b110  # CLASS_WEIGHTS = (0, 1, 1)


def plane_event(seed, h, w):
    """A sparse (h, w) event: ~6 % lit pixels, labels 0–2 not tied to the lit pixels."""
    g = torch.Generator().manual_seed(seed)
    img = torch.where(torch.rand(h, w, generator=g) < 0.06, torch.randn(h, w, generator=g), torch.zeros(h, w))
    lab = torch.where(torch.rand(h * w, generator=g) < 0.08, torch.randint(1, 3, (h * w,), generator=g),
                      torch.zeros(h * w, dtype=torch.long))
    return img, lab


def host_batch(events, codes, bucket=256):
    """``sparse_collate`` of the events transformed on the host, one code per event."""
    return sparse_collate([DihedralAugment.apply_host(i, l, c) for (i, l), c in zip(events, codes)], bucket=bucket)


def dense_batch(events, codes):
    img, lab = DenseCollator()(events)
    return img, lab, torch.tensor(codes, dtype=torch.int32)


def check_against_host(events, codes, compact=emulation.event_compact, to=lambda t: t):
    """event_compact at sparse_collate's own capacities equals it tensor for tensor."""
    ref = host_batch(events, codes)
    img, lab, words = dense_batch(events, codes)
    out = compact(to(img), to(lab), to(words), ref[0].shape[1], ref[3].shape[1], WMASK, 3)
    for name, a, b in zip(("values", "index", "kmask", "qidx", "qlab"), out, ref):
        assert a.dtype == b.dtype and torch.equal(a.cpu(), b), (name, codes)
    counts = torch.tensor([[int((~ref[2][i]).sum()), int((ref[4][i] != -100).sum())] for i in range(len(events))],
                          dtype=torch.int32)
    assert out[5].dtype == torch.int32 and torch.equal(out[5].cpu(), counts), codes
    return out


def test_apply_host_follows_the_code_definition():
    """Output pixel (i, j) takes source (i', j'): bit 2 swaps first, bit 0 mirrors j', bit 1 i'."""
    h = w = 5
    src = torch.arange(h * w, dtype=torch.float32).reshape(h, w)
    for code in range(8):
        out, lab = DihedralAugment.apply_host(src, src.reshape(-1).long(), code)
        for i in range(h):
            for j in range(w):
                si, sj = (j, i) if code & 4 else (i, j)
                sj = w - 1 - sj if code & 1 else sj
                si = h - 1 - si if code & 2 else si
                assert out[i, j] == src[si, sj], (code, i, j)
        assert torch.equal(lab, out.reshape(-1).long())


@pytest.mark.parametrize("code", range(8))
def test_emulation_equals_sparse_collate_every_code(code):
    events = [lartpc_event(20 + i, 64) for i in range(3)]
    check_against_host(events, [code] * 3)


def test_emulation_mixed_codes_in_one_batch():
    events = [lartpc_event(30 + i, 64) for i in range(8)]
    check_against_host(events, list(range(8)))


@pytest.mark.parametrize("code", range(4))
def test_emulation_non_square_plane(code):
    events = [plane_event(40 + i, 24, 40) for i in range(2)]
    check_against_host(events, [code] * 2)


def test_non_square_plane_refuses_a_transposing_code():
    img, lab, words = dense_batch([plane_event(1, 24, 40)], [5])
    with pytest.raises(ValueError, match="square"):
        emulation.event_compact(img, lab, words, 256, 256, WMASK, 3)
    with pytest.raises(ValueError, match="square"):
        ops.event_compact(img, lab, words, 256, 256, CLASS_WEIGHTS)
    with pytest.raises(ValueError, match="square"):
        DihedralAugment.apply_host(*plane_event(1, 24, 40), 4)


def test_code_zero_keys_equal_nonzero_compact():
    events = [lartpc_event(50 + i, 64) for i in range(2)]
    img, lab, words = dense_batch(events, [0, 0])
    out = emulation.event_compact(img, lab, words, 512, 512, WMASK, 3)
    ref = emulation.nonzero_compact(img.reshape(2, -1), 512)
    for a, b in zip(out[:3], ref[:3]):
        assert torch.equal(a, b)
    assert torch.equal(out[5][:, 0], ref[3])


def edge_batch():
    """Four 16 × 16 samples: all zero; labels but no lit pixel; lit pixels but no label; −0.0 / NaN."""
    img = torch.zeros(4, 16, 16)
    lab = torch.zeros(4, 256, dtype=torch.uint8)
    lab[1, [3, 17, 200]] = torch.tensor([1, 2, 1], dtype=torch.uint8)
    img[2, 0, 5], img[2, 15, 15] = 2.0, -1.0
    img[3, 1, 1], img[3, 2, 2], img[3, 3, 3] = -0.0, float("nan"), 4.0
    lab[3, 40] = 2
    return img, lab


def check_edges(compact, to=lambda t: t):
    img, lab = edge_batch()
    words = torch.tensor([3, 6, 5, 0], dtype=torch.int32)
    v, i, m, qi, ql, counts = [t.cpu() for t in compact(to(img), to(lab), to(words), 8, 8, WMASK, 3)]
    assert counts.tolist() == [[0, 0], [0, 3], [2, 0], [2, 1]]
    pad_q = torch.arange(8)
    assert m[0].all() and not v[0].any() and not i[0].any() and torch.equal(qi[0], pad_q) and (ql[0] == -100).all()
    assert m[1].all() and (ql[1, :3] >= 1).all() and (ql[1, 3:] == -100).all() and torch.equal(qi[1, 3:], pad_q[3:])
    assert not m[2, :2].any() and m[2, 2:].all() and (ql[2] == -100).all()
    # sample 3, code 0: −0.0 is zero, NaN is a lit pixel
    assert i[3, :2].tolist() == [34, 51] and torch.isnan(v[3, 0, 0]) and v[3, 1, 0] == 4.0
    assert qi[3, 0] == 40 and ql[3, 0] == 2
    # the same samples through the host path
    events = [(img[b], lab[b].long()) for b in range(4)]
    ref = sparse_collate([DihedralAugment.apply_host(a, b, int(c)) for (a, b), c in zip(events, words)], bucket=8)
    for a, b in zip((v, i, m, qi, ql), ref):
        assert torch.equal(a.nan_to_num(nan=7.0), b.nan_to_num(nan=7.0)) if a.is_floating_point() else torch.equal(a, b)


def test_emulation_edge_cases():
    check_edges(emulation.event_compact)


def check_overflow(compact, to=lambda t: t):
    """Key and query overflow separately: true counts, the first ``cap`` in order."""
    events = [lartpc_event(60 + i, 64) for i in range(2)]
    codes = [6, 1]
    full = host_batch(events, codes)
    nk = (~full[2]).sum(1)
    nq = (full[4] != -100).sum(1)
    assert int(nk.min()) > 40 and int(nq.min()) > 40
    img, lab, words = dense_batch(events, codes)
    for kcap, qcap in ((32, full[3].shape[1]), (full[0].shape[1], 24)):
        out = [t.cpu() for t in compact(to(img), to(lab), to(words), kcap, qcap, WMASK, 3)]
        assert torch.equal(out[5], torch.stack([nk, nq], 1).to(torch.int32))
        for a, b, cap in zip(out[:5], full, (kcap, kcap, kcap, qcap, qcap)):
            assert torch.equal(a, b[:, :cap])


def test_emulation_overflow_keeps_the_first_slots_and_true_counts():
    check_overflow(emulation.event_compact)


def test_counting_call_and_bad_code():
    events = [lartpc_event(70 + i, 64) for i in range(2)]
    img, lab, _ = dense_batch(events, [0, 0])
    nine = torch.tensor([9, -1], dtype=torch.int32)
    zero = torch.zeros(2, dtype=torch.int32)
    a = emulation.event_compact(img, lab, nine, 512, 512, WMASK, 3)
    b = emulation.event_compact(img, lab, zero, 512, 512, WMASK, 3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))  # a code outside 0–7 is the identity
    c = emulation.event_compact(img, lab, zero, 0, 0, WMASK, 3)
    assert c[0].shape == (2, 0, 1) and c[3].shape == (2, 0) and torch.equal(c[5], b[5])


def test_labels_outside_the_weights_are_not_queries():
    img = torch.zeros(1, 8, 8)
    lab = torch.zeros(1, 64, dtype=torch.uint8)
    lab[0, :5] = torch.tensor([1, 200, 2, 8, 3], dtype=torch.uint8)
    out = emulation.event_compact(img, lab, torch.zeros(1, dtype=torch.int32), 4, 4, WMASK, 3)
    assert out[5].tolist() == [[0, 2]] and out[3][0, :2].tolist() == [0, 2] and out[4][0].tolist() == [1, 2, -100, -100]


def test_ops_event_compact_builds_wmask_from_the_weights():
    events = [lartpc_event(80 + i, 64) for i in range(2)]
    img, lab, words = dense_batch(events, [2, 7])
    for weights, mask in (((0.0, 1.0, 1.0), 0b110), ((0.0, 0.0, 2.5), 0b100), ((1.0, 1.0, 1.0), 0b111)):
        a = ops.event_compact(img, lab, words, 512, 4096, weights)
        b = emulation.event_compact(img, lab, words, 512, 4096, mask, 3)
        assert isinstance(a, tuple) and all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        ops.event_compact(img, lab.long(), words, 512, 512, CLASS_WEIGHTS)


def test_event_loss_equals_sparse_loss_on_collated_events():
    """Same tensors in, same loss out: bitwise; gradients at test_lartpc.py's tolerance."""
    torch.manual_seed(0)
    size = 32
    model = LArPerceiver(size)
    events = [lartpc_event(3000 + i, size) for i in range(2)]
    codes = [5, 2]
    w = class_weights("cpu")
    ref_batch = host_batch(events, codes, bucket=64)
    ref, ref_acc = model.sparse_loss(ref_batch, w)
    ref.backward()
    g_ref = {n: p.grad.clone() for n, p in model.perceiver.named_parameters()}
    model.zero_grad()
    loss, acc, counts = model.event_loss(dense_batch(events, codes), w, ref_batch[0].shape[1], ref_batch[3].shape[1])
    loss.backward()
    assert torch.equal(loss, ref), (float(loss), float(ref))
    assert all(float(acc[k]) == float(ref_acc[k]) for k in ref_acc)
    assert counts.shape == (2, 2) and int(counts[:, 0].max()) <= ref_batch[0].shape[1]
    for n, p in model.perceiver.named_parameters():
        gd = g_ref[n]
        tol = 1e-5 * max(1.0, float(gd.abs().max()))
        assert torch.allclose(p.grad, gd, atol=tol, rtol=1e-4), (n, float((p.grad - gd).abs().max()))
    # pixels past a capacity leave the loss, and the counts show it
    small, _, c2 = model.event_loss(dense_batch(events, codes), w, 16, 16)
    assert torch.equal(c2, counts) and int(c2.min()) > 16 and not torch.equal(small, loss)


def test_dense_collator_stacks_bytes():
    events = [lartpc_event(i, 32) for i in range(3)]
    img, lab = DenseCollator()(events)
    assert img.shape == (3, 32, 32) and img.dtype == torch.float32
    assert lab.shape == (3, 1024) and lab.dtype == torch.uint8
    assert torch.equal(lab.long(), torch.stack([e[1] for e in events]))


def test_dihedral_draw():
    aug = DihedralAugment("dihedral")
    a = aug.draw(DihedralAugment.rng(3, 1), 4096)
    b = aug.draw(DihedralAugment.rng(3, 1), 4096)
    assert a.dtype == np.int32 and a.shape == (4096,) and np.array_equal(a, b)
    assert not np.array_equal(a, aug.draw(DihedralAugment.rng(3, 2), 4096))  # another rank, other draws
    assert sorted(set(a.tolist())) == list(range(8))
    f = DihedralAugment("flip").draw(DihedralAugment.rng(0, 0), 4096)
    assert sorted(set(f.tolist())) == [0, 1, 2, 3]
    assert not aug.draw(DihedralAugment.rng(0, 0), 64, train=False).any()
    assert not DihedralAugment("none").draw(DihedralAugment.rng(0, 0), 64).any()
    with pytest.raises(ValueError):
        DihedralAugment("rotate")


def test_run_device_collate_on_cpu(tmp_path, capsys):
    import run

    ck = tmp_path / "ckpt"
    run.main(["--device-collate", "--augment", "dihedral", "--size", "32", "--events", "8", "--max-steps", "3",
              "--device", "cpu", "--workers", "0", "--log-dir", str(tmp_path / "runs"), "--ckpt-dir", str(ck)])
    state = torch.load(next(ck.glob("model_*.ckpt")), weights_only=True)
    assert all(torch.isfinite(v).all() for v in state["model_state_dict"].values() if v.is_floating_point())
    out = capsys.readouterr().out
    assert "device collate:" in out and "overflow" not in out


def test_run_reports_overflow(tmp_path, capsys):
    import run

    run.main(["--device-collate", "--key-capacity", "8", "--query-capacity", "8", "--size", "32", "--events", "4",
              "--val-events", "4", "--max-steps", "1", "--device", "cpu", "--workers", "0",
              "--log-dir", str(tmp_path / "runs"), "--ckpt-dir", str(tmp_path / "ckpt")])
    assert "step 0: capacity overflow, dropped" in capsys.readouterr().out


def test_run_flags_pick_the_collator():
    import run

    base = ["--size", "32", "--events", "4", "--val-events", "4", "--workers", "0", "--device", "cpu"]
    for loader in run.make_loaders(run.parse_args(base)):
        assert type(loader.collate_fn) is SparseCollator
    for loader in run.make_loaders(run.parse_args(base + ["--device-collate"])):
        assert type(loader.collate_fn) is DenseCollator
    with pytest.raises(SystemExit):
        run.parse_args(base + ["--augment", "flip"])  # needs --device-collate
