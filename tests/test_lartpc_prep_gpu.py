"""``event_compact`` (csrc/lartpc_prep.hip) on the GPU against its emulation — integers and copied
floats, so everything is ``torch.equal`` — the checked build's error bits, and a captured training
step over ``LArPerceiver.event_loss`` that follows the staged dihedral codes."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from perceiver_io_amd.data.lartpc import DenseCollator, sparse_collate
from perceiver_io_amd.data.synthetic import lartpc_event
from test_lartpc_prep import WMASK, check_edges, check_overflow, dense_batch, host_batch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


def _emu():
    from perceiver_io_amd.ops import emulation

    return emulation


def _cuda(t):
    return t.to(DEV)


@functools.lru_cache(maxsize=None)
def _events(size, n):
    img, lab = DenseCollator()([lartpc_event(90 + i, size) for i in range(n)])
    return img, lab


@functools.lru_cache(maxsize=None)
def _reference(size, codes, kcap, qcap):
    """The emulation's result on the CPU, computed once per case and never modified."""
    img, lab = _events(size, len(codes))
    return tuple(_emu().event_compact(img, lab, torch.tensor(codes, dtype=torch.int32), kcap, qcap, WMASK, 3))


def _check(size, codes, kcap, qcap, segs=0, tile=0):
    img, lab = _events(size, len(codes))
    words = torch.tensor(codes, dtype=torch.int32, device=DEV)
    out = _ext().event_compact(img.to(DEV), lab.to(DEV), words, kcap, qcap, WMASK, 3, segs, tile)
    ref = _reference(size, codes, kcap, qcap)
    for name, a, b in zip(("values", "index", "kmask", "qidx", "qlab", "counts"), out, ref):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b), (name, codes, segs, tile)
    return out


# 64 × 64 = 4 tiles of 1,024: the default launch has one tile per segment; (1, 4) is the
# single-segment kernel without a count launch, (3, 8) two-tile segments of the 8-load kernel
# with the last one cut short, (7, 4) segments that start past the end of the plane
@pytest.mark.parametrize("segs,tile", [(0, 0), (1, 4), (3, 8), (7, 4)])
@pytest.mark.parametrize("code", range(8))
def test_small_events_every_code(code, segs, tile):
    _check(64, (code,) * 3, 512, 768, segs, tile)


def test_small_events_mixed_codes_in_one_batch():
    for codes in ((0, 5, 3), (7, 2, 4), (6, 1, 6)):
        _check(64, codes, 512, 768)


@pytest.mark.parametrize("segs,tile", [(0, 0), (2, 8)])
def test_segment_ends_inside_a_tile(segs, tile):
    """96 × 96 = 9,216 pixels: no multiple of a tile, so the last segment ends mid-tile."""
    for codes in ((0, 3), (4, 7)):
        _check(96, codes, 1024, 1024, segs, tile)


def test_real_shape():
    out = _check(512, (5, 6), 8192, 8192)
    assert int(out[5].min()) > 1000  # many segments carry keys and queries
    assert torch.equal(_check(512, (5, 6), 0, 0)[5], out[5])  # the counting call


def test_equals_sparse_collate_at_its_capacities():
    events = [lartpc_event(90 + i, 64) for i in range(3)]
    codes = (3, 4, 6)
    ref = host_batch(events, codes)
    out = _check(64, codes, ref[0].shape[1], ref[3].shape[1])
    for a, b in zip(out[:5], ref):
        assert torch.equal(a.cpu(), b)


def test_code_zero_keys_equal_nonzero_compact():
    img, lab = _events(64, 3)
    out = _check(64, (0, 0, 0), 512, 768)
    ref = _ext().nonzero_compact(img.reshape(3, -1).to(DEV), 512)
    assert all(torch.equal(a, b) for a, b in zip(out[:3], ref[:3])) and torch.equal(out[5][:, 0], ref[3])


def test_edge_cases():
    check_edges(_ext().event_compact, _cuda)


def test_overflow_keeps_the_first_slots_and_true_counts():
    check_overflow(_ext().event_compact, _cuda)


def test_bad_code_is_the_identity_and_bad_labels_are_not_queries():
    img, lab = _events(64, 2)
    lab = lab.clone()
    lab[0, :4] = torch.tensor([200, 8, 3, 1], dtype=torch.uint8)
    ref = _emu().event_compact(img, lab, torch.zeros(2, dtype=torch.int32), 512, 768, WMASK, 3)
    words = torch.tensor([9, -3], dtype=torch.int32, device=DEV)
    out = _ext().event_compact(img.to(DEV), lab.to(DEV), words, 512, 768, WMASK, 3)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(out, ref))


def test_two_calls_give_identical_bytes_and_words_are_read_from_memory():
    img, lab = _events(64, 3)
    dimg, dlab = img.to(DEV), lab.to(DEV)
    words = torch.tensor([1, 6, 4], dtype=torch.int32, device=DEV)
    a = _ext().event_compact(dimg, dlab, words, 512, 768, WMASK, 3)
    b = _ext().event_compact(dimg, dlab, words, 512, 768, WMASK, 3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    words.copy_(torch.tensor([2, 6, 7], dtype=torch.int32))  # in place: same pointer, new codes
    c = _ext().event_compact(dimg, dlab, words, 512, 768, WMASK, 3)
    assert not torch.equal(c[1][0], a[1][0]) and torch.equal(c[1][1], a[1][1]) and not torch.equal(c[3][2], a[3][2])
    assert all(torch.equal(x.cpu(), y) for x, y in zip(c, _reference(64, (2, 6, 7), 512, 768)))


def test_non_square_planes_are_refused():
    from perceiver_io_amd import ops

    img = torch.zeros(1, 24, 40, device=DEV)
    lab = torch.zeros(1, 960, dtype=torch.uint8, device=DEV)
    words = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="square"):
        _ext().event_compact(img, lab, words, 64, 64, WMASK, 3)
    with pytest.raises(ValueError, match="square"):
        ops.event_compact(img, lab, words, 64, 64, (0.0, 1.0, 1.0))


_CHECKED_PROBE = r"""
import torch
from perceiver_io_amd import ops
from perceiver_io_amd.ops import ext
K = ext.require()
assert K.checked_build() and K.__name__.endswith("_C_check"), K.__name__
g = torch.Generator().manual_seed(0)
img = torch.where(torch.rand(2, 64, 64, generator=g) < 0.05, torch.ones(2, 64, 64), torch.zeros(2, 64, 64)).cuda()
lab = torch.randint(0, 3, (2, 4096), generator=g).to(torch.uint8).cuda()
K.check_errors(True)
good = torch.tensor([7, 0], dtype=torch.int32).cuda()
K.event_compact(img, lab, good, 512, 4096, 6, 3)
assert K.check_errors(False) == 0  # codes 0-7 and labels below the class count raise nothing
for words, labels, bit in ((torch.tensor([9, 0], dtype=torch.int32).cuda(), lab, 128),
                           (good, lab.clone().index_fill_(1, torch.tensor([5]).cuda(), 200), 4)):
    try:
        K.event_compact(img, labels, words, 512, 4096, 6, 3)
        raise SystemExit("the checked launch did not raise")
    except RuntimeError as e:
        assert "checked build: event_compact" in str(e) and f"error bits {bit}:" in str(e), e
assert K.check_errors(True) == 0  # read and cleared by the raising launch
# inside a captured graph nothing can raise: the word stays set for check_device_errors
bad = torch.tensor([9, 0], dtype=torch.int32).cuda()
s = torch.cuda.Stream()
s.wait_stream(torch.cuda.current_stream())
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g, stream=s):
    out = K.event_compact(img, lab, bad, 512, 4096, 6, 3)
g.replay()
torch.cuda.synchronize()
assert K.check_errors(False) == 128
try:
    ops.check_device_errors()
    raise SystemExit("check_device_errors did not raise")
except RuntimeError as e:
    assert "event_compact" in str(e), e
assert K.check_errors(True) == 0
print("CHECKED_OK")
"""


def test_checked_build_flags_bad_codes_and_labels():
    from perceiver_io_amd.csrc.build import ext_path

    assert ext_path("_C_check").exists(), "the checked extension is not built"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PERCEIVER_CHECKED="1", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", _CHECKED_PROBE], env=env, capture_output=True, text=True, timeout=240,
                       cwd=root)
    assert r.returncode == 0 and "CHECKED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_graph_engine_follows_the_staged_codes():
    """One captured step over ``event_loss``, three steps with three word vectors: each loss matches
    an eager fused step on the host-collated events of that code (the tolerance of
    ``test_model_gpu.test_graph_engine_matches_eager_steps``), and one graph serves them all."""
    from perceiver_io_amd.models.lartpc import LArPerceiver, class_weights
    from perceiver_io_amd.ops.optim import FusedAdam
    from perceiver_io_amd.train.engine import StepEngine

    events = [lartpc_event(90 + i, 64) for i in range(3)]
    steps = [(0, 5, 3), (6, 6, 1), (4, 2, 7)]
    shapes = sparse_collate(events, bucket=256)  # counts do not change under the symmetries
    kcap, qcap = shapes[0].shape[1], shapes[3].shape[1]
    w = class_weights(DEV)
    losses = {}
    for graph in (False, True):
        torch.manual_seed(6)
        model = LArPerceiver(64).to(DEV)
        opt = FusedAdam(model.trained_parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=10.0)
        if graph:
            fn = lambda b: model.event_loss(b, w, kcap, qcap)[0]  # noqa: E731
        else:
            fn = lambda b: model.sparse_loss(b, w)[0]  # noqa: E731
        eng = StepEngine(fn, opt, device=DEV, graph=graph, warmup_eager=0)
        out = []
        for codes in steps:
            if graph:
                batch = tuple(t.to(DEV) for t in dense_batch(events, codes))
            else:
                batch = tuple(t.to(DEV) for t in host_batch(events, codes))
                assert batch[0].shape[1] == kcap and batch[3].shape[1] == qcap
            out.append(float(eng.step(batch)))
        losses[graph] = out
        if graph:
            assert eng.num_graphs == 1 and eng.captures == 1 and eng.replays == 3
    for a, b in zip(losses[False], losses[True]):
        assert abs(a - b) <= 5e-3 * abs(a), losses
