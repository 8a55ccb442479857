"""RandAugment on the GPU: the kernels of ``csrc/randaugment.hip`` against ``emulation.rand_augment``,
uint8 equality everywhere — every operation alone on both store variants and on grids of one and
several workgroups per sample, mixed layer sequences, the degenerate inputs of the CPU file, the
checked build's error bit, affine words that address nothing, launch-to-launch equality, a captured
graph replayed with two word blocks, and the trainer's graph path with and without the option."""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

from test_randaugment import BAD_OPS, degenerate_cases, image, word

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(3, 5, 7, 3),      # scalar variant, an image smaller than one workgroup
          (2, 8, 8, 1),      # grey, vector variant
          (2, 33, 20, 3),    # vector variant, odd rows
          (4, 64, 64, 3),    # several workgroups per sample: histograms merged across them
          (1, 224, 224, 3)]  # the ImageNet source


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


def _emu():
    from perceiver_io_amd.ops import emulation

    return emulation


def _matrix(H, W, kind, a):
    """An inverse matrix about the image centre: kind 0 rotation by ``a`` rad, 1 x-shear, 2 shift."""
    cx, cy = W / 2.0, H / 2.0
    if kind == 0:
        c, s = math.cos(a), math.sin(a)
        return (c, -s, cx - c * cx + s * cy, s, c, cy - s * cx - c * cy)
    if kind == 1:
        return (1.0, a, -a * cy, 0.0, 1.0, 0.0)
    return (1.0, 0.0, round(4 * a), 0.0, 1.0, -round(3 * a))


def op_words(op, B, H, W):
    """(B, 1, 8) words of one operation, another strength per sample."""
    rows = []
    for b in range(B):
        v = {2: 0.3 + 0.55 * b, 3: 1.9 - 0.6 * b, 4: 0.1 + 0.7 * b, 5: 1.8 - 0.5 * b, 6: 1 + 2 * b, 7: 60.0 * b + 0.5}.get(op, 0.0)
        m = _matrix(H, W, b % 3, 0.35 - 0.3 * b) if op == 1 else (1, 0, 0, 0, 1, 0)
        rows.append(word(op, v, m))
    return torch.stack(rows)[:, None]


@functools.lru_cache(maxsize=None)
def _src(B, H, W, C):
    """A batch (shared, never modified): random samples, but sample 0 uses a narrow band of levels
    (autocontrast and equalize have work to do there) and the last one is dark."""
    src = torch.stack([image(H, W, C, seed=20 + b) for b in range(B)])
    src[0] = src[0] // 3 + 40
    src[-1] = (src[-1].int() * src[-1].int() // 300).to(torch.uint8)
    return src


@functools.lru_cache(maxsize=None)
def _single_op_case(shape, op):
    B, H, W, C = shape
    words = op_words(op, B, H, W)
    return words, _emu().rand_augment(_src(*shape), words, 7)


@pytest.mark.parametrize("op", range(10))
@pytest.mark.parametrize("shape", SHAPES)
def test_each_op_alone_equals_the_emulation(shape, op):
    words, want = _single_op_case(shape, op)
    src = _src(*shape).to(DEV)
    got = _ext().rand_augment(src, words.to(DEV), 7)
    again = _ext().rand_augment(src, words.to(DEV), 7)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and got.shape == src.shape and got.is_contiguous()
    diff = (got.cpu().int() - want.int()).abs()
    print(f"{shape} op {op}: {int((diff > 0).sum())} bytes differ, max {int(diff.max())}")
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got, again)  # integer atomics only: launch-to-launch equal
    # the case is not vacuous: only identity, color on a grey image, and equalize with fewer than
    # 255 pixels (its step is 0) leave the batch as it was
    same = op == 0 or (op == 3 and shape[3] == 1) or (op == 9 and shape[1] * shape[2] < 255)
    assert torch.equal(want, _src(*shape)) == same


# sample → its three layers: every sample another sequence, each with two statistics operations
# (4, 8, 9) in a row, so a histogram must come from the previous layer's output and start from zero
SEQUENCES = [(9, 8, 4), (4, 9, 1), (8, 4, 5), (1, 9, 9), (3, 8, 9), (7, 4, 8), (9, 9, 2), (5, 8, 4)]


@pytest.mark.parametrize("hw", [(33, 20), (31, 21)], ids=["vector", "scalar"])
def test_mixed_layer_sequences(hw):
    from perceiver_io_amd import ops

    H, W = hw
    B = len(SEQUENCES)
    src = _src(B, H, W, 3)
    words = torch.stack([torch.cat([op_words(op, B, H, W)[b] for op in seq]) for b, seq in enumerate(SEQUENCES)])
    assert tuple(words.shape) == (B, 3, 8)
    want = _emu().rand_augment(src, words, 3)
    got = ops.rand_augment(src.to(DEV), words, 3)  # host words are moved
    assert torch.equal(got.cpu(), want)
    # each layer matters: the first two alone give something else
    assert not torch.equal(_ext().rand_augment(src.to(DEV), words[:, :2].contiguous().to(DEV), 3).cpu(), want)
    ops.check_device_errors()


@pytest.mark.parametrize("case", degenerate_cases(), ids=lambda c: c[0])
def test_degenerate_inputs_are_left_unchanged(case):
    _, img, words, want = case
    got = _ext().rand_augment(img[None].to(DEV), torch.stack(words)[None].to(DEV), 0)
    assert torch.equal(got[0].cpu(), want)


def test_affine_words_that_address_nothing_yield_fill():
    """NaN, huge and infinite coordinates fail the range check made on the floats, before any
    index exists: every pixel takes ``fill``.  The source is carved from the middle of a larger
    allocation, as in the crop-box test of batch_augment."""
    mats = [(float("nan"),) * 6, (1e30,) * 6, (1.0, 0.0, float("inf"), 0.0, 1.0, 0.0), (-1e30, 0.0, 0.0, 0.0, 1.0, 0.0),
            (1.0, 0.0, 0.0, float("nan"), 1.0, 0.0), (1.0, 0.0, -7.0, 0.0, 1.0, 0.0)]
    B = len(mats)
    big = torch.stack([image(9, 7, 3, seed=40 + b) for b in range(B + 8)]).to(DEV)
    src = big[4:4 + B]
    words = torch.stack([word(1, 0.0, m) for m in mats])[:, None]
    got = _ext().rand_augment(src, words.to(DEV), 200).cpu()
    assert (got == 200).all()
    assert torch.equal(got, _emu().rand_augment(src.cpu(), words, 200))


def test_binding_checks():
    from perceiver_io_amd import ops

    K = _ext()
    s = _src(*SHAPES[0]).to(DEV)
    w = op_words(2, 3, 5, 7).to(DEV)
    for bad in (lambda: K.rand_augment(s.float(), w, 0),                          # dtype
                lambda: K.rand_augment(s.permute(0, 2, 1, 3), w, 0),              # not contiguous
                lambda: K.rand_augment(s[..., :2].contiguous(), w, 0),            # two channels
                lambda: K.rand_augment(s, w[:2], 0),                              # batch mismatch
                lambda: K.rand_augment(s, w[:, :, :6].contiguous(), 0),           # word length
                lambda: K.rand_augment(s, w.cpu(), 0),
                lambda: K.rand_augment(s, w.double(), 0),
                lambda: K.rand_augment(s, w.repeat(1, 9, 1), 0),                  # N > 8
                lambda: K.rand_augment(s, w, 256)):
        with pytest.raises(RuntimeError):
            bad()
    with pytest.raises(ValueError):
        ops.rand_augment(s[..., :2].contiguous(), w)


_CHECKED_PROBE = r"""
import sys
import torch
sys.path.insert(0, "tests")
from test_randaugment import BAD_OPS, image, word
from perceiver_io_amd import ops
from perceiver_io_amd.ops import ext
K = ext.require()
assert K.checked_build() and K.__name__.endswith("_C_check"), K.__name__
src = torch.stack([image(9, 8, 3, seed=b) for b in range(len(BAD_OPS))]).cuda()
good = torch.stack([word(k + 6, 3.0) for k in range(len(BAD_OPS))])[:, None].cuda()
a = K.rand_augment(src, good, 0)
torch.cuda.synchronize()
assert K.check_errors(False) == 0  # op words of the table raise nothing
bad = torch.stack([word(op, 0.5) for op in BAD_OPS])[:, None].cuda()
b = K.rand_augment(src, bad, 0)  # identity, no exception
torch.cuda.synchronize()
assert torch.equal(b, src) and not torch.equal(a, src)
assert K.check_errors(False) == 32
try:
    ops.check_device_errors()
    raise SystemExit("check_device_errors did not raise")
except RuntimeError as e:
    assert "rand_augment" in str(e), e
assert K.check_errors(True) == 0  # cleared
print("CHECKED_OK")
"""


def test_checked_build_flags_op_words_outside_the_table():
    from perceiver_io_amd.csrc.build import ext_path

    if not ext_path("_C_check").exists():
        pytest.skip("the checked extension is not built")
    assert len(BAD_OPS) == 4
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PERCEIVER_CHECKED="1", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", _CHECKED_PROBE], env=env, capture_output=True, text=True, timeout=240,
                       cwd=root)
    assert r.returncode == 0 and "CHECKED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_graph_replay_reads_staged_words():
    """One rand_augment call captured, replayed with two staged (src, words): each replay equals the
    emulation for its own values — fresh words per replay, histograms cleared on every replay."""
    from perceiver_io_amd import ops

    B, H, W = 4, 24, 20
    sets = []
    for k, seqs in enumerate([[(9, 4), (8, 9), (1, 5), (4, 4)], [(2, 9), (9, 9), (4, 8), (0, 1)]]):
        src = torch.stack([image(H, W, 3, seed=60 + 10 * k + b) for b in range(B)])
        words = torch.stack([torch.cat([op_words(op, B, H, W)[b] for op in seq]) for b, seq in enumerate(seqs)])
        sets.append((src, words, _emu().rand_augment(src, words, 5)))
    s_src, s_words = torch.zeros_like(sets[0][0]).to(DEV), torch.zeros_like(sets[0][1]).to(DEV)
    with ops.backend("hip"):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up off the capture
            ops.rand_augment(s_src, s_words, 5)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.rand_augment(s_src, s_words, 5)
        for src, words, want in sets + sets[:1]:
            s_src.copy_(src)
            s_words.copy_(words)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out.cpu(), want)
    assert not torch.equal(sets[0][2], sets[1][2])
    ops.check_device_errors()


def _fit_and_record(tmp_path, monkeypatch, *flags):
    """img_clf fit on the graph path over 16 × 16 uint8 sources cropped to 12 × 12; → (cli, steps):
    per training step the batch ``graph_batch`` handed to the step engine and the input the step
    computed from it (copied to a buffer of the test's by the step itself, captured or eager)."""
    from perceiver_io_amd.cli.tasks import main
    from perceiver_io_amd.tasks import LitImageClassifier

    B = 8
    seen = torch.zeros(B, 12, 12, 1, device=DEV)
    steps, pending = [], []
    inputs, graph_batch = LitImageClassifier.inputs, LitImageClassifier.graph_batch

    def flush():
        if pending:
            torch.cuda.synchronize()
            steps.append((pending.pop(), seen.clone()))

    def rec_inputs(self, batch):
        out = inputs(self, batch)
        if self.training and out[0].shape == seen.shape:
            seen.copy_(out[0])
        return out

    def rec_graph_batch(self, batch):
        flush()
        out = graph_batch(self, batch)
        pending.append(tuple(t.clone() if torch.is_tensor(t) else t for t in out))
        return out

    monkeypatch.setattr(LitImageClassifier, "inputs", rec_inputs)
    monkeypatch.setattr(LitImageClassifier, "graph_batch", rec_graph_batch)
    monkeypatch.chdir(tmp_path)
    cli = main("img_clf", ["fit", "--data=SyntheticImageDataModule", "--data.image_shape=[12,12,1]",
                           "--data.source_shape=[16,16,1]", "--data.num_classes=10", "--data.size=32",
                           "--data.batch_size=8", "--data.num_workers=0", "--data.device_augment=true",
                           "--data.scale=[0.5,1.0]", *flags,
                           "--model.num_latents=16", "--model.num_latent_channels=64", "--model.num_encoder_layers=1",
                           "--model.num_encoder_self_attention_layers_per_block=1", "--model.num_frequency_bands=4",
                           "--trainer.accelerator=gpu", "--trainer.devices=1", "--trainer.max_epochs=1",
                           "--trainer.limit_val_batches=1", "--trainer.log_every_n_steps=1"])
    flush()
    return cli, steps


def test_trainer_graph_path_with_rand_augment(tmp_path, monkeypatch):
    from perceiver_io_amd import ops

    cli, steps = _fit_and_record(tmp_path, monkeypatch, "--data.rand_augment_ops=2")
    tr = cli.trainer
    eng = tr._engine
    assert tr.fused and eng.graph_enabled and tr.global_step == 4 and len(steps) == 4
    assert eng.num_graphs == 1 and eng.replays == 2  # two eager warm-ups, then two replayed steps
    (key,) = eng._graphs
    assert ("T", (8, 16, 16, 1), torch.uint8) in key and ("T", (8, 2, 8), torch.float32) in key
    assert math.isfinite(tr.callback_metrics["train_loss"])
    for batch, x_in in steps:
        assert len(batch) == 5 and tuple(batch[4].shape) == (8, 2, 8)
        ra = _emu().rand_augment(batch[0].cpu(), batch[4].cpu(), 0)
        assert torch.equal(x_in, ops.batch_augment(ra.to(DEV), batch[3], [0.5], [0.5], (12, 12)))
    # the words did something, and every step had its own
    batch, x_in = steps[-1]
    assert not torch.equal(x_in, ops.batch_augment(batch[0], batch[3], [0.5], [0.5], (12, 12)))
    assert not torch.equal(steps[-1][0][4], steps[-2][0][4])
    ops.check_device_errors()


def test_trainer_graph_path_without_the_option_is_unchanged(tmp_path, monkeypatch):
    from perceiver_io_amd import ops

    cli, steps = _fit_and_record(tmp_path, monkeypatch)
    eng = cli.trainer._engine
    assert eng.graph_enabled and eng.replays == 2 and len(steps) == 4
    assert "rand_augment_ops" not in cli.trainer.datamodule.hparams
    for batch, x_in in steps:
        assert len(batch) == 4  # (x, y, None, aug): no fifth element, batch_augment alone
        assert torch.equal(x_in, ops.batch_augment(batch[0], batch[3], [0.5], [0.5], (12, 12)))
    ops.check_device_errors()
