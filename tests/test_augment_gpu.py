"""Device-side image augmentation on the GPU: the ``batch_augment`` kernel against its emulation
(both store variants, mixed flips, up- and downsampling, a 1 × 1 box), the copy path bit for bit
against the host transform, launch-to-launch equality, box clamping inside owned memory, a captured
graph reading staged parameters, and the trainer's graph path on raw uint8 batches."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_augment import AUGMENT_TOL, CLAMP_CASES, MEAN3, STD3, clamp_params, host_transform

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (B, Hs, Ws, C, oh, ow): ow·C % 4 == 0 → the 16-byte store variant, else the scalar one
SHAPES = [(3, 9, 11, 3, 7, 5),        # scalar
          (1, 8, 8, 1, 8, 8),         # vector, one sample
          (5, 13, 7, 4, 6, 10),       # vector, 4 channels
          (2, 10, 10, 2, 3, 3),       # scalar, 2 channels
          (128, 28, 28, 1, 24, 24),   # the MNIST batch
          (2, 256, 256, 3, 224, 224)]  # ImageNet shape: several blocks per sample


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


def _emu():
    from perceiver_io_amd.ops import emulation

    return emulation


def _norm(C):
    mean = (MEAN3 + (0.5,))[:C] if C > 1 else (0.5,)
    std = (STD3 + (0.25,))[:C] if C > 1 else (0.5,)
    return list(mean), list(std)


@functools.lru_cache(maxsize=None)
def _case(B, Hs, Ws, C, oh, ow):
    """(src, params) on the host and the emulation's result there (shared, never modified): random
    boxes of every size from 1 × 1 to the whole image — up- and downsampling in one batch — with
    every other sample flipped; sample 0 is a 1 × 1 box, the last one the whole image."""
    g = torch.Generator().manual_seed(B * 1000 + Hs)
    src = torch.randint(0, 256, (B, Hs, Ws, C), dtype=torch.uint8, generator=g)
    h = torch.randint(1, Hs + 1, (B,), generator=g)
    w = torch.randint(1, Ws + 1, (B,), generator=g)
    h[0], w[0] = 1, 1
    h[-1], w[-1] = Hs, Ws
    if B > 2:
        h[1], w[1] = min(2 * oh, Hs), max(ow // 2, 1)  # rows down-, columns upsampled
    y0 = (torch.rand(B, generator=g) * (Hs - h + 1)).long()
    x0 = (torch.rand(B, generator=g) * (Ws - w + 1)).long()
    p = torch.zeros(B, 8)
    p[:, 0], p[:, 1], p[:, 2], p[:, 3] = y0, x0, h, w
    p[:, 4] = (torch.arange(B) % 2).float()
    mean, std = _norm(C)
    return src, p, _emu().batch_augment(src, p, mean, std, (oh, ow))


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_matches_emulation(shape):
    B, Hs, Ws, C, oh, ow = shape
    src, p, want = _case(*shape)
    mean, std = _norm(C)
    got = _ext().batch_augment(src.to(DEV), p.to(DEV), mean, std, oh, ow)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, oh, ow, C) and got.is_contiguous()
    gap = (got.cpu() - want).abs().max().item()
    print(f"{shape}: max |kernel - emulation| = {gap:.3e}, bitwise equal: {torch.equal(got.cpu(), want)}")
    assert gap <= AUGMENT_TOL, gap
    # launch-to-launch: no atomics, a fixed reading order
    again = _ext().batch_augment(src.to(DEV), p.to(DEV), mean, std, oh, ow)
    assert torch.equal(got, again)


def test_ops_dispatch_and_binding_checks():
    from perceiver_io_amd import ops

    src, p, want = _case(*SHAPES[0])
    mean, std = _norm(3)
    got = ops.batch_augment(src.to(DEV), p, mean, std, (7, 5))  # host params are moved
    assert (got.cpu() - want).abs().max().item() <= AUGMENT_TOL
    K = _ext()
    s, q = src.to(DEV), p.to(DEV)
    for bad in (lambda: K.batch_augment(s.float(), q, mean, std, 7, 5),             # dtype
                lambda: K.batch_augment(s.permute(0, 2, 1, 3), q, mean, std, 7, 5),  # not contiguous
                lambda: K.batch_augment(s, q[:, :6].contiguous(), mean, std, 7, 5),  # params shape
                lambda: K.batch_augment(s, q[:2], mean, std, 7, 5),
                lambda: K.batch_augment(s, q.cpu(), mean, std, 7, 5),
                lambda: K.batch_augment(s, q, mean[:2], std, 7, 5),
                lambda: K.batch_augment(torch.zeros(1, 4, 4, 5, dtype=torch.uint8, device=DEV), q[:1], [0.5] * 5,
                                        [0.5] * 5, 2, 2),                            # C > 4
                lambda: K.batch_augment(s, q, mean, std, 1 << 15, 1 << 15)):         # output ≥ 2^30 elements
        with pytest.raises(RuntimeError):
            bad()


def test_copy_path_bit_equal():
    B = 128
    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (B, 28, 28, 1), dtype=torch.uint8, generator=g)
    u8[0] = torch.arange(784).remainder(256).to(torch.uint8).reshape(28, 28, 1)  # every byte value
    tops = torch.randint(0, 5, (B,), generator=g)
    lefts = torch.randint(0, 5, (B,), generator=g)
    p = torch.zeros(B, 8)
    p[:, 0], p[:, 1], p[:, 2], p[:, 3] = tops, lefts, 24, 24
    got = _ext().batch_augment(u8.to(DEV), p.to(DEV), [0.5], [0.5], 24, 24).cpu()
    assert torch.equal(got, _emu().batch_augment(u8, p, [0.5], [0.5], (24, 24)))
    host = torch.stack([host_transform(u8[k, :, :, 0], int(tops[k]), int(lefts[k])) for k in range(B)])
    assert torch.equal(got, host)
    # flipped copies: still no arithmetic but the normalize
    p[:, 4] = 1.0
    got = _ext().batch_augment(u8.to(DEV), p.to(DEV), [0.5], [0.5], 24, 24).cpu()
    assert torch.equal(got, host.flip(2))
    # three channels with per-channel statistics: (v / 255 − mean) / std in that order
    src, _, _ = _case(*SHAPES[0])
    q = torch.zeros(3, 8)
    q[:, 0], q[:, 1], q[:, 2], q[:, 3] = torch.tensor([0, 1, 2]), torch.tensor([6, 0, 3]), 7, 5
    got = _ext().batch_augment(src.to(DEV), q.to(DEV), list(MEAN3), list(STD3), 7, 5).cpu()
    want = torch.stack([src[k, k:k + 7, int(q[k, 1]):int(q[k, 1]) + 5].float() for k in range(3)])
    want = (want / 255.0 - torch.tensor(MEAN3)) / torch.tensor(STD3)
    assert torch.equal(got, want)


@pytest.mark.parametrize("out_hw", [(4, 5), (4, 4)])
def test_clamped_boxes_stay_inside_the_source(out_hw):
    """Overhanging, zero, negative, NaN and infinite words: the source is carved from the middle of
    a larger allocation, so even a wrong clamp would stay inside owned memory; the result is the
    emulation's (the explicitly clamped boxes)."""
    B = len(CLAMP_CASES)
    raw, good = clamp_params(flag=1.0)
    g = torch.Generator().manual_seed(5)
    big = torch.randint(0, 256, (B + 8, 9, 11, 3), dtype=torch.uint8, generator=g).to(DEV)
    src = big[4:4 + B]
    assert src.is_contiguous() and src.data_ptr() == big.data_ptr() + 4 * 9 * 11 * 3
    got = _ext().batch_augment(src, raw.to(DEV), list(MEAN3), list(STD3), *out_hw).cpu()
    assert torch.isfinite(got).all()
    assert torch.equal(got, _ext().batch_augment(src, good.to(DEV), list(MEAN3), list(STD3), *out_hw).cpu())
    want = _emu().batch_augment(src.cpu(), raw, MEAN3, STD3, out_hw)
    assert (got - want).abs().max().item() <= AUGMENT_TOL


_CHECKED_PROBE = r"""
import sys
import torch
sys.path.insert(0, "tests")
from test_augment import CLAMP_CASES, MEAN3, STD3, clamp_params
from perceiver_io_amd import ops
from perceiver_io_amd.ops import ext
K = ext.require()
assert K.checked_build() and K.__name__.endswith("_C_check"), K.__name__
raw, good = clamp_params(flag=1.0)
B = len(CLAMP_CASES)
big = torch.randint(0, 256, (B + 8, 9, 11, 3), dtype=torch.uint8, device="cuda")
src = big[4:4 + B]
a = K.batch_augment(src, good.cuda(), list(MEAN3), list(STD3), 4, 5)
torch.cuda.synchronize()
assert K.check_errors(False) == 0  # boxes inside the source raise nothing
b = K.batch_augment(src, raw.cuda(), list(MEAN3), list(STD3), 4, 5)  # clamped, no exception
torch.cuda.synchronize()
assert torch.equal(a, b)
assert K.check_errors(False) == 16
try:
    ops.check_device_errors()
    raise SystemExit("check_device_errors did not raise")
except RuntimeError as e:
    assert "batch_augment" in str(e), e
assert K.check_errors(True) == 0  # cleared
print("CHECKED_OK")
"""


def test_checked_build_flags_clamped_boxes():
    from perceiver_io_amd.csrc.build import ext_path

    if not ext_path("_C_check").exists():
        pytest.skip("the checked extension is not built")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PERCEIVER_CHECKED="1", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", _CHECKED_PROBE], env=env, capture_output=True, text=True, timeout=240,
                       cwd=root)
    assert r.returncode == 0 and "CHECKED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_graph_replay_reads_staged_params():
    """batch_augment + batch_mix captured once, replayed with two different staged (src, params,
    mix): each replay equals the eager calls on those values."""
    from perceiver_io_amd import ops

    B, Hs, Ws, C, oh, ow = 6, 20, 24, 3, 12, 16
    mean, std = list(MEAN3), list(STD3)
    g = torch.Generator().manual_seed(2)
    y = torch.randint(0, 10, (B,), generator=g).to(DEV)

    def values(k):
        src = torch.randint(0, 256, (B, Hs, Ws, C), dtype=torch.uint8, generator=g)
        p = torch.zeros(B, 8)
        p[:, 2] = torch.randint(1, Hs + 1, (B,), generator=g)
        p[:, 3] = torch.randint(1, Ws + 1, (B,), generator=g)
        p[:, 0] = (torch.rand(B, generator=g) * (Hs - p[:, 2] + 1)).floor()
        p[:, 1] = (torch.rand(B, generator=g) * (Ws - p[:, 3] + 1)).floor()
        p[:, 4] = (torch.arange(B) % 2 == k).float()
        mix = torch.tensor([[1.0, 0.3, 0, 0, 0, 0], [2.0, 1.0 - 5 * 8 / (oh * ow), 3.0, 8.0, 4.0, 12.0]][k])
        return src.to(DEV), p.to(DEV), mix.to(DEV)

    sets = [values(0), values(1)]
    with ops.backend("hip"):
        want = []
        for src, p, mix in sets:
            x = ops.batch_augment(src, p, mean, std, (oh, ow))
            want.append((x, ops.batch_mix(x, y, mix)[0]))
        s_src, s_p, s_mix = (torch.zeros_like(t) for t in sets[0])
        s_p[:, 2:4] = 1.0
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up off the capture
            ops.batch_mix(ops.batch_augment(s_src, s_p, mean, std, (oh, ow)), y, s_mix)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            gx = ops.batch_augment(s_src, s_p, mean, std, (oh, ow))
            gm = ops.batch_mix(gx, y, s_mix)[0]
        for (src, p, mix), (wx, wm) in zip(sets, want):
            s_src.copy_(src)
            s_p.copy_(p)
            s_mix.copy_(mix)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(gx, wx) and torch.equal(gm, wm)
    assert not torch.equal(want[0][0], want[1][0])
    ops.check_device_errors()


def test_trainer_graph_path_on_raw_uint8_batches(tmp_path):
    """img_clf fit on the bf16 graph path with device augmentation and CutMix: 6 steps, the last a
    partial batch; one captured graph per batch shape, a finite loss, clean device error words."""
    from perceiver_io_amd import ops
    from perceiver_io_amd.cli.tasks import main

    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        cli = main("img_clf", ["fit", "--data=MNISTDataModule", "--data.synthetic=true", "--data.synthetic_size=100",
                               "--data.val_split=20", "--data.batch_size=15", "--data.num_workers=0",
                               "--data.random_crop=24", "--data.device_augment=true", "--data.hflip=0.5",
                               "--model.num_latents=16", "--model.num_latent_channels=64",
                               "--model.num_encoder_layers=2", "--model.num_encoder_self_attention_layers_per_block=1",
                               "--model.cutmix_alpha=1.0", "--model.label_smoothing=0.1",
                               "--trainer.accelerator=gpu", "--trainer.devices=1", "--trainer.max_epochs=1",
                               "--trainer.limit_val_batches=1", "--trainer.log_every_n_steps=1"])
    finally:
        os.chdir(old)
    tr = cli.trainer
    eng = tr._engine
    assert tr.fused and eng.graph_enabled
    assert tr.global_step == 6  # 80 training images: five batches of 15 and one of 5
    assert eng.num_graphs == 2 and eng.captures == 2  # one per batch shape
    assert eng.replays == 4  # two eager warm-ups, then every step replayed
    keys = list(eng._graphs)
    assert all(("T", (n, 28, 28, 1), torch.uint8) in k and ("T", (n, 8), torch.float32) in k
               for k, n in zip(keys, (15, 5))), keys
    m = tr.callback_metrics
    assert math.isfinite(m["train_loss"]) and math.isfinite(m["val_loss"])
    ops.check_device_errors()
