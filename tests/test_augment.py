"""Device-side image augmentation on the CPU: the emulation of ``batch_augment`` against
``F.interpolate`` in fp64, the copy path against the host transform bit for bit, box clamping, the
host parameter draws, the data modules' raw-uint8 path, and the options through the CLI."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

# emulation (fp32, each operation rounded on its own) vs the fp64 F.interpolate pipeline over CASES:
# largest |gap| measured 1.849e-06 on the CPU (the 9 × 11 → 4 × 5 case: an fp32 rounding of λ times a
# 255-step between neighbours, over 255·std ≈ 57); the bound is 4 × that = 7.4e-06, rounded up to one
# significant digit.  Both sides are deterministic: the margin only covers another torch build's rounding.
AUGMENT_TOL = 8e-6

MEAN3, STD3 = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# (Hs, Ws, C, out_hw, boxes [y0, x0, h, w]): upsampling, downsampling, non-square, whole image, 1 × 1
CASES = [
    (9, 11, 3, (8, 8), [(2, 3, 3, 3), (0, 0, 9, 11), (1, 2, 5, 7), (8, 10, 1, 1)]),
    (9, 11, 3, (4, 5), [(0, 0, 9, 11), (3, 1, 6, 4), (0, 5, 9, 2), (2, 2, 4, 5)]),
    (8, 8, 1, (8, 8), [(2, 1, 3, 3), (0, 0, 8, 8), (0, 3, 8, 4), (5, 5, 2, 3)]),
    (8, 8, 1, (4, 5), [(0, 0, 8, 8), (1, 1, 6, 7), (4, 0, 3, 8), (0, 0, 4, 5)]),
]


def _src(B, Hs, Ws, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, Hs, Ws, C), dtype=torch.uint8, generator=g)


def _params(boxes, flips):
    p = torch.zeros(len(boxes), 8)
    for k, (b, f) in enumerate(zip(boxes, flips)):
        p[k, :4] = torch.tensor(b, dtype=torch.float32)
        p[k, 4] = float(f)
    return p


def interpolate_reference(src, boxes, flips, mean, std, out_hw):
    """slice → F.interpolate(bilinear, align_corners=False, antialias=False) → flip → normalize, fp64"""
    C = src.shape[3]
    m = torch.tensor(mean, dtype=torch.float64).expand(C) if len(mean) == 1 else torch.tensor(mean, dtype=torch.float64)
    s = torch.tensor(std, dtype=torch.float64).expand(C) if len(std) == 1 else torch.tensor(std, dtype=torch.float64)
    outs = []
    for k, ((y0, x0, h, w), f) in enumerate(zip(boxes, flips)):
        crop = src[k, y0:y0 + h, x0:x0 + w].double().permute(2, 0, 1)[None]
        r = F.interpolate(crop, size=tuple(out_hw), mode="bilinear", align_corners=False, antialias=False)[0]
        r = r.permute(1, 2, 0)
        if f:
            r = r.flip(1)
        outs.append((r / 255.0 - m) / s)
    return torch.stack(outs)


@pytest.mark.parametrize("flip", [False, True, "mixed"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_emulation_matches_interpolate(case, flip):
    from perceiver_io_amd.ops import emulation

    Hs, Ws, C, out_hw, boxes = CASES[case]
    flips = [bool(k % 2) for k in range(len(boxes))] if flip == "mixed" else [flip] * len(boxes)
    mean, std = (MEAN3, STD3) if C == 3 else ((0.5,), (0.5,))
    src = _src(len(boxes), Hs, Ws, C, seed=case)
    got = emulation.batch_augment(src, _params(boxes, flips), mean, std, out_hw)
    assert got.dtype == torch.float32 and got.shape == (len(boxes),) + tuple(out_hw) + (C,) and got.is_contiguous()
    want = interpolate_reference(src, boxes, flips, mean, std, out_hw)
    gap = (got.double() - want).abs().max().item()
    print(f"case {case} flip {flip}: max |emulation - fp64 F.interpolate| = {gap:.3e}")
    assert gap <= AUGMENT_TOL, gap
    if flip is True:  # the flip really mirrors the columns
        plain = emulation.batch_augment(src, _params(boxes, [False] * len(boxes)), mean, std, out_hw)
        assert torch.equal(got, plain.flip(2))


def test_ops_batch_augment_dispatches_to_the_emulation_on_cpu():
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops import emulation

    Hs, Ws, C, out_hw, boxes = CASES[0]
    src = _src(len(boxes), Hs, Ws, C)
    p = _params(boxes, [True, False, True, False])
    assert torch.equal(ops.batch_augment(src, p, MEAN3, STD3, out_hw), emulation.batch_augment(src, p, MEAN3, STD3, out_hw))
    # one value for all channels
    assert torch.equal(ops.batch_augment(src, p, 0.5, [0.5], out_hw),
                       emulation.batch_augment(src, p, [0.5] * 3, [0.5] * 3, out_hw))
    with pytest.raises(ValueError):
        ops.batch_augment(src.float(), p, MEAN3, STD3, out_hw)
    with pytest.raises(ValueError):
        ops.batch_augment(src, p, (0.5, 0.5), STD3, out_hw)


def host_transform(u8, top, left, crop=24):
    """``_Transformed.__getitem__``'s arithmetic on one (28, 28) uint8 image"""
    x = u8.float() / 255.0
    x = x[top:top + crop, left:left + crop]
    x = (x - 0.5) / 0.5
    return x.unsqueeze(-1)


def test_copy_path_is_the_host_transform_bit_for_bit():
    from perceiver_io_amd import ops

    B = 16
    u8 = _src(B, 28, 28, 1, seed=3)
    u8[0] = torch.arange(784, dtype=torch.int64).remainder(256).to(torch.uint8).reshape(28, 28, 1)  # every byte value
    g = torch.Generator().manual_seed(4)
    tops = torch.randint(0, 5, (B,), generator=g).tolist()
    lefts = torch.randint(0, 5, (B,), generator=g).tolist()
    tops[:2], lefts[:2] = [0, 4], [4, 0]
    p = _params([(t, l, 24, 24) for t, l in zip(tops, lefts)], [False] * B)
    got = ops.batch_augment(u8, p, (0.5,), (0.5,), (24, 24))
    want = torch.stack([host_transform(u8[k, :, :, 0], tops[k], lefts[k]) for k in range(B)])
    assert torch.equal(got, want)
    # normalize=False: mean 0, std 1 leave v / 255
    got = ops.batch_augment(u8, p, (0.0,), (1.0,), (24, 24))
    want = torch.stack([(u8[k, :, :, 0].float() / 255.0)[tops[k]:tops[k] + 24, lefts[k]:lefts[k] + 24, None] for k in range(B)])
    assert torch.equal(got, want)


# overhanging every edge, h = 0, negative and NaN words → the explicitly clamped box (source 9 × 11)
NAN = float("nan")
CLAMP_CASES = [
    ((-3.0, 2.0, 5.0, 4.0), (0, 2, 5, 4)),        # above the top edge: the offset counts as 0
    ((2.0, -1.0, 3.0, 6.0), (2, 0, 3, 6)),        # left of the left edge
    ((6.0, 2.0, 7.0, 4.0), (6, 2, 3, 4)),         # past the bottom edge: the height shrinks
    ((1.0, 8.0, 4.0, 9.0), (1, 8, 4, 3)),         # past the right edge
    ((12.0, 15.0, 3.0, 3.0), (8, 10, 1, 1)),      # wholly outside: the last pixel
    ((2.0, 3.0, 0.0, 4.0), (2, 3, 1, 4)),         # h = 0
    ((2.0, 3.0, 4.0, -5.0), (2, 3, 4, 1)),        # negative width
    ((NAN, 3.0, 4.0, 4.0), (0, 3, 4, 4)),         # NaN offset
    ((2.0, NAN, NAN, 4.0), (2, 0, 1, 4)),         # NaN offset and size
    ((2.0, 3.0, 4.0, NAN), (2, 3, 4, 1)),
    ((0.0, 0.0, 1e9, 1e9), (0, 0, 9, 11)),        # huge sizes: the whole image
    ((float("inf"), float("-inf"), float("inf"), 3.0), (8, 0, 1, 3)),
]


def clamp_params(flag=0.0):
    raw = torch.zeros(len(CLAMP_CASES), 8)
    good = torch.zeros(len(CLAMP_CASES), 8)
    for k, (r, c) in enumerate(CLAMP_CASES):
        raw[k, :4] = torch.tensor(r)
        good[k, :4] = torch.tensor(c, dtype=torch.float32)
        raw[k, 4] = good[k, 4] = flag if k % 2 else 0.0
    return raw, good


@pytest.mark.parametrize("out_hw", [(4, 5), (1, 1)])
def test_boxes_are_clamped_into_the_source(out_hw):
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops import emulation

    raw, good = clamp_params(flag=1.0)
    src = _src(len(CLAMP_CASES), 9, 11, 3, seed=5)
    y0, x0, h, w, _ = emulation.augment_boxes(raw, 9, 11)
    assert torch.stack([y0, x0, h, w], 1).tolist() == [list(c) for _, c in CLAMP_CASES]
    got = ops.batch_augment(src, raw, MEAN3, STD3, out_hw)
    assert torch.isfinite(got).all()
    assert torch.equal(got, ops.batch_augment(src, good, MEAN3, STD3, out_hw))
    # a NaN flip word does not flip
    p = good.clone()
    p[:, 4] = NAN
    q = good.clone()
    q[:, 4] = 0.0
    assert torch.equal(ops.batch_augment(src, p, MEAN3, STD3, out_hw), ops.batch_augment(src, q, MEAN3, STD3, out_hw))


# ---- DeviceAugment.draw ------------------------------------------------------------------------
def test_draw_random_crop():
    from perceiver_io_amd.data.augment import DeviceAugment

    aug = DeviceAugment((28, 28), (24, 24), mode="random_crop", hflip=0.5)
    a = aug.draw(np.random.default_rng(7), 500, True)
    b = aug.draw(np.random.default_rng(7), 500, True)
    assert a.dtype == np.float32 and a.shape == (500, 8) and np.array_equal(a, b)
    assert not np.array_equal(a, aug.draw(np.random.default_rng(8), 500, True))
    assert (a[:, 2] == 24).all() and (a[:, 3] == 24).all() and (a[:, 5:] == 0).all()
    assert set(np.unique(a[:, 0])) == set(range(5)) and set(np.unique(a[:, 1])) == set(range(5))  # uniform on 0..4
    assert set(np.unique(a[:, 4])) == {0.0, 1.0} and 0.4 < a[:, 4].mean() < 0.6
    e = aug.draw(np.random.default_rng(7), 9, False)
    assert (e == np.array([2, 2, 24, 24, 0, 0, 0, 0], dtype=np.float32)).all()  # centred, unflipped, constant
    assert (DeviceAugment((28, 28), (24, 24)).draw(np.random.default_rng(7), 64, True)[:, 4] == 0).all()
    with pytest.raises(ValueError):
        DeviceAugment((28, 28), (32, 32), mode="random_crop")
    with pytest.raises(ValueError):
        DeviceAugment((28, 28), (24, 24), mode="center")


@pytest.mark.parametrize("source_hw", [(256, 256), (200, 320)])
def test_draw_random_resized_crop(source_hw):
    from perceiver_io_amd.data.augment import DeviceAugment

    H, W = source_hw
    scale, ratio = (0.08, 1.0), (3 / 4, 4 / 3)
    aug = DeviceAugment(source_hw, (224, 224), mode="random_resized_crop", scale=scale, ratio=ratio, hflip=0.5)
    n = 2000
    p = aug.draw(np.random.default_rng(11), n, True)
    assert np.array_equal(p, aug.draw(np.random.default_rng(11), n, True))
    y0, x0, h, w = (p[:, k].astype(np.int64) for k in range(4))
    assert (p[:, :4] == np.stack([y0, x0, h, w], 1)).all()  # integers stored as floats
    assert (y0 >= 0).all() and (x0 >= 0).all() and (h >= 1).all() and (w >= 1).all()
    assert (y0 + h <= H).all() and (x0 + w <= W).all()
    fb = np.array(aug.fallback_box())
    accepted = ~(np.stack([y0, x0, h, w], 1) == fb).all(1)
    assert accepted.sum() > 0.9 * n
    # w = round(√(A·r)), h = round(√(A/r)): the real-valued sides lie within ±0.5 px of (h, w), so
    # the box's area and ratio lie within the products / quotients of the widened sides
    hh, ww = h[accepted].astype(np.float64), w[accepted].astype(np.float64)
    area_lo, area_hi = (hh - 0.5) * (ww - 0.5) / (H * W), (hh + 0.5) * (ww + 0.5) / (H * W)
    ratio_lo, ratio_hi = (ww - 0.5) / (hh + 0.5), (ww + 0.5) / (hh - 0.5)
    assert (area_hi >= scale[0]).all() and (area_lo <= scale[1]).all()
    assert (ratio_hi >= ratio[0]).all() and (ratio_lo <= ratio[1]).all()
    frac = hh * ww / (H * W)
    assert frac.min() < 0.2 and frac.max() > 0.6  # the draws span the scale range
    assert 0.4 < p[:, 4].mean() < 0.6
    # evaluation: constant, unflipped, centred, eval_crop_pct of the shorter side
    e = aug.draw(np.random.default_rng(1), 5, False)
    side = int(round(0.875 * min(H, W)))
    assert (e == np.array([(H - side) // 2, (W - side) // 2, side, side, 0, 0, 0, 0], dtype=np.float32)).all()


def test_draw_falls_back_when_nothing_fits():
    from perceiver_io_amd.data.augment import DeviceAugment

    aug = DeviceAugment((64, 64), (32, 32), mode="random_resized_crop", scale=(1.0, 1.0), ratio=(8.0, 8.0))
    p = aug.draw(np.random.default_rng(2), 300, True)
    assert aug.fallback_box() == (28, 0, 8, 64)  # the whole width at ratio 8, centred
    assert (p[:, :4] == np.array([28, 0, 8, 64], dtype=np.float32)).all()
    tall = DeviceAugment((64, 64), (32, 32), mode="random_resized_crop", scale=(1.0, 1.0), ratio=(0.125, 0.125))
    assert tall.fallback_box() == (0, 28, 64, 8)
    # the aspect ratio of out_hw in evaluation
    wide = DeviceAugment((100, 200), (32, 64), mode="random_resized_crop", eval_crop_pct=0.8)
    assert wide.eval_box() == (30, 60, 40, 80)


def test_apply_runs_the_op():
    from perceiver_io_amd.data.augment import DeviceAugment
    from perceiver_io_amd.ops import emulation

    aug = DeviceAugment((9, 11), (4, 5), mode="random_resized_crop", hflip=0.5, mean=MEAN3, std=STD3)
    src = _src(6, 9, 11, 3)
    p = aug.draw(np.random.default_rng(0), 6, True)
    assert torch.equal(aug.apply(src, p), emulation.batch_augment(src, torch.from_numpy(p), MEAN3, STD3, (4, 5)))


# ---- data modules ------------------------------------------------------------------------------
def test_mnist_device_augment_yields_raw_uint8():
    from perceiver_io_amd.data import MNISTDataModule

    dm = MNISTDataModule(synthetic=True, synthetic_size=48, val_split=16, random_crop=24, device_augment=True,
                         batch_size=8, num_workers=0, hflip=0.25)
    assert dm.image_shape == (24, 24, 1)
    dm.setup()
    x, y = next(iter(dm.train_dataloader()))
    assert x.dtype == torch.uint8 and tuple(x.shape) == (8, 28, 28, 1) and y.dtype == torch.int64
    xv, _ = next(iter(dm.val_dataloader()))
    assert xv.dtype == torch.uint8 and tuple(xv.shape) == (8, 28, 28, 1)
    a = dm.augment
    assert a.mode == "random_crop" and a.source_hw == (28, 28) and a.out_hw == (24, 24) and a.hflip == 0.25
    assert a.mean == [0.5] and a.std == [0.5]
    assert MNISTDataModule(synthetic=True, device_augment=True, normalize=False).augment.std == [1.0]
    with pytest.raises(ValueError):
        MNISTDataModule(synthetic=True, device_augment=True, channels_last=False)
    # the default is the host pipeline, unchanged
    host = MNISTDataModule(synthetic=True, synthetic_size=48, val_split=16, random_crop=24, batch_size=8, num_workers=0)
    host.setup()
    assert host.augment is None and "device_augment" not in host.hparams
    xh, _ = next(iter(host.val_dataloader()))
    assert xh.dtype == torch.float32 and tuple(xh.shape) == (8, 24, 24, 1)
    # the device path's evaluation batch is the host pipeline's, bit for bit
    assert torch.equal(a.apply(xv, a.draw(np.random.default_rng(0), 8, False)), xh)


def test_synthetic_image_module_device_augment():
    from perceiver_io_amd.data import SyntheticImageDataModule

    dm = SyntheticImageDataModule(image_shape=(16, 16, 3), num_classes=5, size=8, batch_size=4, num_workers=0,
                                  device_augment=True)
    dm.setup()
    x, y = next(iter(dm.train_dataloader()))
    assert x.dtype == torch.uint8 and tuple(x.shape) == (4, 48, 48, 3) and dm.image_shape == (16, 16, 3)
    assert dm.augment.mode == "random_resized_crop" and dm.augment.source_hw == (48, 48) and dm.augment.hflip == 0.5
    out = dm.augment.apply(x, dm.augment.draw(np.random.default_rng(0), 4, True))
    assert tuple(out.shape) == (4, 16, 16, 3) and out.abs().max() <= 1.0
    assert SyntheticImageDataModule(image_shape=(16, 16, 3), size=8).augment is None


def test_npy_image_module_round_trip(tmp_path):
    from perceiver_io_amd.data import DATAMODULE_REGISTRY, NpyImageDataModule

    assert DATAMODULE_REGISTRY["NpyImageDataModule"] is NpyImageDataModule
    rng = np.random.default_rng(0)
    ti, tl = rng.integers(0, 256, (10, 12, 14, 3), dtype=np.uint8), rng.integers(0, 4, 10)
    vi, vl = rng.integers(0, 256, (6, 12, 14, 3), dtype=np.uint8), rng.integers(0, 4, 6)
    for name, arr in (("train_images", ti), ("train_labels", tl), ("val_images", vi), ("val_labels", vl)):
        np.save(tmp_path / f"{name}.npy", arr)
    dm = NpyImageDataModule(str(tmp_path), image_shape=(8, 8, 3), num_classes=4, batch_size=4, num_workers=0,
                            shuffle=False)
    dm.prepare_data()
    dm.setup()
    assert dm.image_shape == (8, 8, 3) and dm.augment.source_hw == (12, 14) and dm.augment.out_hw == (8, 8)
    batches = list(dm.train_dataloader())
    assert [tuple(b[0].shape) for b in batches] == [(4, 12, 14, 3), (4, 12, 14, 3), (2, 12, 14, 3)]
    assert batches[0][0].dtype == torch.uint8
    assert np.array_equal(torch.cat([b[0] for b in batches]).numpy(), ti)
    assert torch.cat([b[1] for b in batches]).tolist() == tl.tolist()
    xv, yv = next(iter(dm.val_dataloader()))
    assert np.array_equal(xv.numpy(), vi[:4]) and yv.tolist() == vl[:4].tolist()
    with pytest.raises(FileNotFoundError):
        NpyImageDataModule(str(tmp_path / "missing")).prepare_data()


# ---- task module and CLI -------------------------------------------------------------------------
def _tiny_img(**kw):
    from perceiver_io_amd.tasks import LitImageClassifier

    return LitImageClassifier(image_shape=(24, 24, 1), num_classes=10,
                              optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3}},
                              num_latents=8, num_latent_channels=64, num_encoder_layers=1,
                              num_encoder_self_attention_layers_per_block=1, num_frequency_bands=4, **kw)


def test_eager_step_equals_the_host_transformed_step_bitwise():
    from perceiver_io_amd.data.augment import DeviceAugment

    torch.manual_seed(0)
    lit = _tiny_img(label_smoothing=0.1, mixup_alpha=0.8, cutmix_alpha=1.0)
    lit.train()
    aug = DeviceAugment((28, 28), (24, 24), mode="random_crop")
    u8 = _src(6, 28, 28, 1, seed=9)
    y = torch.randint(0, 10, (6,))
    p = aug.draw(np.random.default_rng(3), 6, True)
    xh = torch.stack([host_transform(u8[k, :, :, 0], int(p[k, 0]), int(p[k, 1])) for k in range(6)])
    mix = torch.tensor([2.0, 1.0 - 8 * 12 / 576.0, 5.0, 13.0, 10.0, 22.0])
    with pytest.raises(RuntimeError, match="no augmenter"):
        lit.step((u8, y, mix, torch.from_numpy(p)))
    lit.augment = aug
    for m in (mix, torch.tensor([1.0, 0.3, 0.0, 0.0, 0.0, 0.0])):
        l_dev, a_dev = lit.step((u8, y, m, torch.from_numpy(p)))
        l_host, a_host = lit.step((xh, y, m))
        assert torch.equal(l_dev, l_host) and torch.equal(a_dev, a_host)
    # hard-label path (options off) and evaluation (the centred draw, made in the step)
    plain = _tiny_img()
    plain.augment = aug
    plain.train()
    assert torch.equal(plain.step((u8, y, None, torch.from_numpy(p)))[0], plain.step((xh, y))[0])
    plain.eval()
    xe = torch.stack([host_transform(u8[k, :, :, 0], 2, 2) for k in range(6)])
    with torch.no_grad():
        assert torch.equal(plain.step([u8, y])[0], plain.step([xe, y])[0])
    # graph_batch: (x, y, mix | None, aug) for raw batches, today's layouts otherwise
    gb = plain.graph_batch([u8, y])
    assert len(gb) == 4 and gb[2] is None and tuple(gb[3].shape) == (6, 8) and gb[3].dtype == torch.float32
    assert (gb[3][:, 2:4] == 24).all()
    gb = lit.graph_batch([u8, y])
    assert len(gb) == 4 and tuple(gb[2].shape) == (6,) and tuple(gb[3].shape) == (6, 8)
    assert len(lit.graph_batch([xh, y])) == 3 and len(plain.graph_batch([xh, y])) == 2


def _run_cli(task, tmp_path, *flags):
    from perceiver_io_amd.cli.tasks import main as cli_main

    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        return cli_main(task, list(flags))
    finally:
        os.chdir(old)


def test_cli_fit_with_device_augment(tmp_path, monkeypatch):
    """4 CPU steps (precision 32, eager) of the smallest MNIST-shape classifier on raw uint8 batches
    with MixUp / CutMix and label smoothing on: one augmentation per training and validation batch,
    finite losses."""
    from perceiver_io_amd import ops

    calls = []
    real = ops.batch_augment

    def counted(src, params, mean, std, out_hw):
        calls.append((tuple(src.shape), src.dtype, tuple(params.shape), tuple(out_hw), bool((params[:, 0] == 2).all())))
        return real(src, params, mean, std, out_hw)

    monkeypatch.setattr(ops, "batch_augment", counted)
    cli = _run_cli("img_clf", tmp_path, "fit", "--data=MNISTDataModule", "--data.synthetic=true",
                   "--data.synthetic_size=48", "--data.batch_size=8", "--data.num_workers=0", "--data.val_split=16",
                   "--data.random_crop=24", "--data.device_augment=true",
                   "--optimizer.lr=0.001", "--trainer.accelerator=cpu", "--trainer.precision=32", "--trainer.max_epochs=1",
                   "--trainer.limit_train_batches=4", "--trainer.limit_val_batches=2", "--trainer.log_every_n_steps=1",
                   "--trainer.num_sanity_val_steps=0", "--trainer.seed=5",
                   "--model.num_latents=8", "--model.num_latent_channels=64", "--model.num_encoder_layers=1",
                   "--model.num_encoder_self_attention_layers_per_block=1", "--model.num_frequency_bands=4",
                   "--model.label_smoothing=0.1", "--model.mixup_alpha=0.8", "--model.cutmix_alpha=1.0")
    tr = cli.trainer
    assert tr.global_step == 4
    assert tuple(cli.model.hparams.image_shape) == (24, 24, 1) and cli.datamodule.augment is not None
    m = tr.callback_metrics
    assert math.isfinite(m["train_loss"]) and math.isfinite(m["val_loss"])
    assert 0.0 <= m["train_acc"] <= 1.0 and 0.0 <= m["val_acc"] <= 1.0
    assert len(calls) == 6, calls  # 4 training + 2 validation batches
    assert all(c[:4] == ((8, 28, 28, 1), torch.uint8, (8, 8), (24, 24)) for c in calls)
    assert not all(c[4] for c in calls[:4]) and all(c[4] for c in calls[4:])  # random offsets, then the centred box
