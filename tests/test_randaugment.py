"""RandAugment on raw uint8 batches, CPU side: ``emulation.rand_augment`` (the definition the kernels
of ``csrc/randaugment.hip`` are compared with) against PIL, its degenerate inputs, the host draws
of ``data.augment.RandAugment`` and the data-module / task-module wiring."""
import math

import numpy as np
import pytest
import torch

# (H, W, C) of the PIL comparisons: odd sizes in colour, a small grey image
PIL_SHAPES = [(33, 20, 3), (16, 16, 1)]
BAD_OPS = (float("nan"), -1.0, 10.0, 2.5)


def _emu():
    from perceiver_io_amd.ops import emulation

    return emulation


def image(H, W, C, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + H * 131 + W * 17 + C)
    return torch.randint(0, 256, (H, W, C), dtype=torch.uint8, generator=g)


def word(op, v=0.0, m=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0)):
    return torch.tensor([float(op), float(v), *[float(a) for a in m]], dtype=torch.float32)


def run(img, *words, fill=0):
    """The layers ``words`` on one (H, W, C) uint8 image."""
    return _emu().rand_augment(img[None], torch.stack(list(words))[None], fill)[0]


def to_pil(img):
    from PIL import Image

    a = img.numpy()
    return Image.fromarray(a[..., 0], "L") if a.shape[2] == 1 else Image.fromarray(a, "RGB")


def from_pil(im):
    a = np.asarray(im)
    return torch.from_numpy(a.reshape(a.shape[0], a.shape[1], -1).copy())


def degenerate_cases():
    """(name, image, words, expected) shared with the GPU file: inputs on which an operation must
    leave the image unchanged."""
    const = torch.full((6, 5, 3), 77, dtype=torch.uint8)
    small = image(9, 7, 3, seed=4)  # n = 63 < 255 pixels: equalize's step is 0
    cases = [("constant_autocontrast", const, [word(8)], const),
             ("constant_equalize", const, [word(9)], const),
             ("small_equalize", small, [word(9)], small),
             ("sharpness_1x1", image(1, 1, 3, seed=5), [word(5, 1.7)], image(1, 1, 3, seed=5)),
             ("sharpness_2x2", image(2, 2, 1, seed=6), [word(5, 0.2)], image(2, 2, 1, seed=6))]
    for k, bad in enumerate(BAD_OPS):
        img = image(5, 7, 3, seed=10 + k)
        cases.append((f"bad_op_{bad}", img, [word(bad, 0.5, (0.5, 0.1, 1.0, 0.0, 2.0, 0.0))], img))
    return cases


# ---- the emulation against PIL ------------------------------------------------------------------
@pytest.mark.parametrize("shape", PIL_SHAPES)
def test_posterize_solarize_equalize_equal_pil(shape):
    ImageOps = pytest.importorskip("PIL.ImageOps")
    img = image(*shape)
    for bits in (1, 4, 7, 8):
        assert torch.equal(run(img, word(6, bits)), from_pil(ImageOps.posterize(to_pil(img), bits))), bits
    for thr in (0, 77, 128, 255):
        assert torch.equal(run(img, word(7, thr)), from_pil(ImageOps.solarize(to_pil(img), thr))), thr
    assert torch.equal(run(img, word(9)), from_pil(ImageOps.equalize(to_pil(img))))
    # a skewed histogram with an empty top end: another last non-zero bin, another step
    dark = (img.to(torch.int32) * img.to(torch.int32) // 400).to(torch.uint8)
    assert dark.max() < 200
    assert torch.equal(run(dark, word(9)), from_pil(ImageOps.equalize(to_pil(dark))))


@pytest.mark.parametrize("shape", PIL_SHAPES)
def test_enhancements_within_one_level_of_pil(shape):
    """PIL evaluates these in double precision or with another final rounding: one grey level is
    the quantisation step."""
    ImageOps = pytest.importorskip("PIL.ImageOps")
    from PIL import ImageEnhance

    img = image(*shape)
    narrow = (img // 3 + 40).to(torch.uint8)  # lo = 40, hi ≤ 125: autocontrast has work to do
    gap = (run(narrow, word(8)).int() - from_pil(ImageOps.autocontrast(to_pil(narrow))).int()).abs().max().item()
    print(f"{shape} autocontrast: max |emulation - PIL| = {gap}")
    assert gap <= 1
    for op, enh in ((2, ImageEnhance.Brightness), (3, ImageEnhance.Color), (4, ImageEnhance.Contrast),
                    (5, ImageEnhance.Sharpness)):
        for f in (0.1, 0.73, 1.0, 1.27, 1.9):
            want = from_pil(enh(to_pil(img)).enhance(f))
            gap = (run(img, word(op, f)).int() - want.int()).abs().max().item()
            print(f"{shape} op {op} factor {f}: max |emulation - PIL| = {gap}")
            assert gap <= 1, (op, f, gap)


def affine_cases(H, W):
    """Inverse matrices (m00, m01, m02, m10, m11, m12) about the centre: an integer translation, a
    shear and a rotation."""
    cx, cy = W / 2.0, H / 2.0
    th = math.radians(31.0)
    c, s = math.cos(th), math.sin(th)
    # the small offsets keep every sampling coordinate away from the integers (asserted below)
    return {"translate": (1.0, 0.0, -3.0, 0.0, 1.0, 2.0),
            "shear": (1.0, 0.2734375, -0.2734375 * cy + 0.37, 0.0, 1.0, 0.0),
            "rotate": (c, -s, cx - c * cx + s * cy + 0.413, s, c, cy - s * cx - c * cy + 0.337)}


@pytest.mark.parametrize("shape", PIL_SHAPES)
@pytest.mark.parametrize("name", ["translate", "shear", "rotate"])
def test_affine_equals_pil_nearest(shape, name):
    pytest.importorskip("PIL")
    from PIL import Image

    H, W, C = shape
    m = affine_cases(H, W)[name]
    # precondition, in float64: no sampling coordinate within 1e-3 of an integer, so neither fp32
    # rounding nor PIL's fixed-point coefficients can move a floor
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    for a, b, t in (m[:3], m[3:]):
        s = a * jj + b * ii + t
        assert np.abs(s - np.rint(s)).min() > 1e-3, name
    img = image(*shape, seed=2)
    fill = 9
    want = to_pil(img).transform((W, H), Image.AFFINE, m, Image.NEAREST, fillcolor=fill if C == 1 else (fill,) * 3)
    got = run(img, word(1, 0.0, m), fill=fill)
    assert torch.equal(got, from_pil(want))
    assert (got == fill).any() and (got != fill).any()  # part of the output lies outside the source


def test_affine_rejects_unusable_coordinates():
    img = image(5, 7, 3, seed=3)
    for m in ((float("nan"),) * 6, (1e30,) * 6, (1.0, 0.0, float("inf"), 0.0, 1.0, 0.0), (-1e30, 0, 0, 0, 1, 0)):
        assert (run(img, word(1, 0.0, m), fill=200) == 200).all(), m


# ---- degenerate inputs and layer order ----------------------------------------------------------
@pytest.mark.parametrize("case", degenerate_cases(), ids=lambda c: c[0])
def test_degenerate_inputs_are_left_unchanged(case):
    _, img, words, want = case
    assert torch.equal(run(img, *words), want)


def test_layers_run_in_order_on_uint8_intermediates():
    img = image(20, 21, 3, seed=8)  # n = 420 pixels: equalize's step is 1
    a, b = word(7, 100.0), word(9)
    assert torch.equal(run(img, a, b), run(run(img, a), b))
    assert not torch.equal(run(img, a, b), run(img, b, a))
    # color on a grey image is a copy
    grey = image(6, 6, 1, seed=1)
    assert torch.equal(run(grey, word(3, 1.8)), grey)


def test_ops_rand_augment_dispatches_to_the_emulation_on_cpu():
    from perceiver_io_amd import ops

    src = torch.stack([image(8, 6, 3, seed=k) for k in range(3)])
    words = torch.stack([torch.stack([word(k + 6, 3.0), word(9)]) for k in range(3)])
    assert torch.equal(ops.rand_augment(src, words), _emu().rand_augment(src, words))
    for bad in (lambda: ops.rand_augment(src.float(), words),
                lambda: ops.rand_augment(src[..., :2].contiguous(), words),  # two channels
                lambda: ops.rand_augment(src.permute(0, 2, 1, 3), words),    # not contiguous
                lambda: ops.rand_augment(src, words[:2]),
                lambda: ops.rand_augment(src, words[:, :, :6]),
                lambda: ops.rand_augment(src, words, fill=256)):
        with pytest.raises(ValueError):
            bad()


# ---- host draws ------------------------------------------------------------------------------------
def test_draw_shape_dtype_determinism_and_coverage():
    from perceiver_io_amd.data.augment import RandAugment

    ra = RandAugment((32, 24), num_ops=2, magnitude=9)
    w = ra.draw(np.random.default_rng(5), 2048, True)
    assert w.shape == (2048, 2, 8) and w.dtype == np.float32
    assert np.array_equal(w, ra.draw(np.random.default_rng(5), 2048, True))
    assert not np.array_equal(w, ra.draw(np.random.default_rng(6), 2048, True))
    assert set(np.unique(w[..., 0]).tolist()) == set(float(k) for k in range(10))  # 4,096 draws
    # both signs of a signed operation, and only shears / translations / rotations move pixels
    bright = w[..., 1][w[..., 0] == 2]
    assert (bright > 1).any() and (bright < 1).any()
    ident = np.array([1, 0, 0, 0, 1, 0], dtype=np.float32)
    assert (w[..., 2:][w[..., 0] != 1] == ident).all()
    ev = ra.draw(np.random.default_rng(5), 16, False)
    assert ev.shape == (16, 2, 8) and (ev[..., 0] == 0).all() and (ev[..., 2:] == ident).all()
    for bad in (dict(num_ops=0), dict(num_ops=9), dict(magnitude=31), dict(magnitude=-1), dict(fill=256)):
        with pytest.raises(ValueError):
            RandAugment((32, 24), **bad)


def test_draw_magnitude_zero_is_identity_equivalent():
    from perceiver_io_amd.data.augment import RandAugment

    w = RandAugment((32, 24), num_ops=3, magnitude=0).draw(np.random.default_rng(1), 512, True)
    assert (w[..., 2:] == np.array([1, 0, 0, 0, 1, 0], dtype=np.float32)).all()
    enh = (w[..., 0] >= 2) & (w[..., 0] <= 5)
    assert enh.any() and (w[..., 1][enh] == 1.0).all()


@pytest.mark.parametrize("magnitude,bits,thresh", [(0, 8, 255.0), (9, 7, 178.5), (30, 4, 0.0)])
def test_draw_posterize_and_solarize_follow_the_table(magnitude, bits, thresh):
    """torchvision: posterize keeps 8 − round(m / 7.5) bits, the solarize threshold is
    linspace(255, 0, 31)[m]."""
    from perceiver_io_amd.data.augment import RandAugment

    w = RandAugment((32, 24), magnitude=magnitude).draw(np.random.default_rng(2), 1024, True)
    post, sol = w[..., 1][w[..., 0] == 6], w[..., 1][w[..., 0] == 7]
    assert post.size and sol.size
    assert (post == bits).all() and np.allclose(sol, thresh, rtol=0, atol=1e-4)


def test_drawn_geometry():
    from perceiver_io_amd.data.augment import RA_NAMES, RandAugment

    H, W = 15, 11
    ra = RandAugment((H, W), num_ops=1, magnitude=30)
    w = ra.draw(np.random.default_rng(3), 4096, True)[:, 0]
    aff = w[w[:, 0] == 1]
    # the 2 × 2 parts seen: shears ±0.3, whole-pixel translations, rotations by ±30°
    lin = {tuple(np.round(r, 4)) for r in aff[:, [2, 3, 5, 6]].astype(np.float64)}
    c, s = round(math.cos(math.radians(30)), 4), round(math.sin(math.radians(30)), 4)
    assert lin == {(1, 0.3, 0, 1), (1, -0.3, 0, 1), (1, 0, 0.3, 1), (1, 0, -0.3, 1), (1, 0, 0, 1), (c, -s, s, c),
                   (c, s, -s, c)}
    shifts = aff[(aff[:, [2, 3, 5, 6]] == np.array([1, 0, 0, 1], dtype=np.float32)).all(1)][:, [4, 7]]
    tx, ty = int(150.0 / 331.0 * W), int(150.0 / 331.0 * H)
    assert {tuple(r) for r in shifts.tolist()} == {(tx, 0), (-tx, 0), (0, ty), (0, -ty)}
    assert len(RA_NAMES) == 14
    # every drawn matrix maps the centre of the image to itself, so a rotation keeps the centre
    # pixel of a centred symmetric pattern
    yy, xx = torch.meshgrid(torch.arange(H) - H // 2, torch.arange(W) - W // 2, indexing="ij")
    pat = ((yy.abs() + xx.abs()) * 9 + 3).to(torch.uint8)[..., None]
    rot = [r for r in aff if abs(r[2] - c) < 1e-3]
    assert rot
    for r in rot[:4]:
        out = run(pat, torch.from_numpy(r))
        assert out[H // 2, W // 2, 0] == pat[H // 2, W // 2, 0] == 3
        assert not torch.equal(out, pat)
    # a translation by (tx, 0) moves the image right and fills the left columns
    right = run(pat, word(1, 0.0, (1, 0, -tx, 0, 1, 0)), fill=255)
    assert torch.equal(right[:, tx:], pat[:, :W - tx]) and (right[:, :tx] == 255).all()


# ---- data modules and task module --------------------------------------------------------------
def test_data_modules_take_the_options(tmp_path):
    from perceiver_io_amd.data import MNISTDataModule, NpyImageDataModule, SyntheticImageDataModule

    with pytest.raises(ValueError, match="device_augment"):
        MNISTDataModule(synthetic=True, rand_augment_ops=2)
    with pytest.raises(ValueError, match="device_augment"):
        SyntheticImageDataModule(image_shape=(8, 8, 3), rand_augment_ops=2)
    dm = MNISTDataModule(synthetic=True, device_augment=True, random_crop=24, rand_augment_ops=2, rand_augment_magnitude=5,
                         rand_augment_fill=128)
    ra = dm.augment.rand_augment
    assert (ra.num_ops, ra.magnitude, ra.fill, ra.source_hw) == (2, 5, 128, (28, 28))
    assert dm.hparams["rand_augment_ops"] == 2 and dm.hparams["rand_augment_magnitude"] == 5
    # unset: nothing recorded, no member
    plain = MNISTDataModule(synthetic=True, device_augment=True, random_crop=24)
    assert plain.augment.rand_augment is None and not any(k.startswith("rand_augment") for k in plain.hparams)
    sm = SyntheticImageDataModule(image_shape=(8, 8, 3), device_augment=True, source_shape=(12, 10, 3), rand_augment_ops=3)
    assert sm.augment.rand_augment.num_ops == 3 and sm.augment.rand_augment.source_hw == (12, 10)
    assert not any(k.startswith("rand_augment") for k in
                   SyntheticImageDataModule(image_shape=(8, 8, 3), device_augment=True).hparams)
    for split, n in (("train", 6), ("val", 4)):
        np.save(tmp_path / f"{split}_images.npy", np.zeros((n, 10, 12, 3), dtype=np.uint8))
        np.save(tmp_path / f"{split}_labels.npy", np.zeros(n, dtype=np.int64))
    nm = NpyImageDataModule(str(tmp_path), image_shape=(8, 8, 3), num_workers=0, rand_augment_ops=2)
    nm.setup()
    assert nm.augment.rand_augment.source_hw == (10, 12) and nm.hparams["rand_augment_ops"] == 2
    nm = NpyImageDataModule(str(tmp_path), image_shape=(8, 8, 3), num_workers=0)
    nm.setup()
    assert nm.augment.rand_augment is None and "rand_augment_ops" not in nm.hparams


def _tiny_img(**kw):
    from perceiver_io_amd.tasks import LitImageClassifier

    return LitImageClassifier(image_shape=(12, 12, 1), num_classes=10,
                              optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3}},
                              num_latents=8, num_latent_channels=64, num_encoder_layers=1,
                              num_encoder_self_attention_layers_per_block=1, num_frequency_bands=4, **kw)


def test_task_module_carries_the_words():
    from perceiver_io_amd.data.augment import DeviceAugment, RandAugment

    torch.manual_seed(0)
    B = 6
    u8 = torch.stack([image(16, 16, 1, seed=k) for k in range(B)])
    y = torch.randint(0, 10, (B,))
    with_ra = DeviceAugment((16, 16), (12, 12), mode="random_crop", rand_augment=RandAugment((16, 16), num_ops=2))
    without = DeviceAugment((16, 16), (12, 12), mode="random_crop")
    lit = _tiny_img()
    lit.train()
    lit.augment = with_ra
    gb = lit.graph_batch([u8, y])
    assert len(gb) == 5 and gb[2] is None and tuple(gb[3].shape) == (B, 8)
    assert tuple(gb[4].shape) == (B, 2, 8) and gb[4].dtype == torch.float32
    # the step's input: rand_augment with the carried words on the source, then batch_augment
    x, _, _ = lit.inputs(gb)
    want = without.apply(_emu().rand_augment(u8, gb[4]), gb[3])
    assert torch.equal(x, want) and not torch.equal(x, without.apply(u8, gb[3]))
    assert math.isfinite(float(lit.step(gb)[0]))
    # a four-element batch: training draws the words in the step, evaluation applies none
    assert not torch.equal(lit.inputs((u8, y, None, gb[3]))[0], without.apply(u8, gb[3]))
    lit.eval()
    assert torch.equal(lit.inputs((u8, y, None, gb[3]))[0], without.apply(u8, gb[3]))
    # option unset: exactly today's batch and input
    plain = _tiny_img()
    plain.train()
    plain.augment = without
    gb4 = plain.graph_batch([u8, y])
    assert len(gb4) == 4 and gb4[2] is None and tuple(gb4[3].shape) == (B, 8)
    assert torch.equal(plain.inputs(gb4)[0], _emu().batch_augment(u8, gb4[3], [0.5], [0.5], (12, 12)))
    with pytest.raises(ValueError):
        without.apply(u8, gb4[3], gb[4])
    with pytest.raises(ValueError):
        DeviceAugment((16, 16), (12, 12), rand_augment=RandAugment((20, 16)))
