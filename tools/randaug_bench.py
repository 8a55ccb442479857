"""Device-side RandAugment (``csrc/randaugment.hip``): the kernels alone, their floors, the training
step with and without them, and the host cost they replace.

(a) ``rand_augment`` with N = 2 layers at 32 × 256 × 256 × 3 and 128 × 28 × 28 × 1 under the worst-case
    op mix (every sample equalizes twice: both launches of both layers do their full work) and a
    typical one (``RandAugment(magnitude=9).draw``), against a ``copy_`` of the image bytes and the
    bytes-moved floor: a layer reads and writes the batch once (2 · N · bytes; a statistics layer
    reads it once more), at the HBM peak of ``--peak-gbps``;
(b) ``img_clf fit`` steps/s on the captured-graph path with ``device_augment=true``, with and without
    ``rand_augment_ops=2``: synthetic MNIST (batch 128) and a pre-decoded random 256 × 256 × 3 uint8
    set through ``NpyImageDataModule`` (batch 32); ``--steps`` steps timed after ``--warmup`` steps;
(c) if PIL imports: the per-sample host time of the same two drawn operations done with PIL
    (``ImageOps`` / ``ImageEnhance`` / ``Image.transform``), what a loader worker would spend.

Device events around ``--iters`` calls after ``--kwarmup`` calls; the sides alternate in ``--rounds``
rounds and the median round is reported with the min–max spread.  Needs a GPU.

    python tools/randaug_bench.py [--parts abc] [--steps 200] [--warmup 50] [--out profiles/randaugment.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.augment_bench import _ab, _fmt, _StepTimer  # noqa: E402

KERNEL_SHAPES = {"imagenet": (32, 256, 256, 3), "mnist": (128, 28, 28, 1)}
STATS_OPS = (4, 8, 9)


def _words(kind, B, H, W):
    from perceiver_io_amd.data.augment import RandAugment

    if kind == "drawn":
        return torch.from_numpy(RandAugment((H, W), num_ops=2, magnitude=9).draw(np.random.default_rng(0), B, True))
    w = torch.zeros(B, 2, 8)
    w[..., 0], w[..., 2], w[..., 6] = 9.0, 1.0, 1.0  # equalize twice
    return w


def bench_kernel(a, K):
    rows = []
    for name, shape in KERNEL_SHAPES.items():
        B, H, W, C = shape
        g = torch.Generator().manual_seed(0)
        src = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).cuda()
        dst = torch.empty_like(src)
        nbytes = src.numel()
        words = {k: _words(k, B, H, W).cuda() for k in ("equalize", "drawn")}
        fns = {k: (lambda w=w: K.rand_augment(src, w, 0)) for k, w in words.items()}
        fns["copy_"] = lambda: dst.copy_(src)
        r = _ab(fns, a.iters, a.kwarmup, a.rounds)
        row = dict(config=name, shape=list(shape), layers=2, image_bytes=nbytes, us=r)
        msg = f"kernel {name:8s}:"
        for k, w in words.items():
            stats = int(sum((w[..., 0] == op).sum() for op in STATS_OPS))  # layers that read their input twice
            moved = 2 * 2 * nbytes + stats * (nbytes // B)
            row[f"{k}_bytes_moved"] = moved
            row[f"{k}_GBps"] = moved / (r[k][0] * 1e-6) / 1e9
            row[f"{k}_floor_us"] = moved / (a.peak_gbps * 1e9) * 1e6
            msg += f"   {_fmt(r, k)} ({row[f'{k}_GBps']:.0f} GB/s, floor {row[f'{k}_floor_us']:.1f} us)"
        row["copy_GBps"] = 2 * nbytes / (r["copy_"][0] * 1e-6) / 1e9
        print(msg + f"   {_fmt(r, 'copy_')} ({row['copy_GBps']:.0f} GB/s)", flush=True)
        rows.append(row)
    return rows


FIT_CASES = {
    "mnist": (128, ["--data=MNISTDataModule", "--data.synthetic=true", "--data.synthetic_size=42000",
                    "--data.batch_size=128", "--data.random_crop=24", "--data.device_augment=true"]),
    "imagenet_npy": (32, ["--data=NpyImageDataModule", "--data.batch_size=32", "--data.num_classes=1000"]),
}
NPY_IMAGES = 512


def _write_npy_set(root):
    rng = np.random.default_rng(0)
    for split, n in (("train", NPY_IMAGES), ("val", 64)):
        np.save(os.path.join(root, f"{split}_images.npy"), rng.integers(0, 256, (n, 256, 256, 3), dtype=np.uint8))
        np.save(os.path.join(root, f"{split}_labels.npy"), rng.integers(0, 1000, n))


def bench_fit(a):
    from perceiver_io_amd.cli.tasks import _model_class, task_cli

    rows = []
    for name, (batch, flags) in FIT_CASES.items():
        row = dict(config=name, batch=batch, steps=a.steps, warmup=a.warmup)
        with tempfile.TemporaryDirectory() as tmp:
            if "npy" in name:
                _write_npy_set(tmp)
                flags = flags + [f"--data.data_dir={tmp}"]
            for side, extra in (("plain", []), ("rand_augment", ["--data.rand_augment_ops=2"])):
                args = ["fit", *flags, *extra, "--trainer.accelerator=gpu", "--trainer.devices=1",
                        f"--trainer.max_steps={a.warmup + a.steps}", "--trainer.max_epochs=1000",
                        "--trainer.limit_val_batches=0", "--trainer.num_sanity_val_steps=0",
                        "--trainer.enable_checkpointing=false", "--trainer.enable_progress_bar=false",
                        f"--trainer.default_root_dir={tmp}"]
                cli = task_cli("img_clf")(_model_class("img_clf"), run=False, args=args, save_config=False)
                timer = _StepTimer(a.warmup, a.steps)
                cli.trainer.callbacks.append(timer)
                cli.run_fit()
                eng = cli.trainer._engine
                row[side] = dict(steps_per_sec=timer.steps_per_sec, step_us=1e6 / timer.steps_per_sec,
                                 graphs=eng.num_graphs, replays=eng.replays)
                del cli
                torch.cuda.empty_cache()
        print(f"fit {name:12s}:" + "".join(f"   {s} {row[s]['steps_per_sec']:8.1f} steps/s ({row[s]['step_us']:.0f} us)"
                                           for s in ("plain", "rand_augment")), flush=True)
        rows.append(row)
    return rows


def _pil_layer(im, word, fill):
    from PIL import Image, ImageEnhance, ImageOps

    op, v = int(word[0]), float(word[1])
    if op == 1:
        return im.transform(im.size, Image.AFFINE, [float(m) for m in word[2:]], Image.NEAREST,
                            fillcolor=fill if im.mode == "L" else (fill,) * 3)
    if 2 <= op <= 5:
        enh = (ImageEnhance.Brightness, ImageEnhance.Color, ImageEnhance.Contrast, ImageEnhance.Sharpness)[op - 2]
        return enh(im).enhance(v)
    if op == 6:
        return ImageOps.posterize(im, max(1, int(v)))
    return {7: lambda: ImageOps.solarize(im, v), 8: lambda: ImageOps.autocontrast(im), 9: lambda: ImageOps.equalize(im)
            }.get(op, lambda: im)()


def bench_pil(a):
    try:
        from PIL import Image
    except ImportError:
        print("PIL not installed: host comparison not measured", flush=True)
        return None
    rows = []
    for name, (B, H, W, C) in KERNEL_SHAPES.items():
        rng = np.random.default_rng(0)
        imgs = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
        ims = [Image.fromarray(i[..., 0], "L") if C == 1 else Image.fromarray(i, "RGB") for i in imgs]
        row = dict(config=name, shape=[B, H, W, C])
        for kind in ("equalize", "drawn"):
            words = _words(kind, B, H, W).numpy()
            t = []
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                for im, w in zip(ims, words):
                    for layer in w:
                        im = _pil_layer(im, layer, 0)
                    np.asarray(im)
                t.append((time.perf_counter() - t0) / B * 1e6)
            row[f"{kind}_us_per_sample"] = float(np.median(t))
        print(f"PIL {name:8s}: equalize {row['equalize_us_per_sample']:.1f} us / sample, drawn "
              f"{row['drawn_us_per_sample']:.1f} us / sample (one host thread)", flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parts", default="abc", help="which parts to run: a (kernels, floors), b (fit), c (PIL)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kwarmup", type=int, default=20, help="warm-up calls of part (a)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200, help="timed training steps per side of part (b)")
    ap.add_argument("--warmup", type=int, default=50, help="training steps before the timed ones")
    ap.add_argument("--peak-gbps", type=float, default=8000.0, help="HBM peak the bytes-moved floor is taken at")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("randaug_bench needs a GPU: timings from anything else say nothing")
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops import ext

    K = ext.require()
    res = dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=a.rounds, peak_gbps=a.peak_gbps)
    if "a" in a.parts:
        res["kernel"] = bench_kernel(a, K)
    if "b" in a.parts:
        res["fit"] = bench_fit(a)
    if "c" in a.parts:
        res["pil"] = bench_pil(a)
    ops.check_device_errors()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
