"""Device-side image augmentation (``csrc/augment.hip``): the kernel alone, its floor, and the
loader-bound training rate with the transforms on the host and on the device.

(a) ``batch_augment`` at 128 × 28 × 28 × 1 → 24 × 24 (the MNIST ``random_crop``, copy path) and
    32 × 256 × 256 × 3 → 224 × 224 (random-resized crops with flips): time and achieved bytes/s
    (source box bytes read + output bytes written), against the ATen composition on the same device
    tensors: per-sample slice, ``F.interpolate``, flip, normalize;
(b) a ``copy_`` of the same number of output bytes: the floor of anything that writes that output;
(c) ``img_clf fit`` steps/s over the real ``DataLoader`` with the host transforms and with
    ``device_augment=true``, for synthetic MNIST (``random_crop=24``, batch 128) and for
    ``SyntheticImageDataModule`` (batch 32): ``--steps`` steps timed after ``--warmup`` steps.  The
    synthetic ImageNet-shape loader computes every image in its workers, so a third row runs
    ``NpyImageDataModule`` (device path only) over a pre-decoded random 256 × 256 × 3 uint8 set;
    ``bench.py --config mnist / imagenet`` (synthetic device batches, no loader) is the ceiling and is
    run separately in the same session; pass its samples/s with ``--ceiling mnist=… imagenet=…``.

Device events around ``--iters`` calls after ``--kwarmup`` calls; the sides alternate in ``--rounds``
rounds and the median round is reported with the min–max spread.  Needs a GPU.

    python tools/augment_bench.py [--parts abc] [--steps 200] [--warmup 50] [--out profiles/augment.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from perceiver_io_amd.train.callbacks import Callback  # noqa: E402

KERNEL_CASES = {
    "mnist": dict(src=(128, 28, 28, 1), out=(24, 24), mode="random_crop", hflip=0.0, mean=[0.5], std=[0.5]),
    "imagenet": dict(src=(32, 256, 256, 3), out=(224, 224), mode="random_resized_crop", hflip=0.5,
                     mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225]),
}


def _time(fn, iters):
    """mean µs per call over ``iters`` calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def _ab(fns, iters, warmup, rounds):
    """{name: (median µs, min, max)} of the alternated sides"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            t[n].append(_time(fn, iters))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in t.items()}


def _fmt(r, n):
    return f"{n} {r[n][0]:8.1f} us [{r[n][1]:.1f}, {r[n][2]:.1f}]"


def bench_kernel(a, K):
    from perceiver_io_amd.data.augment import DeviceAugment

    rows = []
    for name, c in KERNEL_CASES.items():
        B, Hs, Ws, C = c["src"]
        oh, ow = c["out"]
        g = torch.Generator().manual_seed(0)
        src = torch.randint(0, 256, c["src"], dtype=torch.uint8, generator=g).cuda()
        aug = DeviceAugment((Hs, Ws), (oh, ow), mode=c["mode"], hflip=c["hflip"], mean=c["mean"], std=c["std"])
        ph = aug.draw(np.random.default_rng(0), B, True)
        p = torch.from_numpy(ph).cuda()
        boxes = [tuple(int(v) for v in row[:4]) + (bool(row[4] >= 0.5),) for row in ph]
        mean = torch.tensor(c["mean"], device="cuda")
        std = torch.tensor(c["std"], device="cuda")

        def fused():
            return K.batch_augment(src, p, c["mean"], c["std"], oh, ow)

        def aten():  # the boxes are host integers here: the composition cannot read them from the device
            outs = []
            for k, (y0, x0, h, w, flip) in enumerate(boxes):
                crop = src[k, y0:y0 + h, x0:x0 + w].permute(2, 0, 1)[None].float()
                if (h, w) != (oh, ow):
                    crop = F.interpolate(crop, size=(oh, ow), mode="bilinear", align_corners=False, antialias=False)
                r = crop[0].permute(1, 2, 0)
                outs.append(r.flip(1) if flip else r)
            return (torch.stack(outs) / 255.0 - mean) / std

        err = (fused() - aten()).abs().max().item()
        out_bytes = B * oh * ow * C * 4
        read_bytes = int(sum(h * w for _, _, h, w, _ in boxes)) * C
        flat_src = torch.empty(out_bytes // 4, device="cuda")
        flat_dst = torch.empty_like(flat_src)
        r = _ab({"batch_augment": fused, "aten": aten, "copy_": lambda: flat_dst.copy_(flat_src)},
                a.iters, a.kwarmup, a.rounds)
        gbs = (out_bytes + read_bytes) / (r["batch_augment"][0] * 1e-6) / 1e9
        copy_gbs = 2 * out_bytes / (r["copy_"][0] * 1e-6) / 1e9
        rows.append(dict(config=name, src=list(c["src"]), out=[oh, ow], us=r, out_bytes=out_bytes, box_bytes_read=read_bytes,
                         batch_augment_GBps=gbs, copy_GBps=copy_gbs, max_abs_diff_vs_aten=err))
        print(f"kernel {name:8s}: {_fmt(r, 'batch_augment')} ({gbs:.0f} GB/s)   {_fmt(r, 'aten')}   "
              f"{_fmt(r, 'copy_')} ({copy_gbs:.0f} GB/s)   max |diff| vs ATen {err:.1e}", flush=True)
    return rows


class _StepTimer(Callback):
    """Trainer callback: wall time of steps (warmup, warmup + steps], the device drained at both ends."""

    def __init__(self, warmup, steps):
        self.warmup, self.steps = warmup, steps
        self.t0 = self.t1 = None

    def on_train_batch_end(self, trainer, module):
        if trainer.global_step == self.warmup:
            torch.cuda.synchronize()
            self.t0 = time.perf_counter()
        elif trainer.global_step == self.warmup + self.steps:
            torch.cuda.synchronize()
            self.t1 = time.perf_counter()

    @property
    def steps_per_sec(self):
        return self.steps / (self.t1 - self.t0)


# name → (ceiling config, batch, sides, flags)
FIT_CASES = {
    "mnist": ("mnist", 128, ("host", "device"),
              ["--data=MNISTDataModule", "--data.synthetic=true", "--data.synthetic_size=42000",
               "--data.batch_size=128", "--data.random_crop=24"]),
    "imagenet": ("imagenet", 32, ("host", "device"),
                 ["--data=SyntheticImageDataModule", "--data.batch_size=32", "--data.size=10000"]),
    "imagenet_npy": ("imagenet", 32, ("device",),
                     ["--data=NpyImageDataModule", "--data.batch_size=32", "--data.num_classes=1000",
                      "--data.mean=[0.485,0.456,0.406]", "--data.std=[0.229,0.224,0.225]"]),
    "imagenet_npy_w8": ("imagenet", 32, ("device",),
                        ["--data=NpyImageDataModule", "--data.batch_size=32", "--data.num_classes=1000",
                         "--data.num_workers=8"]),
}
NPY_IMAGES = 2048


def _write_npy_set(root):
    rng = np.random.default_rng(0)
    for split, n in (("train", NPY_IMAGES), ("val", 64)):
        np.save(os.path.join(root, f"{split}_images.npy"), rng.integers(0, 256, (n, 256, 256, 3), dtype=np.uint8))
        np.save(os.path.join(root, f"{split}_labels.npy"), rng.integers(0, 1000, n))


def bench_fit(a, ceilings):
    from perceiver_io_amd.cli.tasks import _model_class, task_cli

    rows = []
    for name, (ceil_name, batch, sides, flags) in FIT_CASES.items():
        row = dict(config=name, batch=batch, steps=a.steps, warmup=a.warmup)
        for side in sides:
            with tempfile.TemporaryDirectory() as tmp:
                if "npy" in name:
                    _write_npy_set(tmp)
                    flags = flags + [f"--data.data_dir={tmp}"]
                args = ["fit", *flags, *(["--data.device_augment=true"] if side == "device" and "npy" not in name else []),
                        "--trainer.accelerator=gpu", "--trainer.devices=1", f"--trainer.max_steps={a.warmup + a.steps}",
                        "--trainer.max_epochs=1000", "--trainer.limit_val_batches=0", "--trainer.num_sanity_val_steps=0",
                        "--trainer.enable_checkpointing=false", "--trainer.enable_progress_bar=false",
                        f"--trainer.default_root_dir={tmp}"]
                cli = task_cli("img_clf")(_model_class("img_clf"), run=False, args=args, save_config=False)
                timer = _StepTimer(a.warmup, a.steps)
                cli.trainer.callbacks.append(timer)
                cli.run_fit()
                eng = cli.trainer._engine
                row[side] = dict(steps_per_sec=timer.steps_per_sec, samples_per_sec=timer.steps_per_sec * batch,
                                 graphs=eng.num_graphs, replays=eng.replays,
                                 num_workers=cli.datamodule.num_workers)
                del cli
                torch.cuda.empty_cache()
        ceil = ceilings.get(ceil_name)
        row["ceiling_samples_per_sec"] = ceil
        msg = f"fit {name:12s}:"
        for side in sides:
            msg += f"   {side} {row[side]['steps_per_sec']:8.1f} steps/s ({row[side]['samples_per_sec']:.0f} img/s)"
            if ceil:
                row[f"{side}_fraction_of_ceiling"] = row[side]["samples_per_sec"] / ceil
                msg += f" = {100 * row[side]['samples_per_sec'] / ceil:.1f} % of the ceiling {ceil:.0f} img/s"
        print(msg, flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parts", default="abc", help="which parts to run: a and b (kernel, floor), c (fit)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kwarmup", type=int, default=20, help="warm-up calls of parts (a) and (b)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200, help="timed training steps per side of part (c)")
    ap.add_argument("--warmup", type=int, default=50, help="training steps before the timed ones")
    ap.add_argument("--ceiling", nargs="*", default=[], metavar="CONFIG=SAMPLES_PER_SEC",
                    help="bench.py's samples/s of the same session, e.g. mnist=156000 imagenet=20000")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs a GPU: timings from anything else say nothing")
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops import ext

    K = ext.require()
    ceilings = {k: float(v) for k, v in (c.split("=", 1) for c in a.ceiling)}
    res = dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=a.rounds)
    if "a" in a.parts or "b" in a.parts:
        res["kernel"] = bench_kernel(a, K)
    if "c" in a.parts:
        res["fit"] = bench_fit(a, ceilings)
    ops.check_device_errors()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
