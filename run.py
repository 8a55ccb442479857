#!/usr/bin/env python
"""LArTPC per-pixel semantic segmentation with Perceiver IO (reference ``run.py``).

512×512 single-plane wire images → 3 classes per pixel (background / track / shower).  The
model is the reference's (``perceiver_io_amd/models/lartpc.py``): Fourier-encoded image input,
32×64 latents, 3 layers × (1 cross + 3 self-attention), one decoder query per pixel, a 3-way
classifier, and a U-ResNet built alongside (unused, as in the reference).  Training follows
the reference: weighted cross-entropy with background weight 0, Adam (lr 1e-3, L2 weight decay
1e-4), grad-norm clip 10, ReduceLROnPlateau(patience 5000, factor 0.1) stepped on the training
loss, batch 4, per-class accuracies, validation each epoch, and a checkpoint
``{'epoch', 'model_state_dict', 'optimizer_state_dict'}``.

On a GPU the default is the MI355X path:

* **sparse execution** (``models/lartpc.py``).  The encoder sees only the non-zero pixels and
  the decoder only the weighted pixels.  Loss and gradients are the same as the dense model's.
  Pass ``--dense`` to run all 262,144 keys and queries, the reference's cost.
* **fused kernels + hipGraph step** (``StepEngine``).  One graph is captured per capacity bucket.
  ``FusedAdam`` does the coupled-L2 Adam update and the clip in one kernel pass.
  ReduceLROnPlateau reads the previous step's loss, so the host never waits on the step in
  flight.  The reference steps it on the current loss; with patience 5000 the one-step lag
  changes nothing in practice.

``--device-collate`` moves batch building onto the device (``LArPerceiver.event_loss``): the
loaders only stack dense events (fp32 image, uint8 labels), and ``ops.event_compact`` builds the
sparse batch inside the step at fixed capacities, so training captures exactly one graph.
``--augment {flip,dihedral}`` adds flips and 90° turns for free: one int32 code per sample is drawn
on the host and the compaction reads the pixels through it (validation runs code 0).  Unset
``--key-capacity`` / ``--query-capacity`` are sized by one counting pass over both loaders.  Pixels
past a capacity are dropped from the loss, and every log step that sees an overflow says so.

``--focal-gamma G``, ``--dice-weight D``, ``--ce-weight W`` and ``--dice-eps E`` replace the weighted
cross-entropy by ``W`` · focal cross-entropy (γ = ``G``) + ``D`` · soft Dice, the two usual losses for
data this unbalanced (``ops.pixel_head.pixel_seg_loss``).  Training and validation use it on every
path: the fused head kernels on the sparse ones, an eager composition of the same definition with
``--dense``.  The two component values and the per-class Dice coefficients are logged beside the
accuracies.  With none of the four given, nothing changes.

``--engine eager`` (the default on CPU) runs the reference sequence exactly: zero_grad,
forward, ``scheduler.step(loss)``, backward, ``clip_grad_norm_``, ``Adam.step``.

Documented differences: a synthetic track/shower generator stands in for the larcv/ROOT
reader (``data/synthetic.py:lartpc_event``), because larcv and ROOT are not available.
Logits are permuted to (B, 3, H·W) instead of reshaped (defect D6).  Metrics go to
tfevents/JSONL.  With the fused optimizer, ``optimizer_state_dict`` covers the trained (Perceiver)
parameters.  The unused U-ResNet never has a gradient, and torch's Adam skips it too.

    python run.py [--epochs 10] [--events 64] [--size 512] [--batch-size 4] [--dense] [--engine eager]
    python run.py --device-collate --augment dihedral [--key-capacity K] [--query-capacity Q]
    python run.py --focal-gamma 2 --dice-weight 0.5 [--ce-weight 1] [--dice-eps 1]

``--segment CKPT --out DIR`` trains nothing: it loads ``model_state_dict`` from the checkpoint,
segments the validation events through ``LArPerceiver.segment`` (sparse, no dense logits) and
writes one uint8 H×W class map ``event_<i>.npy`` per event, then prints the per-class IoU.

    python run.py --segment ckpt/model_9.ckpt --out segmented [--val-events 8] [--size 512]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from perceiver_io_amd.data.lartpc import DenseCollator, DihedralAugment, SparseCollator, _round_up  # noqa: E402
from perceiver_io_amd.data.synthetic import SyntheticLArTPC  # noqa: E402
from perceiver_io_amd.models.lartpc import LArPerceiver, SegLoss, accuracies, class_weights, iou  # noqa: E402
from perceiver_io_amd.ops.emulation import check_seg_params  # noqa: E402
from perceiver_io_amd.ops.pixel_head import seg_loss_logits  # noqa: E402
from perceiver_io_amd.train.loggers import TensorBoardLogger  # noqa: E402

__all__ = ["LArPerceiver", "accuracies", "main"]


def _to(batch, dev):
    return tuple(t.to(dev, non_blocking=True) for t in batch)


def make_step_fn(model, weights, sparse: bool, metrics: dict, seg=None):
    """loss_fn(batch) → loss; per-class accuracies of the batch land in ``metrics`` (device).  With
    ``seg`` (a ``SegLoss``) the loss is focal cross-entropy + soft Dice, and its two component
    values and the per-class Dice coefficients land there too."""

    def loss_fn(batch):
        if sparse:
            loss, acc = model.sparse_loss(batch, weights, seg)
        else:
            img, lab = batch
            out = model(img)
            if seg is None:
                loss = F.cross_entropy(out, lab, weight=weights)
                acc = accuracies(out.argmax(1).detach(), lab)
            else:  # logits exist here: the same definition as an eager composition
                loss, acc = seg_loss_logits(out.permute(0, 2, 1), lab, weights, *seg)
        metrics.update(acc)
        return loss

    return loss_fn


def make_event_step_fn(model, weights, caps, metrics: dict, side: dict, seg=None):
    """loss_fn((img, lab, words)) → loss of ``--device-collate``; accuracies land in ``metrics``, the
    batch's true key / query counts (B, 2) in ``side`` (device tensors).  ``seg``: as in
    :func:`make_step_fn`."""

    def loss_fn(batch):
        loss, acc, counts = model.event_loss(batch, weights, caps[0], caps[1], loss=seg)
        metrics.update(acc)
        side["counts"] = counts
        return loss

    return loss_fn


def size_capacities(loaders, dev, bucket: int):
    """One counting pass (``event_compact`` with capacities 0) over ``loaders``: the largest key and
    query count of any event, kept on the device and read once, rounded up to ``bucket``."""
    from perceiver_io_amd import ops
    from perceiver_io_amd.models.lartpc import CLASS_WEIGHTS

    top = torch.zeros(2, dtype=torch.int32, device=dev)
    for loader in loaders:
        for img, lab in loader:
            words = torch.zeros(img.shape[0], dtype=torch.int32, device=dev)
            counts = ops.event_compact(img.to(dev), lab.to(dev), words, 0, 0, CLASS_WEIGHTS)[5]
            top = torch.maximum(top, counts.max(0).values)
    k, q = top.tolist()  # the only read
    return _round_up(k, bucket), _round_up(q, bucket)


def report_overflow(counts, caps, step: int) -> None:
    """Print the pixels a batch lost to the capacities (never silent)."""
    k, q = counts.max(0).values.tolist()
    if k > caps[0] or q > caps[1]:
        c = counts.long()
        lost_k = int((c[:, 0] - caps[0]).clamp(min=0).sum())
        lost_q = int((c[:, 1] - caps[1]).clamp(min=0).sum())
        print(f"step {step}: capacity overflow, dropped {lost_k} key and {lost_q} query pixels "
              f"(largest event {k} keys / {q} queries, capacities {caps[0]} / {caps[1]})", flush=True)


def segment_events(model, a, dev):
    """``--segment``: ``event_<i>.npy`` (uint8 H×W class map: the class of every non-zero pixel, 0
    elsewhere) for each validation event, and the per-class IoU against the synthetic labels."""
    import numpy as np

    state = torch.load(a.segment, map_location=dev, weights_only=True)
    model.load_state_dict(state["model_state_dict"])
    model.eval()
    os.makedirs(a.out, exist_ok=True)
    val = torch.utils.data.DataLoader(SyntheticLArTPC(a.val_events, a.size, seed=1), batch_size=a.batch_size)
    confusion, n = None, 0
    for img, lab in val:
        seg = model.segment(img.to(dev), bucket=a.bucket, labels=lab.to(dev))
        confusion = seg.confusion if confusion is None else confusion + seg.confusion
        for m in seg.class_map.cpu().numpy():
            np.save(os.path.join(a.out, f"event_{n}.npy"), m.reshape(a.size, a.size))
            n += 1
    per, mean = iou(confusion)
    names = ("background", "track", "shower")
    print(f"segmented {n} events -> {a.out}", flush=True)
    print("IoU: " + ", ".join(f"{k} {float(v):.4f}" for k, v in zip(names, per)) + f", mean {float(mean):.4f}", flush=True)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--val-events", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--max-steps", type=int, default=-1)
    ap.add_argument("--log-dir", default="runs")
    ap.add_argument("--ckpt-dir", default="ckpt")
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--engine", choices=["auto", "graph", "eager"], default="auto",
                    help="graph: fused kernels + hipGraph step (GPU default); eager: the reference sequence")
    ap.add_argument("--dense", action="store_true", help="evaluate all pixels (the reference's cost)")
    ap.add_argument("--bucket", type=int, default=2048, help="sparse capacity rounding (keys / queries)")
    ap.add_argument("--log-every", type=int, default=1)
    ap.add_argument("--workers", type=int, default=1)
    ap.add_argument("--device-collate", action="store_true",
                    help="build the sparse batch on the device at fixed capacities (one captured graph)")
    ap.add_argument("--augment", choices=["none", "flip", "dihedral"], default="none",
                    help="flips / 90-degree turns read through the compaction (needs --device-collate)")
    ap.add_argument("--key-capacity", type=int, default=None, help="key slots per event (default: counted, rounded to --bucket)")
    ap.add_argument("--query-capacity", type=int, default=None, help="query slots per event (default: counted)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the augmentation draws")
    ap.add_argument("--focal-gamma", type=float, default=None, help="focal exponent of the cross-entropy term (default 0)")
    ap.add_argument("--ce-weight", type=float, default=None, help="weight of the (focal) cross-entropy term (default 1)")
    ap.add_argument("--dice-weight", type=float, default=None, help="weight of the soft-Dice term (default 0)")
    ap.add_argument("--dice-eps", type=float, default=None, help="smoothing of the soft-Dice coefficients (default 1)")
    ap.add_argument("--segment", metavar="CKPT", default=None,
                    help="no training: segment the validation events with this checkpoint and write class maps to --out")
    ap.add_argument("--out", metavar="DIR", default="segmented", help="output directory of --segment")
    a = ap.parse_args(argv)
    if a.augment != "none" and not a.device_collate:
        ap.error("--augment needs --device-collate")
    if a.device_collate and a.dense:
        ap.error("--device-collate builds sparse batches: drop --dense")
    given = (a.focal_gamma, a.ce_weight, a.dice_weight, a.dice_eps)
    a.seg_loss = None  # none of the four given: the weighted cross-entropy, exactly as before
    if any(v is not None for v in given):
        a.seg_loss = SegLoss(*(d if v is None else v for v, d in zip(given, SegLoss())))
        try:
            check_seg_params(*a.seg_loss)
        except ValueError as e:
            ap.error(str(e))
    return a


def make_loaders(a):
    """(train, validation) loaders: the host collator by default, dense stacks with --device-collate."""
    collate = DenseCollator() if a.device_collate else SparseCollator(a.bucket) if not a.dense else None
    kw = dict(num_workers=a.workers, persistent_workers=a.workers > 0, collate_fn=collate)
    train = torch.utils.data.DataLoader(SyntheticLArTPC(a.events, a.size, seed=0), batch_size=a.batch_size,
                                        shuffle=True, drop_last=True, **kw)
    val = torch.utils.data.DataLoader(SyntheticLArTPC(a.val_events, a.size, seed=1), batch_size=a.batch_size,
                                      drop_last=True, collate_fn=collate)
    return train, val


def main(argv=None):
    a = parse_args(argv)
    dev = torch.device(a.device)
    torch.manual_seed(0)
    model = LArPerceiver(a.size).to(dev)
    if a.segment is not None:
        return segment_events(model, a, dev)
    weights = class_weights(dev)
    sparse = not a.dense
    train, val = make_loaders(a)
    fused = dev.type == "cuda" and a.engine != "eager"
    if fused:
        from perceiver_io_amd.ops.optim import FusedAdam
        from perceiver_io_amd.train.engine import StepEngine

        opt = FusedAdam(model.trained_parameters(), lr=a.lr, weight_decay=1e-4, max_grad_norm=10.0)
    else:
        opt = torch.optim.Adam(model.parameters(), lr=a.lr, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, patience=5000, factor=0.1)
    metrics: dict = {}
    side: dict = {}  # --device-collate: the batch's counts, a static output of the captured graph
    caps, aug, rng = None, None, None
    if a.device_collate:
        caps = (a.key_capacity, a.query_capacity)
        if None in caps:
            counted = size_capacities((train, val), dev, a.bucket)
            caps = tuple(c if c is not None else n for c, n in zip(caps, counted))
        print(f"device collate: {caps[0]} key and {caps[1]} query slots per event, augment {a.augment}", flush=True)
        aug, rng = DihedralAugment(a.augment), DihedralAugment.rng(a.seed, 0)
        loss_fn = make_event_step_fn(model, weights, caps, metrics, side, a.seg_loss)
    else:
        loss_fn = make_step_fn(model, weights, sparse, metrics, a.seg_loss)
    if a.seg_loss is not None:
        print("loss: {1:g} x focal CE (gamma {0:g}) + {2:g} x soft Dice (eps {3:g})".format(*a.seg_loss), flush=True)

    def with_words(batch, training: bool):
        if aug is None:
            return batch
        return (*batch, torch.from_numpy(aug.draw(rng, batch[0].shape[0], training)))

    engine = None
    if fused:
        engine = StepEngine(loss_fn, opt, None, device=dev, graph=True,
                            state_hooks=(lambda: (dict(metrics), dict(side)),
                                         lambda s: (metrics.update(s[0]), side.update(s[1]))))
    log = TensorBoardLogger(a.log_dir, name="lartpc")
    step, epoch, prev = 0, 0, None
    t_start, n_timed = None, 0
    for epoch in range(a.epochs):
        model.train()
        for batch in train:
            batch = _to(with_words(batch, True), dev)
            t0 = time.perf_counter()
            if fused:
                loss = engine.step(batch)
                if prev is not None:
                    sched.step(float(prev))  # the previous step's loss: no wait on this one
                prev = loss
            else:
                opt.zero_grad()
                loss = loss_fn(batch)
                sched.step(loss.item())  # stepped before backward, like the reference
                loss.backward()
                torch.nn.utils.clip_grad_norm_(model.parameters(), 10)
                opt.step()
            if step == 2:  # throughput after graph capture / allocator warm-up
                if dev.type == "cuda":
                    torch.cuda.synchronize()
                t_start, n_timed = time.perf_counter(), 0
            elif t_start is not None:
                n_timed += a.batch_size
            if step % a.log_every == 0:
                vals = {k: float(v) for k, v in metrics.items()}
                log.log_metrics({"loss": float(loss), "lr": opt.param_groups[0]["lr"],
                                 **{f"train_{k}": v for k, v in vals.items()}}, step)
                parts = "".join(f" {k} {vals[k]:.4f}" for k in ("focal", "dice") if k in vals)
                print(f"epoch {epoch} step {step} loss {float(loss):.4f}{parts} acc {vals.get('acc', 0):.3f} "
                      f"{time.perf_counter() - t0:.3f}s", flush=True)
                if caps is not None:
                    report_overflow(side["counts"], caps, step)
            step += 1
            if 0 < a.max_steps <= step:
                break
        model.eval()
        vl, va, vs = [], [], {}
        with torch.no_grad():
            for batch in val:
                batch = _to(with_words(batch, False), dev)
                vm: dict = {}
                if caps is not None:
                    vl.append(float(make_event_step_fn(model, weights, caps, vm, {}, a.seg_loss)(batch)))
                else:
                    vl.append(float(make_step_fn(model, weights, sparse, vm, a.seg_loss)(batch)))
                va.append(float(vm["acc"]))
                for k, v in vm.items():  # the new loss's components and per-class Dice
                    if k == "focal" or k.startswith("dice"):
                        vs.setdefault(k, []).append(float(v))
        if vl:
            log.log_metrics({"validation_loss": sum(vl) / len(vl), "val_acc": sum(va) / len(va),
                             **{f"val_{k}": sum(v) / len(v) for k, v in vs.items()}}, step)
            print(f"validation loss: {sum(vl) / len(vl):.4f}", flush=True)
        if 0 < a.max_steps <= step:
            break
    if t_start is not None and n_timed:
        if dev.type == "cuda":
            torch.cuda.synchronize()
        print(f"throughput: {n_timed / (time.perf_counter() - t_start):.1f} samples/s "
              f"({'sparse' if sparse else 'dense'}, {'fused graph' if fused else 'eager'}"
              f"{', device collate' if caps is not None else ''})", flush=True)
    if engine is not None and caps is not None:
        print(f"captured training graphs: {engine.num_graphs}", flush=True)
    os.makedirs(a.ckpt_dir, exist_ok=True)
    torch.save({"epoch": epoch, "model_state_dict": model.state_dict(), "optimizer_state_dict": opt.state_dict()},
               os.path.join(a.ckpt_dir, f"model_{epoch}.ckpt"))
    log.close()


if __name__ == "__main__":
    main()
