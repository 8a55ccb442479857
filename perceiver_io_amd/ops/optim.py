"""Flat parameter space + fused AdamW (SURVEY K-15, §5.8).

``FlatParameterSpace`` re-homes every trainable parameter into ONE contiguous fp32 buffer
(and its gradient into one fp32 buffer, with a bf16 shadow of the weights for the GEMM
kernels).  Consequences on MI355X:
  * the data-parallel all-reduce is one (or a few bucketed) RCCL call(s) over a flat
    buffer instead of ~190 per-tensor collectives (``parallel/reducer.py``);
  * the optimizer is a single kernel launch over the flat buffers that also refreshes the
    bf16 shadow (no per-step weight casts);
  * zeroing gradients is one memset;
  * parameters flagged ``_pio_replicate`` (the fused attention/MLP layers) are placed first
    and get an 8-way replicated gradient accumulator ``grad_rep`` (8, n_rep): the fused
    backward kernels add their per-row-tile weight-gradient partials into replica
    (tile mod 8), so no address takes more than 1/8 of the tiles' float atomics (same-address
    atomics serialise at the memory side); ``fold()`` adds the replicas into ``grad`` (and
    clears them) once per step, before the all-reduce / optimizer.

``FusedAdamW`` is a ``torch.optim.Optimizer`` (so ``torch.optim.lr_scheduler`` schedulers
such as ``OneCycleLR`` drive it through ``param_groups``) with torch.optim.AdamW semantics
and a torch-compatible ``state_dict`` layout (``exp_avg``/``exp_avg_sq``/``step`` per
parameter), so Lightning-layout checkpoints round-trip.  lr/betas/step live in a small
device tensor refreshed before each step, which keeps the update capturable in a hipGraph.
With several parameter groups (at most 8; ``lr``, ``weight_decay`` and ``eps`` per group, equal
``betas``) that tensor carries 4 more words per group and the update is ``adamw_grouped`` over
the chunk table of the flat buffer (csrc/optim.hip); one group runs the single-group kernel.
``param_groups`` builds the usual groups (no decay on 1-d tensors, a prefix → lr multiplier map).

``Lamb`` / ``FusedLamb`` add LAMB: the flat space knows where tensors begin (``offsets``), so the
fused update takes per-tensor trust ratios and per-tensor weight decay from chunk tables
(``lamb_tables``, csrc/lamb.hip; what the updates share on the device is csrc/optim_common.h).

``skip_nonfinite`` (every fused optimizer) puts a step guard in front of the update: one more small
launch judges the gradient's Σ g² on the device and an update whose gradient is not finite does not
happen — inside a replayed graph, with no host in the loop (csrc/health.hip).  ``tensor_stats`` adds
per-tensor gradient / weight norms on request (``request_stats``), the trainer's ``track_grad_norm``.

``WeightEMA`` keeps an exponential moving average of the weights as one more flat fp32 buffer,
updated by one launch behind the fused update and swapped in for evaluation (csrc/ema.hip).
"""
from __future__ import annotations

import contextlib
import math
from typing import Iterable, List, Optional

import torch

from . import emulation, ext

ALIGN = 64  # elements; keeps every parameter view 256-byte aligned


GRAD_REPLICAS = 8  # matches kGradReplicas in csrc/rowgemm.hip
MAX_GROUPS = 8  # parameter groups of a fused optimizer; matches kOptMaxGroups in csrc/optim_common.h


def _kernels(device):
    """The module the flat-space updates are launched from: the HIP extension on the GPU (an error if it
    is not built), its emulation on the CPU."""
    return ext.require() if device.type == "cuda" else emulation


class FlatParameterSpace:
    def __init__(self, params: Iterable[torch.nn.Parameter], with_shadow: Optional[bool] = None,
                 replicate: Optional[bool] = None):
        params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("no trainable parameters")
        dev = params[0].device
        self.device = dev
        if replicate is None:
            # the replicas only serve the in-kernel float-atomic gradient path; with per-tile
            # weight-gradient slabs (ops.fused.WGRAD_SLAB) they would stay zero
            from .fused import WGRAD_SLAB

            replicate = dev.type == "cuda" and not WGRAD_SLAB
        rep = [p for p in params if replicate and getattr(p, "_pio_replicate", False)]
        rep_ids = {id(p) for p in rep}
        # replicated parameters first (one contiguous region), then the rest in module order
        self.params: List[torch.nn.Parameter] = rep + [p for p in params if id(p) not in rep_ids]
        self.offsets = []
        off = 0
        for p in self.params:
            self.offsets.append(off)
            off += (p.numel() + ALIGN - 1) // ALIGN * ALIGN
        self.numel = off
        self.n_rep = self.offsets[len(rep)] if len(rep) < len(self.params) else off
        if not rep:
            self.n_rep = 0
        self.data = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grad_rep = torch.zeros(GRAD_REPLICAS, self.n_rep, dtype=torch.float32, device=dev) if rep else None
        if with_shadow is None:
            with_shadow = dev.type == "cuda"
        self.shadow = torch.zeros(off, dtype=torch.bfloat16, device=dev) if with_shadow else None
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                n = p.numel()
                self.data[o:o + n].copy_(p.detach().reshape(-1).float())
                p.data = self.data[o:o + n].view_as(p)
                p.grad = self.grad[o:o + n].view_as(p)
                p._pio_flat = True  # its gradient is a view of this flat buffer (ops/fused.py in-place paths)
                if self.grad_rep is not None and o < self.n_rep:
                    p._pio_grad_rep = self.grad_rep[:, o:o + n]  # (8, numel) replica view
        if self.shadow is not None:
            from .fused import weight_cache

            for p, o in zip(self.params, self.offsets):
                weight_cache.bind(p, self.shadow[o:o + p.numel()].view(p.shape))

    def fold(self):
        """grad[:n_rep] += Σ replicas; replicas ← 0 (no-op without replicated parameters)."""
        if self.grad_rep is None:
            return
        _kernels(self.device).fold_replicas(self.grad, self.grad_rep)

    def views(self, buf: torch.Tensor):
        return [buf[o:o + p.numel()].view(p.shape) for p, o in zip(self.params, self.offsets)]

    def zero_grad_buffers(self):
        """Zero the gradient buffer and its replicas (capturable; no Python-side view fixes)."""
        self.grad.zero_()
        if self.grad_rep is not None:
            self.grad_rep.zero_()

    def zero_grad(self):
        self.zero_grad_buffers()
        # re-attach views autograd may have replaced (e.g. a grad that was set to None)
        for p, o in zip(self.params, self.offsets):
            g = p.grad
            if g is None or g.data_ptr() != self.grad[o:o + 1].data_ptr():
                p.grad = self.grad[o:o + p.numel()].view_as(p)

    def check_views(self) -> bool:
        return all(p.grad is not None and p.grad.data_ptr() == self.grad[o:o + 1].data_ptr()
                   for p, o in zip(self.params, self.offsets))

    def bucket_ranges(self, bucket_bytes: int, hi: Optional[int] = None):
        """Split [0, hi) (default: the whole buffer) into contiguous ranges of about
        ``bucket_bytes`` at parameter boundaries, in reverse parameter order (gradients of late
        parameters are produced first in backward)."""
        cap = max(ALIGN, bucket_bytes // 4)
        hi = self.numel if hi is None else hi
        ranges = []
        for o in reversed(self.offsets):
            if o >= hi:
                continue
            if hi - o >= cap:
                ranges.append((o, hi))
                hi = o
        if hi > 0:
            ranges.append((0, hi))
        return ranges


class _HostRing:
    """Pinned host staging slots for per-step device hyper-parameters (no reuse before the
    copy that read a slot has completed)."""

    def __init__(self, n: int, width: int, device):
        self.slots = [torch.zeros(width, dtype=torch.float32).pin_memory() for _ in range(n)]
        self.events = [None] * n
        self.i = 0

    def push(self, values, dst: torch.Tensor):
        i = self.i
        self.i = (self.i + 1) % len(self.slots)
        if self.events[i] is not None:
            self.events[i].synchronize()
        s = self.slots[i]
        for j, v in enumerate(values):
            s[j] = float(v)
        dst.copy_(s, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[i] = ev


class FusedAdamW(torch.optim.Optimizer):
    """AdamW over a :class:`FlatParameterSpace` in one kernel (HIP) or its emulation (CPU).

    ``skip_nonfinite``: a step whose gradient is not finite (Σ g² inf or NaN, a finite gradient whose
    Σ g² overflows fp32 included) is skipped on the device: ``sumsq`` → ``step_guard`` → the update with
    the guard's words.  A skipped step leaves weights, moments and shadow as they are, still clears the
    gradient and still delivers the loss, and does not advance the bias corrections (they take the
    *effective* step: attempted − skipped, ``GradScaler``'s meaning of a skip), so a run with one
    poisoned step and a constant learning rate ends bit for bit where the run without that step ends.
    The host's schedules (``lr``, the EMA decay) are functions of the attempted step and keep advancing
    on skipped steps; an attached :class:`WeightEMA` is not gated either: the weights did not move, so
    it averages them once more, as an eager recipe behind ``GradScaler`` does.  :meth:`health` reads the
    counters.  With data parallelism the guard judges the all-reduced gradient, so every rank decides
    alike.  The guard needs the global norm: no per-bucket or range updates.

    ``tensor_stats``: per-tensor ‖g‖, ‖w‖, max|g| and non-finite counts (:meth:`request_stats`,
    :meth:`tensor_stats`; with ``skip_nonfinite`` also of the last skipped step,
    :meth:`skipped_tensor_stats`).  With both options off the optimizer has no extra launch, buffer or
    hyper word."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, max_grad_norm: float = 0.0, flat: Optional[FlatParameterSpace] = None,
                 skip_nonfinite: bool = False, tensor_stats: bool = False):
        if amsgrad:
            raise NotImplementedError("amsgrad is not supported by the fused optimizer")
        params = list(params)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False,
                        maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)
        super().__init__(params, defaults)
        G = len(self.param_groups)
        if G > MAX_GROUPS:
            raise ValueError(f"{type(self).__name__} supports at most {MAX_GROUPS} parameter groups, got {G}")
        for g in self.param_groups[1:]:
            if tuple(g["betas"]) != tuple(self.param_groups[0]["betas"]):
                raise ValueError(f"{type(self).__name__}: betas must be equal in every parameter group "
                                 f"(lr, weight_decay and eps are per group)")
        # always with the bf16 shadow the fused executor reads its GEMM operands from (also for the
        # CPU emulation: re-homed parameters do not share the flat buffer's version counter, so a
        # version-keyed weight cache would never see the in-place update)
        # Without ``flat`` the buffer is laid out in group order.  A caller that needs another order (the
        # Trainer keeps MODEL order, so the reducer's ready points stay contiguous ranges) passes its own
        # space over the same parameters: groups need not be contiguous in it.
        self.flat = flat if flat is not None else FlatParameterSpace(
            [p for g in self.param_groups for p in g["params"]], with_shadow=True)
        homed = {id(p) for p in self.flat.params}
        if any(p.requires_grad and id(p) not in homed for g in self.param_groups for p in g["params"]):
            raise ValueError(f"{type(self).__name__}: a trainable parameter of the groups is missing from `flat`")
        dev = self.flat.device
        self.exp_avg = torch.zeros(self.flat.numel, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(self.flat.numel, dtype=torch.float32, device=dev)
        # 8 global words; with several groups 4 more per group (lr, weight decay, eps, reserved)
        self.hyper = torch.zeros(8 if G == 1 else 8 + 4 * G, dtype=torch.float32, device=dev)
        # several groups: the chunk table of the flat buffer and tensor → group (csrc adamw_grouped_kernel)
        self.chunk_tab = self.tensor_group = None
        if G > 1:
            self.chunk_tab, self.tensor_group = group_tables(self.flat, self.param_groups)
        self.max_grad_norm = float(max_grad_norm)
        # the gradient's sum of squares as fixed-order per-block partials (sumsq → adamw norm_part):
        # no atomics, so the clip factor is bitwise reproducible in every mode
        self.skip_nonfinite, self.track_stats = bool(skip_nonfinite), bool(tensor_stats)
        self.norm_part = (torch.zeros(512, dtype=torch.float32, device=dev)
                          if self.max_grad_norm > 0 or self.skip_nonfinite else None)
        # the step guard's 8 words (csrc/optim_common.h), written by step_guard on the device
        self.guard = torch.zeros(8, dtype=torch.float32, device=dev) if self.skip_nonfinite else None
        self._stats_due = False
        if self.track_stats:
            self._build_stats_buffers()
        self.l2 = False  # decoupled decay (AdamW); FusedAdam sets the coupled L2 form
        self._step = 0
        self._ring = _HostRing(8, self.hyper.numel(), dev) if dev.type == "cuda" else None
        self.grad_scale = 1.0
        # bucket mode (set by the step engine with a data-parallel reducer): each gradient bucket
        # is updated by range_update right after its all-reduce lands, on the reducer's side
        # stream, so device_update has nothing left to do
        self.bucket_mode = False
        # set by the step engine around a captured update: the kernel also copies the step's
        # loss (loss_out[0]) into loss_out[1][hyper[7]] (see StepEngine's loss ring)
        self.loss_out = None
        self.loss_slot = 0
        self.ema = None  # attach_ema: a WeightEMA over self.flat, updated right behind every update

    def _build_stats_buffers(self):
        """The tables and buffers of ``tensor_stats``: the chunk table of the flat buffer (the one a
        grouped or LAMB update already has, else built here), tensor → (first chunk, chunks), the
        per-chunk scratch and the (T, 4) results (a second one for skipped steps with a guard)."""
        f = self.flat
        chunks, tensors = _cut_chunks(f.offsets, [p.numel() for p in f.params])
        if getattr(self, "chunk_tab", None) is None:
            self.chunk_tab = torch.tensor(chunks, dtype=torch.int64, device=f.device).reshape(-1, 3)
        self.stats_tensor_tab = torch.tensor(tensors, dtype=torch.int32, device=f.device).reshape(-1, 2)
        self.stats_part = torch.zeros(4 * len(chunks), dtype=torch.float32, device=f.device)
        self.stats = torch.zeros(len(tensors), 4, dtype=torch.float32, device=f.device)
        self.skip_stats = torch.zeros_like(self.stats) if self.skip_nonfinite else None

    # -- health -------------------------------------------------------------------------
    def health(self) -> dict:
        """The step guard's counters, one host read (a sync): ``skipped`` steps so far, ``consecutive``
        skipped steps ending at the last one, ``last_norm`` (the last step's gradient norm, the mean
        gradient's before clipping, non-finite as it came), ``last_finite_norm`` and
        ``last_skipped_step`` (1-based attempted step, 0: none)."""
        if self.guard is None:
            raise RuntimeError(f"{type(self).__name__}.health() needs skip_nonfinite=True")
        w = self.guard.tolist()
        return {"skipped": int(w[1]), "consecutive": int(w[2]), "last_norm": w[4], "last_finite_norm": w[5],
                "last_skipped_step": int(w[6])}

    def request_stats(self):
        """Make the next staged step a statistics step (``hyper[6]``): its update is preceded by the
        per-tensor statistics launches, read back with :meth:`tensor_stats`."""
        if not self.track_stats:
            raise RuntimeError(f"{type(self).__name__}.request_stats() needs tensor_stats=True")
        self._stats_due = True

    def tensor_stats(self) -> torch.Tensor:
        """(T, 4) fp32 per tensor of ``flat.params``, of the last statistics step: ‖g‖ (of the mean
        gradient, before clipping), ‖w‖ (before the update), max|g| (NaN elements ignored) and the
        number of non-finite gradient elements."""
        if not self.track_stats:
            raise RuntimeError(f"{type(self).__name__}.tensor_stats() needs tensor_stats=True")
        return self.stats

    def skipped_tensor_stats(self) -> torch.Tensor:
        """The same rows of the most recent skipped step (kept until the next skipped step)."""
        if not self.track_stats or self.skip_stats is None:
            raise RuntimeError(f"{type(self).__name__}.skipped_tensor_stats() needs tensor_stats=True and "
                               f"skip_nonfinite=True")
        return self.skip_stats

    def attach_ema(self, ema: Optional["WeightEMA"]):
        """Average the weights after every update: ``hyper[5]`` carries the step's 1 − decay and one
        more launch (``ema_update``) follows the update kernel, inside a captured step too."""
        if ema is not None and ema.flat is not self.flat:
            raise ValueError("attach_ema: the WeightEMA must be built over this optimizer's FlatParameterSpace")
        if ema is not None and self.bucket_mode:
            raise RuntimeError("attach_ema: attach before the step engine is built (per-bucket updates are already on)")
        self.ema = ema

    # -- the update ---------------------------------------------------------------------
    def hyper_values(self):
        """lr / step / betas of the NEXT update (and the step engine's loss-ring slot; with an
        attached :class:`WeightEMA` its 1 − decay of that step, else 0; word 6 is 1 on a statistics
        step, :meth:`request_stats`), in ``self.hyper``'s layout.  Taking the values consumes a
        statistics request: they are staged exactly once per step."""
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        # every update, eager or replayed, stages these first: the place to refuse one that would
        # train the average instead of the weights
        if self.ema is not None and self.ema.swapped:
            raise RuntimeError("optimizer step while the averaged weights are swapped in (WeightEMA.swap)")
        omd = 0.0 if self.ema is None else self.ema.one_minus_decay(self._step + 1)
        due, self._stats_due = (1.0 if self._stats_due else 0.0), False
        vals = [float(g["lr"]), float(self._step + 1), 0.0, float(b1), float(b2), omd, due, float(self.loss_slot)]
        if len(self.param_groups) > 1:  # the group words: every group's scheduled lr reaches a replayed step
            for g in self.param_groups:
                vals += [float(g["lr"]), float(g["weight_decay"]), float(g["eps"]), 0.0]
        return vals

    def stage_hyper(self):
        """Write lr / step / betas for the NEXT update into device memory (outside any graph)."""
        vals = self.hyper_values()
        if self._ring is not None:
            self._ring.push(vals, self.hyper)
        else:
            self.hyper.copy_(torch.tensor(vals))

    def bucket_updates_ok(self) -> bool:
        """Per-bucket updates are exact only without a global gradient norm (clipping), without
        replicated gradient accumulators (a later fold would add into an updated range) and without
        a weight EMA (the side-stream updates would finish after its launch); a range knows no
        tensor boundaries, so several parameter groups take the whole-buffer update too."""
        return (self.max_grad_norm <= 0 and self.flat.grad_rep is None and self.ema is None
                and len(self.param_groups) == 1 and not self.skip_nonfinite and not self.track_stats)

    def range_update(self, lo: int, hi: int):
        """Fused AdamW over flat elements [lo, hi) only (the same per-element arithmetic as the
        whole-buffer kernel, so a step made of range updates is bitwise the full update); the
        gradient range is cleared as it is consumed.  Reads the hyper-parameters already staged
        for this step."""
        if len(self.param_groups) > 1:
            raise NotImplementedError("range updates take one parameter group (a range knows no tensor boundaries)")
        if self.skip_nonfinite:
            raise NotImplementedError("range updates know no global gradient norm: none with skip_nonfinite")
        g = self.param_groups[0]
        f = self.flat
        _kernels(f.device).adamw(f.data[lo:hi], f.grad[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi],
                                 None if f.shadow is None else f.shadow[lo:hi], self.hyper, g["eps"], g["weight_decay"],
                                 0.0, self.grad_scale, l2=self.l2, zero_grad=True)

    def device_update(self, zero_grad: bool = False):
        """The capturable part: fold, (grad-norm, step guard, per-tensor statistics), the fused update
        over the flat buffers (:meth:`_launch_update`), the EMA launch (not gated by the guard).
        ``zero_grad``: the kernel clears the gradient as it consumes it (flat buffers without
        replicas only; the step engine's captured step then skips its leading zero fill).
        In bucket mode the reducer has already updated every bucket: nothing to do."""
        if self.bucket_mode:
            return
        f = self.flat
        K = _kernels(f.device)
        f.fold()
        if self.norm_part is not None:
            K.sumsq(f.grad, self.norm_part)
        more = {}
        if self.guard is not None:  # a trailing keyword of the update only when on
            K.step_guard(self.norm_part, self.hyper, self.guard, self.grad_scale)
            more["guard"] = self.guard
        if self.track_stats:  # while g and w are still this step's; returns at once unless due / skipped
            K.tensor_stats(f.grad, f.data, self.hyper, self.chunk_tab, self.stats_tensor_tab, self.stats_part,
                           self.stats, self.grad_scale, guard=self.guard, skip_stats=self.skip_stats)
        lo = self.loss_out
        self._launch_update(K, zero_grad=zero_grad and f.grad_rep is None, loss_src=None if lo is None else lo[0],
                            loss_ring=None if lo is None else lo[1], norm_part=self.norm_part, **more)
        if self.ema is not None:
            K.ema_update(self.ema.avg, f.data, self.hyper)

    def _launch_update(self, K, **common):
        """The update itself: the single-group kernel, or ``adamw_grouped`` with several groups."""
        f = self.flat
        if len(self.param_groups) > 1:
            K.adamw_grouped(f.data, f.grad, self.exp_avg, self.exp_avg_sq, f.shadow, self.hyper, self.chunk_tab,
                            self.tensor_group, len(self.param_groups), self.max_grad_norm, self.grad_scale, l2=self.l2,
                            **common)
        else:
            g = self.param_groups[0]
            K.adamw(f.data, f.grad, self.exp_avg, self.exp_avg_sq, f.shadow, self.hyper, g["eps"], g["weight_decay"],
                    self.max_grad_norm, self.grad_scale, l2=self.l2, **common)

    @torch.no_grad()
    def step(self, closure=None, staged: bool = False):
        loss = closure() if closure is not None else None
        if not staged:
            self.stage_hyper()
        self.device_update()
        self._step += 1
        return loss

    def zero_grad(self, set_to_none: bool = False):
        self.flat.zero_grad()

    # -- torch-compatible state dict ------------------------------------------------------
    def _state_index(self):
        """state key → index into ``flat.params``.  One group: the flat order itself (the layout of
        every checkpoint so far).  Several groups: torch's convention, parameters numbered in group
        order as in ``param_groups[j]["params"]``, so the state loads into a ``torch.optim.AdamW`` built
        with the same groups."""
        if len(self.param_groups) == 1:
            return {i: i for i in range(len(self.flat.params))}
        pos = {id(p): i for i, p in enumerate(self.flat.params)}
        ordered = [p for g in self.param_groups for p in g["params"]]
        return {k: pos[id(p)] for k, p in enumerate(ordered) if id(p) in pos}

    def state_dict(self):
        sd = super().state_dict()
        state = {}
        ea, es = self.flat.views(self.exp_avg), self.flat.views(self.exp_avg_sq)
        # with a step guard: the effective step, the one the bias corrections have seen
        step = self._step - (int(self.guard[1]) if self.guard is not None else 0)
        for k, i in self._state_index().items():
            state[k] = {"step": torch.tensor(float(step)), "exp_avg": ea[i].clone(), "exp_avg_sq": es[i].clone()}
        sd["state"] = state
        return sd

    def load_state_dict(self, state_dict):
        state = state_dict.get("state", {})
        groups = state_dict["param_groups"]
        for g, sg in zip(self.param_groups, groups):
            for k, v in sg.items():
                if k != "params":
                    g[k] = v
        ea, es = self.flat.views(self.exp_avg), self.flat.views(self.exp_avg_sq)
        step = 0
        index = self._state_index()
        for i, st in state.items():
            i = index[int(i)]
            if "exp_avg" in st:
                ea[i].copy_(st["exp_avg"])
                es[i].copy_(st["exp_avg_sq"])
            step = int(float(st.get("step", 0)))
        self._step = step
        if self.guard is not None:  # the loaded step is an effective one: the counters start over
            self.guard.zero_()


class FusedAdam(FusedAdamW):
    """``torch.optim.Adam`` semantics (coupled L2: ``weight_decay · p`` joins the gradient after
    clipping) in the same single fused kernel — the optimizer of the LArTPC experiment
    (reference ``run.py:134``: ``Adam(lr=1e-3, weight_decay=1e-4)`` + ``clip_grad_norm_(10)``).
    Parameters whose gradient is identically zero still decay, exactly as torch.optim.Adam does
    for parameters that took part in the backward; leave parameters that never receive a
    gradient (torch skips ``grad is None``) out of ``params``."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, max_grad_norm: float = 0.0, flat: Optional[FlatParameterSpace] = None,
                 skip_nonfinite: bool = False, tensor_stats: bool = False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                         max_grad_norm=max_grad_norm, flat=flat, skip_nonfinite=skip_nonfinite, tensor_stats=tensor_stats)
        self.l2 = True


LAMB_CHUNK = 4096  # elements per chunk of the chunk tables; matches kOptChunk in csrc/optim_common.h


def _cut_chunks(offsets, numels):
    """Every tensor range cut into chunks of at most ``LAMB_CHUNK`` elements → ``chunks`` [(start,
    length, tensor)] and ``tensors`` [(first chunk, chunks)]."""
    chunks, tensors = [], []
    for t, (o, n) in enumerate(zip(offsets, numels)):
        tensors.append((len(chunks), (n + LAMB_CHUNK - 1) // LAMB_CHUNK))
        for s in range(0, n, LAMB_CHUNK):
            chunks.append((o + s, min(LAMB_CHUNK, n - s), t))
    return chunks, tensors


def group_tables(flat: FlatParameterSpace, param_groups):
    """The device tables of an update with several parameter groups over ``flat``: ``chunk_tab``
    (C, 3) int64 = (start, length, tensor), cut as for :func:`lamb_tables`, and ``tensor_group`` (T,)
    int32 = the group of every tensor of ``flat.params`` (groups need not be contiguous in the
    buffer)."""
    group_of = {id(p): j for j, g in enumerate(param_groups) for p in g["params"]}
    missing = [i for i, p in enumerate(flat.params) if id(p) not in group_of]
    if missing:
        raise ValueError(f"{len(missing)} parameter(s) of the flat space belong to no parameter group")
    chunks, _ = _cut_chunks(flat.offsets, [p.numel() for p in flat.params])
    return (torch.tensor(chunks, dtype=torch.int64, device=flat.device).reshape(-1, 3),
            torch.tensor([group_of[id(p)] for p in flat.params], dtype=torch.int32, device=flat.device))


def lamb_tables(offsets, numels, weight_decays, adapts, device):
    """The device tables of the fused LAMB update (csrc/lamb.hip) for tensors at ``offsets`` of
    a flat buffer: every tensor range cut into chunks of at most ``LAMB_CHUNK`` elements (never
    across a tensor boundary; the padding between tensors belongs to no chunk).  Returns
    ``chunk_tab`` (C, 3) int64 = (start, length, tensor), ``tensor_tab`` (T, 2) int32 = (first
    chunk, chunks) and ``tensor_opt`` (T, 2) fp32 = (weight decay, adapt)."""
    chunks, tensors = _cut_chunks(offsets, numels)
    opts = [(float(wd), 1.0 if a else 0.0) for wd, a in zip(weight_decays, adapts)]
    return (torch.tensor(chunks, dtype=torch.int64, device=device).reshape(-1, 3),
            torch.tensor(tensors, dtype=torch.int32, device=device).reshape(-1, 2),
            torch.tensor(opts, dtype=torch.float32, device=device).reshape(-1, 2))


def param_groups(module: torch.nn.Module, weight_decay: float, no_decay_1d: bool = False, lr_scales=None):
    """The two standard parameter-group recipes over ``module.named_parameters()`` (trainable ones):
    ``no_decay_1d`` puts tensors with ``ndim ≤ 1`` (biases, LayerNorm gains) into groups with
    ``weight_decay = 0``; ``lr_scales`` maps a name prefix to a learning-rate multiplier
    (``{"encoder.": 0.1}``; the first matching prefix counts, no match is 1.0).  Returns the non-empty
    groups (1–4 with one prefix) as ``{"params", "weight_decay", "lr_scale"}`` dicts in order of first
    appearance; the caller sets ``lr = base · lr_scale`` (:func:`scale_group_lrs`)."""
    lr_scales = dict(lr_scales or {})
    groups = {}
    for name, p in module.named_parameters():
        if not p.requires_grad:
            continue
        scale = next((float(s) for pre, s in lr_scales.items() if name.startswith(pre)), 1.0)
        wd = 0.0 if no_decay_1d and p.dim() <= 1 else float(weight_decay)
        groups.setdefault((scale, wd), {"params": [], "weight_decay": wd, "lr_scale": scale})["params"].append(p)
    return list(groups.values())


def scale_group_lrs(groups, lr: float):
    """``lr = base · lr_scale`` in every group of :func:`param_groups` (in place) → ``groups``."""
    for g in groups:
        g["lr"] = float(lr) * float(g.get("lr_scale", 1.0))
    return groups


def scale_scheduler_init(init: dict, groups) -> dict:
    """A scheduler's ``{class_path, init_args}`` for an optimizer whose ``groups`` carry ``lr_scale``:
    a scalar ``max_lr`` (``OneCycleLR``) becomes the per-group list ``max_lr · lr_scale``.  Anything
    else — no ``max_lr``, a list already, no scaled group — is returned unchanged."""
    args = dict(init.get("init_args", {}) or {})
    scales = [float(g.get("lr_scale", 1.0)) for g in groups]
    if not isinstance(args.get("max_lr"), (int, float)) or all(s == 1.0 for s in scales):
        return init
    args["max_lr"] = [float(args["max_lr"]) * s for s in scales]
    return {**init, "init_args": args}


class Lamb(torch.optim.Optimizer):
    """LAMB (You et al. 2020, the optimizer of the Perceiver papers), parameter by parameter in
    plain PyTorch — the ``--trainer.precision=32`` path and the reference of :class:`FusedLamb`:

        m ← β1·m + (1−β1)·ĝ,  v ← β2·v + (1−β2)·ĝ²          (ĝ: the gradient after global-norm clipping)
        u = (m / (1−β1^t)) / (sqrt(v) / sqrt(1−β2^t) + eps) + wd·w
        w ← w − lr · trust · u,   trust = ‖w‖ / ‖u‖ when both norms are non-zero, else 1

    With ``exclude_1d`` (a group option, default on) tensors with ``ndim ≤ 1`` (biases, LayerNorm
    gains) are neither decayed nor adapted: ``wd = 0``, ``trust = 1``.  ``max_grad_norm > 0`` clips
    the gradient of all groups together by ``max_grad_norm / (‖g‖ + 1e-6)``, as the fused
    optimizers do."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6, weight_decay: float = 0.01,
                 exclude_1d: bool = True, max_grad_norm: float = 0.0):
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, exclude_1d=bool(exclude_1d))
        super().__init__(params, defaults)
        self.max_grad_norm = float(max_grad_norm)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        clip = 1.0
        if self.max_grad_norm > 0:
            sq = [p.grad.float().pow(2).sum() for g in self.param_groups for p in g["params"] if p.grad is not None]
            if sq:
                f = self.max_grad_norm / (math.sqrt(float(torch.stack(sq).sum())) + 1e-6)
                clip = min(f, 1.0)
        for g in self.param_groups:
            b1, b2 = g["betas"]
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] += 1
                grad = p.grad * clip
                m, v = st["exp_avg"], st["exp_avg_sq"]
                m.mul_(b1).add_(grad, alpha=1 - b1)
                v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
                bc1, bc2 = 1 - b1 ** st["step"], 1 - b2 ** st["step"]
                plain = g["exclude_1d"] and p.dim() <= 1
                u = (m / bc1) / (v.sqrt() / math.sqrt(bc2) + g["eps"])
                if not plain and g["weight_decay"]:
                    u = u + g["weight_decay"] * p
                trust = 1.0
                if not plain:
                    nw, nu = float(torch.linalg.vector_norm(p)), float(torch.linalg.vector_norm(u))
                    if nw > 0 and nu > 0:
                        trust = nw / nu
                p.sub_(u, alpha=g["lr"] * trust)
        return loss


class FusedLamb(FusedAdamW):
    """:class:`Lamb` over a :class:`FlatParameterSpace` (up to 8 parameter groups with their own
    ``lr``, ``weight_decay`` and ``exclude_1d``; ``betas`` and ``eps`` must be equal in every group): two streaming HIP
    kernels and a per-tensor reduction over chunk tables of the flat buffer (csrc/lamb.hip), or
    their emulation on the CPU.  A ``FusedAdamW`` to the step engine (captured update, loss ring,
    gradient cleared as it is consumed, ``grad_scale``), with an AdamW-layout ``state_dict``.  The
    trust ratios need whole tensors, so there are no per-bucket or range updates."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6, weight_decay: float = 0.01,
                 exclude_1d: bool = True, max_grad_norm: float = 0.0, flat: Optional[FlatParameterSpace] = None,
                 skip_nonfinite: bool = False, tensor_stats: bool = False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                         flat=flat, skip_nonfinite=skip_nonfinite, tensor_stats=tensor_stats)
        for g in self.param_groups:  # a group option, as in Lamb
            g.setdefault("exclude_1d", bool(exclude_1d))
            # the LAMB kernels take one eps: refuse what plain Lamb would honour per group
            if float(g["eps"]) != float(self.param_groups[0]["eps"]):
                raise ValueError("FusedLamb: eps must be equal in every parameter group "
                                 "(lr, weight_decay and exclude_1d are per group)")
        f = self.flat
        wds, adapts = self._tensor_options()
        self.chunk_tab, self.tensor_tab, self.tensor_opt = lamb_tables(
            f.offsets, [p.numel() for p in f.params], wds, adapts, f.device)
        # per-chunk (Σw², Σu²) of pass 1, and the per-tensor trust ratios of the last update
        self.partials = torch.zeros(2 * self.chunk_tab.shape[0], dtype=torch.float32, device=f.device)
        self.trust = torch.ones(len(f.params), dtype=torch.float32, device=f.device)

    def _tensor_options(self):
        """Per tensor of ``flat.params``, from its group: (weight decay, adapt)."""
        group_of = {id(p): g for g in self.param_groups for p in g["params"]}
        groups = [group_of[id(p)] for p in self.flat.params]
        plain = [g["exclude_1d"] and p.dim() <= 1 for g, p in zip(groups, self.flat.params)]
        return [0.0 if pl else g["weight_decay"] for g, pl in zip(groups, plain)], [not pl for pl in plain]

    def last_trust(self) -> torch.Tensor:
        """(T,) fp32: the trust ratio every tensor of ``flat.params`` took in the last update."""
        return self.trust

    def bucket_updates_ok(self) -> bool:
        return False

    def range_update(self, lo: int, hi: int):
        raise NotImplementedError("FusedLamb updates whole tensors (per-tensor trust ratios): no range updates")

    def _launch_update(self, K, **common):
        """The LAMB launches over the flat buffers."""
        f = self.flat
        K.lamb(f.data, f.grad, self.exp_avg, self.exp_avg_sq, f.shadow, self.hyper, self.chunk_tab, self.tensor_tab,
               self.tensor_opt, self.partials, self.trust, self.param_groups[0]["eps"], self.max_grad_norm,
               self.grad_scale, tensor_group=self.tensor_group, **common)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # weight_decay / exclude_1d may have come with the groups: refresh the table in place
        # (captured graphs read this very tensor)
        wds, adapts = self._tensor_options()
        self.tensor_opt.copy_(torch.tensor([(wd, 1.0 if a else 0.0) for wd, a in zip(wds, adapts)],
                                           dtype=torch.float32).reshape(-1, 2))


class WeightEMA:
    """Exponential moving average of the trainable weights, for evaluation and export.

    Over a :class:`FlatParameterSpace` the average is ONE more flat fp32 buffer ``avg`` (a copy of
    ``flat.data``; padding stays zero), updated by one streaming launch (csrc/ema.hip) that a fused
    optimizer issues right behind its update (``FusedAdamW.attach_ema``) — inside a captured step
    too, where the step's ``1 − decay`` arrives through ``hyper[5]``.  Over a plain parameter list
    (the eager ``--trainer.precision=32`` path) it keeps per-tensor copies and updates them with
    torch ops (:meth:`update`).

    The schedule is a pure function of the 1-based optimizer step ``t``, so resuming and the
    graph path need no counter of their own: steps with ``t % update_every != 0`` do not update;
    the others use ``u = t // update_every`` and ``d = min(decay, (1 + u) / (10 + u))`` with
    ``warmup``, else ``d = decay``.  Each update is ``e ← e + (1 − d)·(w − e)``: difference,
    product and sum rounded to fp32 one by one, on every path; ``d = 0`` copies the weights
    (``e + (w − e)`` misses ``w`` by a rounding where the two are a factor of two apart).

    :meth:`swap` exchanges the weights with their average in place (and rewrites the bf16 shadow
    the fused kernels read), :meth:`averaged` does so around a block and swaps back in ``finally``
    — bitwise, so captured graphs keep their pointers and training goes on unchanged."""

    def __init__(self, flat_or_params, decay: float = 0.9999, warmup: bool = True, update_every: int = 1):
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:  # also refuses NaN
            raise ValueError(f"WeightEMA: decay must be in [0, 1], got {decay}")
        if int(update_every) < 1:
            raise ValueError(f"WeightEMA: update_every must be at least 1, got {update_every}")
        self.decay, self.warmup, self.update_every = decay, bool(warmup), int(update_every)
        self.swapped = False
        if isinstance(flat_or_params, FlatParameterSpace):
            self.flat: Optional[FlatParameterSpace] = flat_or_params
            self.params = self.flat.params
            self.avg = self.flat.data.clone()
            self._avgs = self.flat.views(self.avg)
            self._hyper = None  # update() outside an optimizer: its own hyper block
        else:
            self.flat = None
            self.params = [p for p in flat_or_params if p.requires_grad]
            if not self.params:
                raise ValueError("no trainable parameters")
            self.avg = None
            self._avgs = [p.detach().clone() for p in self.params]

    # -- schedule -----------------------------------------------------------------------------
    def one_minus_decay(self, t: int) -> float:
        """1 − decay of optimizer step ``t`` (1-based) as the fp32 value the update multiplies by
        (formed in double, rounded once); 0.0 on the steps that do not update."""
        t = int(t)
        if t < 1 or t % self.update_every:
            return 0.0
        d = self.decay
        if self.warmup:
            u = t // self.update_every
            d = min(d, (1.0 + u) / (10.0 + u))
        return float(torch.tensor(1.0 - d, dtype=torch.float64).to(torch.float32))

    # -- update (the fused optimizers launch theirs themselves) -------------------------------------
    @torch.no_grad()
    def update(self, t: int):
        """Fold the current weights into the average as optimizer step ``t`` (1-based)."""
        if self.swapped:
            raise RuntimeError("WeightEMA.update while the averaged weights are swapped in")
        omd = self.one_minus_decay(t)
        if omd == 0.0:
            return
        if self.flat is not None:
            if self._hyper is None:
                self._hyper = torch.zeros(8, dtype=torch.float32, device=self.flat.device)
            self._hyper[5] = omd
            _kernels(self.flat.device).ema_update(self.avg, self.flat.data, self._hyper)
            return
        for p, a in zip(self.params, self._avgs):
            if omd == 1.0:
                a.copy_(p.detach())
                continue
            d = p.detach() - a
            d.mul_(omd)
            a.add_(d)

    # -- evaluation with the averaged weights ----------------------------------------------------
    @torch.no_grad()
    def swap(self):
        """Exchange the weights and their average in place (a second call restores both bitwise).
        Everything keyed on a parameter's version sees a change: versions are bumped, and the
        weight-cache entries bound to the flat shadow — rewritten by the same launch — follow."""
        if self.flat is not None:
            f = self.flat
            _kernels(f.device).ema_swap(f.data, self.avg, f.shadow)
            from .fused import weight_cache

            shadows = f.views(f.shadow) if f.shadow is not None else [None] * len(f.params)
            for p, s in zip(f.params, shadows):
                torch.autograd.graph.increment_version(p)
                if s is not None:
                    weight_cache.rewritten(p, s)
        else:
            for p, a in zip(self.params, self._avgs):
                t = p.detach().clone()
                p.copy_(a)  # in place on the parameter itself: bumps its version
                a.copy_(t)
        self.swapped = not self.swapped

    @contextlib.contextmanager
    def averaged(self):
        """Run the block with the averaged weights; the training weights come back in ``finally``."""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    # -- state ------------------------------------------------------------------------------------
    def tensors(self) -> List[torch.Tensor]:
        """The averaged tensors in ``params`` order (views of ``avg`` over a flat space).  While
        swapped in, the average lives in the parameters and these hold the training weights."""
        return list(self._avgs)

    def state_dict(self) -> List[torch.Tensor]:
        if self.swapped:
            raise RuntimeError("WeightEMA.state_dict while the averaged weights are swapped in")
        return [a.detach().clone() for a in self._avgs]

    @torch.no_grad()
    def load_state_dict(self, tensors):
        if self.swapped:
            raise RuntimeError("WeightEMA.load_state_dict while the averaged weights are swapped in")
        tensors = list(tensors)
        if len(tensors) != len(self._avgs):
            raise ValueError(f"WeightEMA: {len(tensors)} tensors for {len(self._avgs)} parameters")
        for a, t in zip(self._avgs, tensors):
            a.copy_(t.reshape(a.shape))
