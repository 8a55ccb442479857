"""The launch variants of the row-pass kernels (csrc/rowgemm.hip) that tests/test_kernels_gpu.py does
not reach: every comparison is the HIP extension against ops/emulation.py on identical inputs, with
that file's ``close()`` / ``rel_fro()`` and the ``rel`` its neighbouring test uses for the same output.

Which test reaches which branch of the ``*_launch`` functions at the end of rowgemm.hip
(operands and the launchers' host arithmetic: tests/rowgemm_cases.py):

split_tiles (grid.y) — ln_linear_fwd, post_attn_ln_linear_fwd, post_attn_bwd, ln_linear_bwd,
ln_linear_post_attn_bwd:
  split 4 (≤ 64 tiles)   every test of parts 2-4 here and test_kernels_gpu.py (R ≤ 512)
  split 2 (65-127 tiles) test_split_* at R = 4197 (66 tiles, the last one 37 rows)
  split 1 (≥ 128 tiles)  test_split_* at R = 8192 (128 whole tiles) and 8197 (129, the last one 5 rows)
  appended slab-job workgroups, (nblk + split − 1) / split of them: the third run of every
  test_split_*_bwd, nblk = 91 (a multiple of neither 2 nor 4)

AV (av_ok: every pointer 16-byte aligned):
  post_attn_fwd_kernel<C, true>            test_kernels_gpu.py test_post_attn, aligned runs of test_misaligned_post_attn_fwd
  post_attn_fwd_kernel<C, false>           test_misaligned_post_attn_fwd, C = 32, 64, 128
  post_attn_ln_linear_fwd_kernel<C, true>  test_split_post_attn_ln_linear_fwd (C = 64, 128), aligned runs below (C = 32)
  post_attn_ln_linear_fwd_kernel<C, false> test_misaligned_post_attn_ln_linear_fwd, C = 32, 64, 128
  post_attn_bwd_kernel<C, true>            test_split_post_attn_bwd, aligned runs of test_misaligned_post_attn_bwd
  post_attn_bwd_kernel<C, false>           test_misaligned_post_attn_bwd, C = 32, 64, 128
  ln_linear_post_attn_bwd_kernel<C, true, NQ>   test_boundary_bwd_row_pass, test_split_boundary_bwd
  ln_linear_post_attn_bwd_kernel<C, false, 3>   test_misaligned_boundary_bwd, C = 32, 64, 128
  ln_linear_fwd_kernel<…, false> at an even Kin: test_misaligned_ln_linear_fwd — "all" (vf = 0), "x"
    (kVecW | kVecLn), "w" (kVecLn), "ln" (kVecW)
  ln_linear_bwd_kernel<…, false> at an even Kin: test_misaligned_ln_linear_bwd — "all" (vf = 0), "g"
    (kVecW | kVecLn), "w" (kVecG | kVecLn), "ln" (kVecG | kVecW)
  wgrad_kernel has no AV flag; its in-kernel scalar staging of G and A: test_misaligned_wgrad

the row-pass boundary kernel ln_linear_post_attn_bwd_kernel<C, AV, NQ> (the launcher hands a call to
chain.hip only for C == 64 && H == 4 && R % 64 == 0 with aligned operands; the launch counters of
tests/test_models.py count Python calls of the op and cannot tell the two kernels apart, so every
case here fails that condition by C, by H or by R % 64 != 0, which the launcher's text makes proof):
  <128, ·, 3> <128, ·, 1>  test_boundary_bwd_row_pass (128, 4, 384 | 128); split: test_split_boundary_bwd
  <32, ·, 3>  <32, ·, 1>   test_boundary_bwd_row_pass (32, 1, 96 | 32)
  <64, ·, 3>               test_boundary_bwd_row_pass (64, 2, 192); test_split_boundary_bwd (H = 2; H = 4 at R % 64 != 0)
  <64, ·, 1>               not reached here (C = 64 query projections run in test_kernels_gpu.py through chain.hip)
  bf16 g widened by the binding: test_boundary_bwd_bf16_g_is_widened

pick_nch:
  ln_linear_fwd   NCH 1: Kin 24 (a 24-column tail), 32;  4: 128;  8: 256  test_chunk_counts_ln_linear_fwd
                  NCH 2, 5: test_kernels_gpu.py (Kin 64, 131)
  ln_linear_bwd, wgrad   NCH 1: Kin 24, 32;  4: 128   test_chunk_counts_ln_linear_bwd_and_wgrad
                  NCH 2, 5: test_kernels_gpu.py

operand types: ln_linear_fwd (x, y) and ln_linear_bwd (G, X), wgrad (G, A) ∈ {fp32, bf16}², all four
pairs in test_chunk_counts_*; the bindings accept every pair.

Per 64-row tile (part 1) every row output is held to the whole-tensor figure.  Largest per-tile
relative Frobenius error measured on an MI355X, per operation (bound min(rel, 1e-2)):
  ln_linear_fwd            y 2.7e-4, mean 1.3e-7, rstd 7.8e-8
  post_attn_ln_linear_fwd  qkv 4.6e-4, mean1 4.0e-4, u 3.3e-4, z 2.0e-4, rstd1 3.3e-5, y / mean2 / rstd2 ≤ 2.6e-7
  post_attn_bwd            delta 5.5e-4, dO 3.8e-4, dy 8.2e-5
  ln_linear_bwd            dx 1.4e-7
  ln_linear_post_attn_bwd  delta 1.2e-3, dO 7.3e-4, dy 4.1e-4
so the bound holds as it stands, with no float64 floor added.
"""
import pytest
import torch

import rowgemm_cases as rc
from test_kernels_gpu import close, rel_fro

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = rc.EPS


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


def _emu():
    from perceiver_io_amd.ops import emulation

    return emulation


def tiles_close(op, a, b, rel, name):
    """every 64-row tile of a row output within the whole-tensor bound of close()"""
    e = rc.tile_rel_fro(a, b)
    worst, at = e.max().item(), int(e.argmax())
    print(f"PERTILE {op} {name} rows={a.shape[0]} worst={worst:.3e} tile={at}/{e.numel()}")
    assert worst <= min(rel, 1e-2), f"{op} {name}: tile {at} of {e.numel()} has relative Frobenius error {worst:.3e}"


def rows_close(op, outs, refs, names, rels, tag=""):
    for a, b, n, rel in zip(outs, refs, names, rels):
        close(a, b, rel, f"{n}{tag}")
        tiles_close(op, a, b, rel, f"{n}{tag}")


def check_job(job_dst, alone, bound):
    """the destinations of a slab job run by a carrier's appended workgroups against the standalone
    slab_reduce of the same slab: the same fp32 terms summed in another order"""
    for i, (a, b, lim) in enumerate(zip(job_dst, alone, bound)):
        err = (a.double() - b.double()).abs().cpu()
        assert bool((err <= lim.cpu()).all()), f"slab job segment {i}: {err.max().item():.3e}"


def _job():
    slab, dst, offs, init = rc.make_job(DEV)
    alone = [t.clone() for t in init]
    _ext().slab_reduce(slab, alone, offs)
    return slab, dst, offs, alone, rc.job_bound(slab, init, offs)


# =================================================================================================
# 1. split count × partial tile × slab job
# =================================================================================================
SPLIT_ROWS = [(4197, 64), (8192, 64), (8197, 64), (4197, 128), (8197, 128)]


def test_split_rows_reach_every_branch():
    assert [rc.split_tiles(r) for r in (512, 4096, 4197, 8128, 8192, 8197)] == [4, 4, 2, 2, 1, 1]
    nblk = rc.job_nblk(rc.JOB_ROWS, rc.slab_layout(rc.JOB_SIZES)[1])
    assert nblk % 2 and nblk % 4  # the appended grid rows do not divide evenly at split 2 (or 4)


@pytest.mark.parametrize("R,C", SPLIT_ROWS)
def test_split_ln_linear_fwd(R, C):
    d = rc.ln_linear_operands(R, C, 3 * C, DEV)
    for act, res, ob in ((0, None, True), (1, d["res"], False)):
        a, b = (K.ln_linear_fwd(d["x"], d["lnw"], d["lnb"], EPS, d["w"], d["bias"], act, res, ob, True)
                for K in (_ext(), _emu()))
        rows_close("ln_linear_fwd", a, b, ("y", "mean", "rstd"), (2e-2, 1e-4, 1e-3), f" act={act}")


@pytest.mark.parametrize("R,C", SPLIT_ROWS)
def test_split_post_attn_ln_linear_fwd(R, C):
    d = rc.post_attn_operands(R, C, DEV)
    args = rc.pa_fwd_args(d) + [d[k] for k in rc.NEXT]
    a, b = (K.post_attn_ln_linear_fwd(*args) for K in (_ext(), _emu()))
    rows_close("post_attn_ln_linear_fwd", a, b, ("z", "y", "mean2", "rstd2", "u", "qkv", "mean1", "rstd1"), (2e-2,) * 8)


def _grads_close(got, ref, names, rels, tag):
    for a, b, n, rel in zip(got, ref, names, rels):
        close(a.reshape(b.shape), b, rel, n + tag)


@pytest.mark.parametrize("R,C", SPLIT_ROWS)
def test_split_post_attn_bwd(R, C):
    """three runs: NaN slab + slab_reduce, plain accumulating targets, and carrying a slab job"""
    H, tiles = 4, (R + 63) // 64
    d = rc.post_attn_operands(R, C, DEV)
    z, y, m, r, u = _emu().post_attn_fwd(*rc.pa_fwd_args(d))
    args = (d["dz"], y, m, r, u, d["o"], d["wo"], d["w1"], d["w2"], d["g2"], d["be2"], H)
    shapes, rows, rels = rc.pa_shapes(C), ("dy", "dO", "delta"), (3e-2,) * 3
    ref_g = [torch.full(s, 0.5, device=DEV) for s in shapes]
    ref = _emu().post_attn_bwd(*args, ref_g)
    # 1: the slab sink
    slab, views, offs = rc.slab_views(tiles, rc.pa_sizes(C), DEV)
    o1 = _ext().post_attn_bwd(*args, views, slab=True)
    assert torch.isfinite(slab).all()  # every tile wrote every element of its row
    dst = [torch.full(s, 0.5, device=DEV) for s in shapes]
    _ext().slab_reduce(slab, dst, offs)
    rows_close("post_attn_bwd", o1, ref, rows, rels, " (slab)")
    _grads_close(dst, ref_g, rc.PA_GRADS, (3e-2,) * 8, " (slab)")
    # 2: plain accumulating targets
    acc = [torch.full(s, 0.5, device=DEV) for s in shapes]
    o2 = _ext().post_attn_bwd(*args, acc)
    rows_close("post_attn_bwd", o2, ref, rows, rels, " (atomic)")
    _grads_close(acc, ref_g, rc.PA_GRADS, (3e-2,) * 8, " (atomic)")
    # 3: the previous kernel's slab job in the appended workgroups
    jslab, jdst, joffs, alone, bound = _job()
    acc = [torch.full(s, 0.5, device=DEV) for s in shapes]
    o3 = _ext().post_attn_bwd(*args, acc, job_slab=jslab, job_dsts=jdst, job_offs=joffs)
    rows_close("post_attn_bwd", o3, ref, rows, rels, " (job)")
    _grads_close(acc, ref_g, rc.PA_GRADS, (3e-2,) * 8, " (job)")
    check_job(jdst, alone, bound)


@pytest.mark.parametrize("R,C", SPLIT_ROWS)
def test_split_ln_linear_bwd(R, C):
    """three runs: NaN slab + slab_reduce, plain accumulating targets, and carrying a slab job"""
    Kin, N, tiles = C, 3 * C, (R + 63) // 64
    d = rc.ln_linear_operands(R, Kin, N, DEV)
    args = (d["g"], d["w"], d["x"], d["mean"], d["rstd"], d["lnw"], d["lnb"], d["dres"], True)
    shapes, sizes, rels = [(Kin,), (Kin,), (N, Kin), (N,)], [Kin, Kin, N * Kin, N], (3e-2, 3e-2, 3e-2, 1e-4)

    def targets():
        return [torch.full(s, 0.5, device=DEV) for s in shapes]

    ref_g = targets()
    ref = _emu().ln_linear_bwd(*args, *ref_g)
    slab, views, offs = rc.slab_views(tiles, sizes, DEV)
    dx1 = _ext().ln_linear_bwd(*args, *views, slab=True)
    assert torch.isfinite(slab).all()
    dst = targets()
    _ext().slab_reduce(slab, dst, offs)
    rows_close("ln_linear_bwd", [dx1], [ref], ["dx"], [3e-2], " (slab)")
    _grads_close(dst, ref_g, rc.LL_GRADS, rels, " (slab)")
    acc = targets()
    dx2 = _ext().ln_linear_bwd(*args, *acc)
    rows_close("ln_linear_bwd", [dx2], [ref], ["dx"], [3e-2], " (atomic)")
    _grads_close(acc, ref_g, rc.LL_GRADS, rels, " (atomic)")
    jslab, jdst, joffs, alone, bound = _job()
    acc = targets()
    dx3 = _ext().ln_linear_bwd(*args, *acc, job_slab=jslab, job_dsts=jdst, job_offs=joffs)
    rows_close("ln_linear_bwd", [dx3], [ref], ["dx"], [3e-2], " (job)")
    _grads_close(acc, ref_g, rc.LL_GRADS, rels, " (job)")
    check_job(jdst, alone, bound)


def _boundary_reference(d, C, nq, H, **kw):
    sizes = rc.boundary_sizes(C, nq)
    slab, tg, _ = rc.slab_views((d["y"].shape[0] + 63) // 64, sizes, DEV, 0.0)
    outs = rc.run_boundary(_emu(), d, H, tg, **kw)
    return list(outs) + rc.slab_sums(slab, sizes)


def _boundary_hip(d, C, nq, H, **kw):
    """one launch into a NaN-filled slab, then slab_reduce onto zeroed destinations: the 15 outputs"""
    sizes = rc.boundary_sizes(C, nq)
    slab, tg, offs = rc.slab_views((d["y"].shape[0] + 63) // 64, sizes, DEV)
    outs = rc.run_boundary(_ext(), d, H, tg, **kw)
    assert torch.isfinite(slab).all()  # every tile stored every element of its slab row
    dst = [torch.zeros(n, device=DEV) for n in sizes]
    _ext().slab_reduce(slab, dst, offs)
    return list(outs) + dst, slab


def _boundary_close(got, ref, tag=""):
    errs = {n: rel_fro(a, b) for n, a, b in zip(rc.BOUNDARY_NAMES, got, ref)}
    assert not {n: e for n, e in errs.items() if not e < 1e-2}, (tag, errs)


@pytest.mark.parametrize("R,C,H", [(4197, 128, 4), (8197, 128, 4), (4197, 64, 2), (8192, 64, 2), (8197, 64, 2),
                                   (4197, 64, 4), (8197, 64, 4)])
def test_split_boundary_bwd(R, C, H):
    """The row-pass boundary kernel at split 2 and 1: C = 128, H = 2 at C = 64, or R % 64 != 0 keep
    the call off the chain kernel (see the module docstring).  The binding takes slab targets only:
    a NaN slab + slab_reduce, then the same carrying a slab job."""
    nq = 3 * C
    assert not (C == 64 and H == 4 and R % 64 == 0)
    d = rc.boundary_operands(R, C, nq, DEV)
    ref = _boundary_reference(d, C, nq, H)
    got, _ = _boundary_hip(d, C, nq, H)
    _boundary_close(got, ref, "slab")
    for a, b, n in zip(got[:3], ref[:3], rc.BOUNDARY_NAMES):
        tiles_close("ln_linear_post_attn_bwd", a, b, 1e-2, n)
    jslab, jdst, joffs, alone, bound = _job()
    got, _ = _boundary_hip(d, C, nq, H, job_slab=jslab, job_dsts=jdst, job_offs=joffs)
    _boundary_close(got, ref, "job")
    for a, b, n in zip(got[:3], ref[:3], rc.BOUNDARY_NAMES):
        tiles_close("ln_linear_post_attn_bwd", a, b, 1e-2, n + " (job)")
    check_job(jdst, alone, bound)


# =================================================================================================
# 2. misaligned operands: the AV = false instantiations.  The aligned and the misaligned run differ
# only in how operands are loaded and rows stored (row_load / tile_fetch / g_fetch / row_store); the
# arithmetic between them is the same source in both instantiations, and every row output has one
# writer and no atomics, so those outputs must agree to the bit.
# =================================================================================================
def _same(a, b, names, tag):
    for x, y, n in zip(a, b, names):
        assert torch.equal(x, y), f"{n}: aligned and misaligned runs differ ({tag})"


@pytest.mark.parametrize("C", [32, 64, 128])
def test_misaligned_post_attn_fwd(C):
    d = rc.post_attn_operands(150, C, DEV)
    names = ("z", "y", "mean", "rstd", "u")
    ref = _emu().post_attn_fwd(*rc.pa_fwd_args(d))
    al = _ext().post_attn_fwd(*rc.pa_fwd_args(d))
    mis = _ext().post_attn_fwd(*rc.pa_fwd_args(rc.off1_all(d)))
    for t1, t2, n in zip(mis, ref, names):
        close(t1, t2, 2e-2, n + " (misaligned)")
    _same(al, mis, names, f"C={C}")


@pytest.mark.parametrize("C", [32, 64, 128])
def test_misaligned_post_attn_ln_linear_fwd(C):
    d = rc.post_attn_operands(200, C, DEV)
    names = ("z", "y", "mean2", "rstd2", "u", "qkv", "mean1", "rstd1")

    def run(K, dd):
        return K.post_attn_ln_linear_fwd(*(rc.pa_fwd_args(dd) + [dd[k] for k in rc.NEXT]))

    ref, al, mis = run(_emu(), d), run(_ext(), d), run(_ext(), rc.off1_all(d))
    for t1, t2, n in zip(mis, ref, names):
        close(t1, t2, 2e-2, n + " (misaligned)")
    _same(al, mis, names, f"C={C}")


@pytest.mark.parametrize("C,H", [(32, 1), (64, 4), (128, 4)])
def test_misaligned_post_attn_bwd(C, H):
    R = 150
    d = rc.post_attn_operands(R, C, DEV)
    z, y, m, r, u = _emu().post_attn_fwd(*rc.pa_fwd_args(d))
    ops = dict(dz=d["dz"], y=y, m=m, r=r, u=u, o=d["o"], wo=d["wo"], w1=d["w1"], w2=d["w2"], g2=d["g2"], be2=d["be2"])

    def run(K, dd):
        grads = [torch.full(s, 0.5, device=DEV) for s in rc.pa_shapes(C)]  # parameter gradients: atomics
        return list(K.post_attn_bwd(*dd.values(), H, grads)) + grads

    ref, al, mis = run(_emu(), ops), run(_ext(), ops), run(_ext(), rc.off1_all(ops))
    for a, b, n in zip(mis, ref, ("dy", "dO", "delta") + rc.PA_GRADS):
        close(a, b, 3e-2, n + " (misaligned)")
    _same(al[:3], mis[:3], ("dy", "dO", "delta"), f"C={C}")


@pytest.mark.parametrize("C,H", [(32, 1), (64, 4), (128, 4)])
def test_misaligned_boundary_bwd(C, H):
    """R = 200 (a partial tile): the aligned run is the row-pass kernel's <C, true, 3> too"""
    R, nq = 200, 3 * C
    d = rc.boundary_operands(R, C, nq, DEV)
    ref = _boundary_reference(d, C, nq, H)
    al, slab_al = _boundary_hip(d, C, nq, H)
    mis, slab_mis = _boundary_hip(rc.off1_all(d), C, nq, H)  # the slab targets stay aligned
    _boundary_close(mis, ref, "misaligned")
    _same(al[:3], mis[:3], rc.BOUNDARY_NAMES, f"C={C}")
    assert torch.equal(slab_al, slab_mis)  # slab rows are plain stores of one workgroup each


def _pick(d, which):
    return rc.off1_all(d, None if which == "all" else {"x": ("x", "dres", "u"), "g": ("g",), "w": ("w",),
                                                       "ln": ("lnw", "lnb")}[which])


@pytest.mark.parametrize("which", ["all", "x", "w", "ln"])
def test_misaligned_ln_linear_fwd(which):
    """Even Kin, AV = false through a misaligned base pointer; one operand class at a time runs each
    vec_flags mix (the forward has no G: its row operand x stands in for it)."""
    R, Kin, N = 200, 64, 192
    d = rc.ln_linear_operands(R, Kin, N, DEV)
    names = ("y", "mean", "rstd")

    def run(K, dd, act, res, ob):
        return K.ln_linear_fwd(dd["x"], dd["lnw"], dd["lnb"], EPS, dd["w"], dd["bias"], act, res, ob, True)

    m = _pick(d, which)
    for act, res, ob in ((0, None, True), (1, "res", False)):
        ref, al, mis = (run(K, dd, act, dd[res] if res else None, ob) for K, dd in ((_emu(), d), (_ext(), d), (_ext(), m)))
        for t1, t2, n, rel in zip(mis, ref, names, (2e-2, 1e-4, 1e-3)):
            close(t1, t2, rel, f"{n} ({which} misaligned)")
        _same(al, mis, names, which)


@pytest.mark.parametrize("which", ["all", "g", "w", "ln"])
def test_misaligned_ln_linear_bwd(which):
    R, Kin, N = 200, 64, 192
    d = rc.ln_linear_operands(R, Kin, N, DEV)

    def run(K, dd):
        tg = [torch.full(s, 0.5, device=DEV) for s in ((Kin,), (Kin,), (N, Kin), (N,))]
        dx = K.ln_linear_bwd(dd["g"], dd["w"], dd["x"], dd["mean"], dd["rstd"], dd["lnw"], dd["lnb"], dd["dres"], True, *tg)
        return [dx] + tg

    ref, al, mis = run(_emu(), d), run(_ext(), d), run(_ext(), _pick(d, which))
    for a, b, n, rel in zip(mis, ref, ("dx",) + rc.LL_GRADS, (3e-2, 3e-2, 3e-2, 3e-2, 1e-4)):
        close(a, b, rel, f"{n} ({which} misaligned)")
    _same(al[:1], mis[:1], ("dx",), which)  # the parameter gradients are atomic adds


def test_misaligned_wgrad():
    """wgrad picks its G / A staging by alignment inside the kernel: scalar loads for both"""
    R, Kin, N = 200, 64, 192
    d = rc.ln_linear_operands(R, Kin, N, DEV)
    m = rc.off1_all(d)
    for mode, a in ((0, "x"), (1, "x"), (2, "u")):
        outs = []
        for K, dd in ((_emu(), d), (_ext(), m)):
            dW, db = torch.ones(N, Kin, device=DEV), torch.ones(N, device=DEV)
            K.wgrad(dd["g"], dd[a], mode, dd["mean"], dd["rstd"], dd["lnw"], dd["lnb"], 64, dW, db)
            outs.append((dW, db))
        close(outs[1][0], outs[0][0], 3e-2, f"dW mode {mode} (misaligned)")
        close(outs[1][1], outs[0][1], 1e-4, f"db mode {mode} (misaligned)")


# =================================================================================================
# 3. the row-pass boundary backward in isolation
# =================================================================================================
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("R", [320, 200])
@pytest.mark.parametrize("C,H,nq", [(128, 4, 384), (128, 4, 128), (32, 1, 96), (32, 1, 32), (64, 2, 192)])
def test_boundary_bwd_row_pass(C, H, nq, R, p):
    """ln_linear_post_attn_bwd_kernel<C, true, NQ> on the operands of test_kernels_gpu.py
    test_ln_linear_post_attn_bwd_isolated at the shapes the chain kernel refuses: all 15 outputs."""
    d = rc.boundary_operands(R, C, nq, DEV)
    kw = dict(seed=torch.tensor([1234567], dtype=torch.int64, device=DEV) if p > 0 else None, site=3, p=p)
    got, _ = _boundary_hip(d, C, nq, H, **kw)
    _boundary_close(got, _boundary_reference(d, C, nq, H, **kw))


def test_boundary_bwd_bf16_g_is_widened():
    """A bf16 g at C = 128: the launcher refuses it (only the chain kernel reads bf16), the binding
    widens it and launches again — bit for bit the result of the same values passed as fp32."""
    C, H, nq, R = 128, 4, 384, 200
    d = rc.boundary_operands(R, C, nq, DEV)
    gb = d["g"].to(torch.bfloat16)
    wide, slab_w = _boundary_hip(dict(d, g=gb.float()), C, nq, H)
    narrow, slab_n = _boundary_hip(dict(d, g=gb), C, nq, H)
    _same(wide[:3], narrow[:3], rc.BOUNDARY_NAMES, "bf16 g")
    assert torch.equal(slab_w, slab_n)
    _boundary_close(narrow, _boundary_reference(dict(d, g=gb.float()), C, nq, H))


# =================================================================================================
# 4. chunk counts and operand types: R = 130 (a partial tile), N = 192 (three column chunks)
# =================================================================================================
PAIRS = [(False, False), (False, True), (True, False), (True, True)]


def _bf(t, on):
    return t.to(torch.bfloat16) if on else t


@pytest.mark.parametrize("xbf,ybf", PAIRS)
@pytest.mark.parametrize("Kin", [24, 32, 128, 256])
def test_chunk_counts_ln_linear_fwd(Kin, xbf, ybf):
    assert rc.pick_nch(Kin) == {24: 1, 32: 1, 128: 4, 256: 8}[Kin]
    d = rc.ln_linear_operands(130, Kin, 192, DEV)
    x = _bf(d["x"], xbf)
    for act, res in ((0, None), (1, d["res"])):
        a, b = (K.ln_linear_fwd(x, d["lnw"], d["lnb"], EPS, d["w"], d["bias"], act, res, ybf, True)
                for K in (_ext(), _emu()))
        assert a[0].dtype == b[0].dtype == (torch.bfloat16 if ybf else torch.float32)
        for t1, t2, n, rel in zip(a, b, ("y", "mean", "rstd"), (2e-2, 1e-4, 1e-3)):
            close(t1, t2, rel, n)


@pytest.mark.parametrize("gbf,xbf", PAIRS)
@pytest.mark.parametrize("Kin", [24, 32, 128])
def test_chunk_counts_ln_linear_bwd_and_wgrad(Kin, gbf, xbf):
    assert rc.pick_nch(Kin) == {24: 1, 32: 1, 128: 4}[Kin]
    R, N = 130, 192
    d = rc.ln_linear_operands(R, Kin, N, DEV)
    g, x = _bf(d["g"], gbf), _bf(d["x"], xbf)
    mean, rstd = x.float().mean(-1), torch.rsqrt(x.float().var(-1, unbiased=False) + EPS)
    res = []
    for K in (_ext(), _emu()):
        tg = [torch.full(s, 0.5, device=DEV) for s in ((Kin,), (Kin,), (N, Kin), (N,))]
        res.append([K.ln_linear_bwd(g, d["w"], x, mean, rstd, d["lnw"], d["lnb"], d["dres"], True, *tg)] + tg)
    for a, b, n, rel in zip(res[0], res[1], ("dx",) + rc.LL_GRADS, (3e-2, 3e-2, 3e-2, 3e-2, 1e-4)):
        close(a, b, rel, n)
    for mode in (0, 1, 2):
        outs = []
        for K in (_ext(), _emu()):
            dW, db = torch.ones(N, Kin, device=DEV), torch.ones(N, device=DEV)
            K.wgrad(g, x, mode, mean, rstd, d["lnw"], d["lnb"], 64, dW, db)
            outs.append((dW, db))
        close(outs[0][0], outs[1][0], 3e-2, f"dW mode {mode}")
        close(outs[0][1], outs[1][1], 1e-4, f"db mode {mode}")
