"""The flat-space optimizer kernels (csrc/optim.hip, lamb.hip, ema.hip), bit for bit against digests
recorded from a trusted commit (tests/golden/optim_digests.json): SHA-256 of the raw bytes of every
output of ``sumsq``, ``adamw`` (float4 and scalar path), ``adamw_grouped``, ``lamb``, ``fold_replicas``,
``ema_update`` and ``ema_swap`` on the flat case of tests/optim_cases.py, after one launch and after
three consecutive ones (steps 3, 4, 5).  No tolerance: a refactor of these kernels must reproduce
every digest.  Inputs come from a seeded CPU generator and only the public extension API is used.

Recording (never through pytest, and never from the tree under test): in a build of the trusted
commit, ``python tests/test_optim_bits_gpu.py --write tests/golden/optim_digests.json --commit HASH``.
The ``adamw_scalar`` entries of the first recording are an exception, explained in the file's
``scalar_path`` field: that commit's scalar kernel differed from its own float4 kernel in the last bit,
so they come from the first tree in which the two paths agree (which the second test here asserts).
"""
import hashlib
import itertools
import json
import os

import pytest
import torch

from optim_cases import NUMELS, flat_case

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_digests.json")
GROUP_OPTS = [(2e-3, 0.01, 1e-8), (5e-4, 0.0, 1e-8), (1e-3, 0.1, 1e-6), (3e-3, 0.05, 1e-7)]
GSCALE = 0.5
CLIP = 5.0  # active: ‖g‖ · GSCALE ≈ 72
LAUNCHES = (1, 3)
FLAGS = list(itertools.product((0.0, CLIP), (False, True), (False, True)))  # clip, l2, zero_grad


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _hyper(step, opts, groups):
    words = [opts[0][0], float(step), 0.0, 0.9, 0.999, 0.25, 0.0, 2.0]
    if groups:
        for lr, wd, eps in opts:
            words += [lr, wd, eps, 0.0]
    return torch.tensor(words, dtype=torch.float32, device=DEV)


class _Bufs:
    """Fresh copies of the case's buffers (m and v with NaN or zero padding), a shadow, a loss ring and
    the gradient's sumsq partials (taken once, from the untouched gradient)."""

    def __init__(self, K, case, nan_pad):
        self.p, self.g = case["p"].clone(), case["g"].clone()
        self.m, self.v = case["m"].clone(), case["v"].clone()
        if not nan_pad:
            self.m, self.v = torch.nan_to_num(self.m), torch.nan_to_num(self.v)
        self.shadow = torch.zeros(self.p.numel(), dtype=torch.bfloat16, device=DEV)
        self.loss, self.ring = torch.tensor(1.25, device=DEV), torch.zeros(4, device=DEV)
        self.part = torch.full((512,), float("nan"), device=DEV)
        K.sumsq(self.g, self.part)

    def flat(self, lo=0, hi=None):
        return [t[lo:hi] for t in (self.p, self.g, self.m, self.v, self.shadow)]

    def outputs(self, **more):
        return dict(p=self.p, g=self.g, m=self.m, v=self.v, shadow=self.shadow, ring=self.ring, **more)


def _adamw(K, b, step, clip, l2, zero_grad, lo=0, hi=None, ring=True):
    lr, wd, eps = GROUP_OPTS[0]
    K.adamw(*b.flat(lo, hi), _hyper(step, GROUP_OPTS[:1], False), eps, wd, clip, GSCALE, l2=l2, zero_grad=zero_grad,
            loss_src=b.loss if ring else None, loss_ring=b.ring if ring else None,
            norm_part=b.part if clip > 0 else None)


def _steps(record, name, launch, outputs):
    """``launch(step)`` for steps 3, 4, 5; the outputs' digests after the first and the third."""
    for i in range(max(LAUNCHES)):
        launch(3 + i)
        if i + 1 in LAUNCHES:
            torch.cuda.synchronize()
            record[f"{name}/launches={i + 1}"] = {k: _sha(t) for k, t in outputs().items()}


def compute_digests():
    K, case = _ext(), flat_case(DEV)
    rec = {}
    part = torch.full((512,), float("nan"), device=DEV)
    K.sumsq(case["g"], part)
    torch.cuda.synchronize()
    rec["sumsq"] = {"part": _sha(part)}
    for clip, l2, zg in FLAGS:
        tag = f"clip={clip},l2={int(l2)},zero_grad={int(zg)}"
        b = _Bufs(K, case, nan_pad=False)
        _steps(rec, f"adamw_vec/{tag}", lambda s: _adamw(K, b, s, clip, l2, zg), b.outputs)
        b = _Bufs(K, case, nan_pad=False)  # [1:]: 4 bytes off the 16-byte alignment → the scalar kernel
        _steps(rec, f"adamw_scalar/{tag}", lambda s: _adamw(K, b, s, clip, l2, zg, lo=1), b.outputs)
        for G in (2, 4):
            b = _Bufs(K, case, nan_pad=True)
            tg = torch.tensor([t % G for t in range(len(NUMELS))], dtype=torch.int32, device=DEV)
            _steps(rec, f"adamw_grouped/G={G},{tag}",
                   lambda s: K.adamw_grouped(*b.flat(), _hyper(s, GROUP_OPTS[:G], True), case["chunk_tab"], tg, G, clip,
                                             GSCALE, l2=l2, zero_grad=zg, loss_src=b.loss, loss_ring=b.ring,
                                             norm_part=b.part if clip > 0 else None), b.outputs)
    for groups, clip in itertools.product((False, True), (0.0, CLIP)):
        b = _Bufs(K, case, nan_pad=False)
        partials = torch.full((2 * case["chunk_tab"].shape[0],), float("nan"), device=DEV)
        trust = torch.full((len(NUMELS),), float("nan"), device=DEV)
        tg = torch.tensor([t % 2 for t in range(len(NUMELS))], dtype=torch.int32, device=DEV) if groups else None
        _steps(rec, f"lamb/groups={int(groups)},clip={clip}",
               lambda s: K.lamb(*b.flat(), _hyper(s, GROUP_OPTS[:2], groups), case["chunk_tab"], case["tensor_tab"],
                                case["tensor_opt"], partials, trust, 1e-6, clip, GSCALE, zero_grad=True, loss_src=b.loss,
                                loss_ring=b.ring, norm_part=b.part if clip > 0 else None, tensor_group=tg),
               lambda: b.outputs(trust=trust))
    n = case["offsets"][8]  # a 64-aligned prefix of the buffer, as FlatParameterSpace.n_rep is
    grad = case["g"].clone()
    rep = torch.randn(8, n, generator=torch.Generator().manual_seed(5)).to(DEV)
    K.fold_replicas(grad, rep)
    torch.cuda.synchronize()
    rec["fold_replicas"] = {"grad": _sha(grad), "rep": _sha(rep)}
    b = _Bufs(K, case, nan_pad=False)
    avg = b.m.clone()
    _steps(rec, "ema_update", lambda s: K.ema_update(avg, b.p, _hyper(s, GROUP_OPTS[:1], False)), lambda: dict(ema=avg, w=b.p))
    _steps(rec, "ema_swap", lambda s: K.ema_swap(b.p, avg, b.shadow), lambda: dict(w=b.p, ema=avg, shadow=b.shadow))
    return rec


@pytest.mark.timeout(120)
def test_every_digest_is_the_recorded_one():
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = compute_digests()
    want = golden["digests"]
    assert sorted(got) == sorted(want), "the set of cases differs from the recorded one"
    bad = [f"{case}: {k}" for case in want for k in want[case] if got[case].get(k) != want[case][k]]
    assert not bad, (
        f"{len(bad)} output(s) differ bit for bit from commit {golden['commit']} ({golden['hipcc']}): {bad[:12]}.  "
        "If the toolchain changed, re-record the digests from a trusted commit built with the new toolchain "
        "(see this file's docstring), never from the tree under test.")


@pytest.mark.timeout(120)
@pytest.mark.parametrize("clip,l2,zero_grad", FLAGS)
def test_scalar_path_is_bitwise_the_vector_path(clip, l2, zero_grad):
    K, case = _ext(), flat_case(DEV)
    vec, sca = _Bufs(K, case, nan_pad=False), _Bufs(K, case, nan_pad=False)
    for step in (3, 4, 5):
        _adamw(K, vec, step, clip, l2, zero_grad)
        _adamw(K, sca, step, clip, l2, zero_grad, lo=1)
        torch.cuda.synchronize()
        for name, a, b in zip("pgmv", vec.flat(1), sca.flat(1)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, step)
        assert torch.equal(vec.shadow[1:].view(torch.int16), sca.shadow[1:].view(torch.int16)), step
    assert torch.equal(sca.p[:1], case["p"][:1]) and not sca.shadow[:1].view(torch.int16).any()  # outside the slice


@pytest.mark.timeout(120)
@pytest.mark.parametrize("l2", [False, True])
def test_range_updates_are_bitwise_the_whole_buffer_update(l2):
    """``FusedAdamW.range_update``'s claim: a step made of slice launches (no clipping, the gradient
    cleared as it is consumed) is the whole-buffer launch bit for bit."""
    K, case = _ext(), flat_case(DEV)
    whole, parts = _Bufs(K, case, nan_pad=False), _Bufs(K, case, nan_pad=False)
    o = case["offsets"]
    bounds = [0, o[3], o[7], o[9], whole.p.numel()]
    for step in (3, 4, 5):
        _adamw(K, whole, step, 0.0, l2, True, ring=False)
        for lo, hi in reversed(list(zip(bounds[:-1], bounds[1:]))):  # late parameters first, as the reducer does
            _adamw(K, parts, step, 0.0, l2, True, lo=lo, hi=hi, ring=False)
        torch.cuda.synchronize()
        for name, a, b in zip("pgmv", whole.flat(), parts.flat()):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, step)
        assert torch.equal(whole.shadow.view(torch.int16), parts.shadow.view(torch.int16)), step


if __name__ == "__main__":  # write mode: see the docstring
    import argparse
    import subprocess

    ap = argparse.ArgumentParser()
    ap.add_argument("--write", required=True, help="the JSON file to write")
    ap.add_argument("--commit", required=True, help="hash of the commit this tree is a build of")
    a = ap.parse_args()
    hipcc = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True,
                           check=True).stdout.splitlines()
    digests = compute_digests()
    with open(a.write, "w") as f:
        json.dump({"commit": a.commit, "hipcc": " | ".join(s.strip() for s in hipcc[:2]), "digests": digests}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    print(f"wrote {len(digests)} cases to {a.write}")
