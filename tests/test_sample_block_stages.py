"""The per-sample block emulation (ops/emulation.py ``sb_fwd`` / ``sb_bwd`` / ``sb_wgrad``) called
directly with its optional stages — pre (a cross layer's post-attention half), post (the next cross
layer's LN + projection, N = C or a decoder's 2C-wide K|V), an empty / absent ``dres``, the
appended slab job — against the float64 composite of tests/sample_block_cases.py.

Bound: the 2 % relative Frobenius error of tests/test_sample_block_gpu.py (bf16 operands, fp32
accumulation), per sample for every tensor with a sample axis.  The cases are those the GPU module
(tests/test_sample_block_stages_gpu.py) runs the kernels on."""
import pytest
import torch

import sample_block_cases as sbc
from perceiver_io_amd.ops import emulation

BOUND = 2e-2


@pytest.fixture(scope="module")
def runs():
    """per case: the operands, one emulated forward / backward / weight-gradient pass and the
    float64 reference, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            c = sbc.case(name, "cpu")
            x0, fwd = sbc.run_fwd(emulation, c)
            bwd = sbc.run_bwd(emulation, c, x0, fwd)
            jobs = sbc.wgrad_jobs(c, fwd, bwd)
            tg = sbc.wgrad_targets(c, jobs)
            sbc.run_wgrad(emulation, c, jobs, bwd["slab"], tg)
            cache[name] = (c, x0, fwd, bwd, tg, sbc.reference(c))
        return cache[name]

    return get


def _check(errs):
    for k, v in errs.items():
        print(f"{k}: {v:.3e}")
    bad = {k: v for k, v in errs.items() if not v < BOUND}
    assert not bad, bad


@pytest.mark.parametrize("name", list(sbc.CASES))
def test_emulated_forward_matches_float64(name, runs):
    """block input after the call (the pre stage's output), block output and Q, per sample"""
    c, x0, fwd, bwd, tg, ref = runs(name)
    if not c["pre"]:
        assert torch.equal(x0, c["x"])  # no pre stage: the input is not written
    _check(sbc.reference_errors(c, x0, fwd, bwd, tg, ref)[0])


@pytest.mark.parametrize("name", list(sbc.CASES))
def test_emulated_backward_matches_float64(name, runs):
    """dx, dO, δ = rowsum(dO∘O) per head (per sample); the reduced LayerNorm slab and every dW / db
    of the grouped weight-gradient jobs"""
    c, x0, fwd, bwd, tg, ref = runs(name)
    _check(sbc.reference_errors(c, x0, fwd, bwd, tg, ref)[1])


def test_emulated_backward_takes_no_dres():
    """post stage, empty dres: an empty tensor and None both mean zero (as the binding's empty one)"""
    c = sbc.case("B5_L3_C64_pre_bcast_post2C_empty_dres", "cpu")
    assert c["dres"].numel() == 0
    x0, fwd = sbc.run_fwd(emulation, c)
    io = sbc.post_io(c, fwd)
    outs = [sbc.run_bwd(emulation, c, x0, fwd, post_io=[io[0], d, io[2], io[3]])
            for d in (c["dres"], None, torch.zeros(c["R"], c["C"]))]
    for other in outs[:2]:
        for (n, a), (_, b) in zip(sbc.named_bwd(c, other), sbc.named_bwd(c, outs[2])):
            assert torch.equal(a, b), n
