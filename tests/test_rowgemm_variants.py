"""The emulation of the layer-boundary backward at C != 64, on the CPU: it is the reference of
tests/test_rowgemm_variants_gpu.py, and whole-model tests are all that otherwise run it there."""
import pytest
import torch

import rowgemm_cases as rc
from perceiver_io_amd.ops import emulation

# twice the largest error measured below
BOUND = 2 * 5.05e-3


@pytest.mark.parametrize("C,H", [(32, 1), (128, 4)])
def test_boundary_emulation_matches_fp64_autograd(C, H):
    """emulation.post_attn_fwd → emulation.ln_linear_post_attn_bwd against float64 autograd of the
    same composite in plain PyTorch (out-projection, residual, LayerNorm, MLP with GELU, residual,
    then LayerNorm and linear), R = 96, p = 0: all 15 outputs by name.

    The emulation rounds every GEMM operand (and dO) to bf16; the reference does not.  Measured
    relative Frobenius errors, C = 32 | C = 128:
      dy 1.89e-3 | 1.79e-3    dO 3.08e-3 | 2.93e-3    delta 3.38e-3 | 2.99e-3
      dlnw 3.18e-3 | 1.99e-3  dlnb 1.57e-3 | 1.78e-3  dWq 2.60e-3 | 2.56e-3   dbq 8.9e-8 | 1.0e-7
      dWo 2.49e-3 | 2.47e-3   dbo 2.48e-3 | 1.94e-3   dg2 2.49e-3 | 3.30e-3   dbe2 5.05e-3 | 3.43e-3
      dW1 3.53e-3 | 3.50e-3   db1 3.58e-3 | 2.67e-3   dW2 3.80e-3 | 3.76e-3   db2 1.55e-3 | 1.46e-3
    The largest is 5.05e-3 (dbe2 at C = 32); every output is held to twice that."""
    R = 96
    d = rc.post_attn_operands(R, C, "cpu")
    gen = torch.Generator().manual_seed(77 + C)
    g, dres = torch.randn(R, 3 * C, generator=gen), torch.randn(R, C, generator=gen)
    ref = rc.boundary_composite_fp64(d, g, dres, H)
    got = rc.boundary_emulation(emulation, d, g, dres, H)
    errs = {n: rc.rel_fro(got[n].reshape(ref[n].shape), ref[n]) for n in rc.BOUNDARY_NAMES}
    print(errs)
    assert not {n: e for n, e in errs.items() if not e <= BOUND}, errs
