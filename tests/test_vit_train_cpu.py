"""Argument checks of the fused dgrad + LayerNorm backward (ops.gemm_layernorm_bwd / mh_gemm_layernorm_bwd) that run before any
device work, so they hold without a GPU."""
import pytest
import torch

from myriad_amd import _lib, ops

BF16, F32 = torch.bfloat16, torch.float32


def _args(M=4, N=8, K=64):
    return (torch.zeros((M, K), dtype=BF16), torch.zeros((N, K), dtype=BF16), torch.zeros((M, N), dtype=F32),
            torch.ones((N,), dtype=F32))


@pytest.mark.parametrize("bad", ["w_dtype", "w_len", "x_shape", "gamma_alone", "gamma_len", "dres_shape"])
def test_gemm_layernorm_bwd_rejects_bad_arguments(bad):
    a, b, x, w = _args()
    kw = {}
    if bad == "w_dtype":
        w = w.to(BF16)
    elif bad == "w_len":
        w = torch.ones((7,), dtype=F32)
    elif bad == "x_shape":
        x = torch.zeros((4, 12), dtype=F32)
    elif bad == "gamma_alone":
        kw = dict(dgamma=torch.zeros(8))
    elif bad == "gamma_len":
        kw = dict(dgamma=torch.zeros(7), dbeta=torch.zeros(7))
    else:
        kw = dict(dres=torch.zeros((4, 7), dtype=F32))
    with pytest.raises((ValueError, _lib.MyriadHipError)):
        ops.gemm_layernorm_bwd(a, b, x, w, 1e-6, **kw)


def test_mh_gemm_layernorm_bwd_argument_errors_before_any_launch():
    L = ops._L()
    # no dY scratch; a width that is not a multiple of 4; parameter gradients without their scratch
    assert L.mh_gemm_layernorm_bwd(0, 64, 0, 64, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 8, 64, 1e-6, 0) != 0
    assert L.mh_gemm_layernorm_bwd(0, 64, 0, 64, 16, 16, 16, 0, 0, 0, 0, 0, 0, 0, 0, 4, 6, 64, 1e-6, 0) != 0
    assert L.mh_gemm_layernorm_bwd(0, 64, 0, 64, 16, 16, 16, 0, 0, 0, 16, 16, 0, 0, 0, 4, 8, 64, 1e-6, 0) != 0
    assert L.mh_gemm_layernorm_bwd(0, 64, 0, 64, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 8, 64, 1e-6, 0) == 0   # M = 0: nothing
