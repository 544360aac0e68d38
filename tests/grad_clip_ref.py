"""The float64 rule of global gradient-norm clipping, as the device computes it (csrc/optim.hip: mh_clip_finalize), for
tests/test_grad_clip_cpu.py (where it is checked against torch.nn.utils.clip_grad_norm_ in float64) and the GPU tests.

The raw gradient buffer holds the SUM over ranks; the optimiser's gradient is grad_scale * g (grad_scale = 1/world).  torch clips
that averaged gradient: coef = min(1, max_norm / (||grad_scale * g|| + 1e-6)), so the one multiplier of the RAW gradient is
s = grad_scale * coef.  The device rounds s to fp32 once; s_ref is the unrounded double."""
import math

import torch


def sumsq_ref(pieces) -> float:
    """Sum of squares of the fp32 tensors `pieces` (None = a piece whose module had no gradient) in float64."""
    return float(sum(p.detach().double().pow(2).sum() for p in pieces if p is not None))


def norm_ref(sumsq: float, grad_scale: float = 1.0) -> float:
    return grad_scale * math.sqrt(sumsq)


def s_ref(sumsq: float, max_norm, grad_scale: float = 1.0) -> float:
    """max_norm None: clipping off."""
    if max_norm is None:
        return grad_scale
    return grad_scale * min(1.0, max_norm / (norm_ref(sumsq, grad_scale) + 1e-6))


def sumsq_bound(n: int) -> float:
    """Relative error allowed to an fp64 sum of n exact fp32 squares: (n + 16) * 2^-53 -- every product is exact in fp64, every
    add errs by at most 2^-53 relative, all terms are positive (no cancellation), in any order; 16 covers the few extra adds
    of the block and finalise stages."""
    return (n + 16) * 2.0 ** -53


def s_bound(n: int) -> float:
    """Relative error allowed to s: one fp32 rounding (2^-24) plus the fp64 noise of the sum under it."""
    return 2.0 ** -24 + sumsq_bound(n)
