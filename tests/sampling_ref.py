"""Test-side restatement of the decode sampler (mh_sample_rows / mh_repetition_penalty_rows, include/myriad_hip.h): HF's per-row
chain RepetitionPenalty -> MinLength ban -> Temperature -> TopK (ties at the k-th value kept) -> TopP -> draw, with the kernel's
Philox4x32-10 uniform.  Logits in float32 (the kernel's arithmetic up to the temperature), probabilities in float64.
What HF leaves open is the header's contract: +0.0 and -0.0 are one value (they compare equal here as floats), a NaN logit is -inf
before the arg-max and the top-k, and a row holding +inf after the ban is its arg-max (the lowest id holding +inf), kept = 1."""
from __future__ import annotations

import numpy as np
import torch

CAP = 1024
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Random123's Philox4x32 with 10 rounds: ctr = 4 u32, key = 2 u32 -> 4 u32."""
    c0, c1, c2, c3 = (int(v) & _U32 for v in ctr)
    k0, k1 = (int(v) & _U32 for v in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _U32, p1 & _U32, ((p0 >> 32) ^ c3 ^ k1) & _U32, p0 & _U32
        k0, k1 = (k0 + _W0) & _U32, (k1 + _W1) & _U32
    return c0, c1, c2, c3


def uniform(seed: int, t: int, row: int) -> float:
    """The kernel's u for generated-token index t of row `row`: key = the 64-bit seed, counter = (t, 0, row, 0)."""
    x0 = philox4x32_10((t, 0, row, 0), (seed & _U32, (seed >> 32) & _U32))[0]
    return float(np.float32((x0 >> 8) * (1.0 / 16777216.0)))


def penalize(x: torch.Tensor, seen_ids, penalty: float) -> torch.Tensor:
    """HF RepetitionPenaltyLogitsProcessor on one float32 row: each seen id once."""
    x = x.clone()
    if penalty != 1.0 and len(seen_ids):
        ids = torch.as_tensor(sorted(set(int(i) for i in seen_ids)), dtype=torch.long)
        p = torch.tensor(penalty, dtype=torch.float32)
        v = x[ids]
        x[ids] = torch.where(v < 0, v * p, v / p)
    return x


def sample_row(x: torch.Tensor, top_k: int, top_p: float, inv_temp: float, ban: int = -1, u: float = None, tol: float = 1e-5):
    """One row.  Returns dict(order = candidate ids in (logit desc, id asc) order, kept = size of the final kept set (-1 on
    overflow), probs = float64 renormalised probabilities of the kept ids, out = the id u picks (when u is given), near = the pick
    or the top-p cut lies within `tol` (relative) of a boundary, so float32 summation order may legitimately move it)."""
    x = x.detach().float().clone()
    V = x.numel()
    if ban >= 0:
        x[ban] = float("-inf")
    x[torch.isnan(x)] = float("-inf")
    res = dict(order=None, kept=-1, probs=None, out=int(torch.argmax(x)), near=False)    # argmax: the first of equal maxima
    if bool((x == float("inf")).any()):
        res.update(order=np.array([res["out"]]), kept=1, probs=np.ones(1))
        return res
    y = x * torch.tensor(np.float32(inv_temp))
    y[torch.isnan(y)] = float("-inf")
    if bool((y == float("inf")).any()):                                                  # pushed to +inf by the temperature
        first = int(torch.nonzero(y == float("inf"))[0])
        res.update(order=np.array([first]), kept=1, probs=np.ones(1), out=first)
        return res
    k = min(max(int(top_k), 1), V)
    thr = torch.topk(y, k).values[-1]
    cand = (y >= thr) & torch.isfinite(y)
    ids = torch.nonzero(cand).flatten().numpy()
    if len(ids) == 0 or len(ids) > CAP:
        return res
    yv = y.numpy()[ids].astype(np.float64)
    o = np.lexsort((ids, -yv))
    ids, yv = ids[o], yv[o]
    p = np.exp(yv - yv[0])
    cum = np.cumsum(p)
    S = cum[-1]
    excl = cum - p
    if top_p >= 1.0:
        mk = len(ids)
    else:
        mk = max(int(np.sum(excl < top_p * S)), 1)
        if np.any(np.abs(excl - top_p * S) <= tol * S):
            res["near"] = True
    res.update(order=ids, kept=mk, probs=p[:mk] / cum[mk - 1])
    if u is not None:
        target = u * cum[mk - 1]
        i = min(int(np.sum(cum[:mk] <= target)), mk - 1)
        res["out"] = int(ids[i])
        if np.any(np.abs(cum[:mk] - target) <= tol * cum[mk - 1]):
            res["near"] = True
    return res
