"""The fp64 bounds and the poison of tests/fp64_bounds.py are tight enough to matter: a torch emulation of each kernel form
(bf16 operands, fp32 accumulation in 64-deep k-tiles, K-split slabs, bf16 outputs; online softmax over 64-key tiles with P
rounded to bf16, rotary rounded once) passes assert_within, and each of the mistakes a kernel change could make fails the same
call.  CPU only, a few seconds."""
import pytest
import torch

from tests import fp64_bounds as fb

BF16, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------------------------- GEMM
def emu_gemm(a, b, out, *, alpha=1.0, bias=None, residual=None, gelu=False, splits=1, bf16_slabs=False, mutant=None):
    """out (a window of a wider buffer) = [residual +] act(alpha * a @ b^T [+ bias]) as the split-K path computes it."""
    M, K = a.shape
    N = b.shape[0]
    nt = K // 64
    tps = -(-nt // splits)
    splits = -(-nt // tps)
    slabs = []
    for s in range(splits):
        acc = torch.zeros(M, N, dtype=F32)
        for t in range(s * tps, min(nt, (s + 1) * tps)):
            if mutant == "drop_ktile" and t == nt // 2:
                continue
            acc = acc + a[:, 64 * t:64 * t + 64].float() @ b[:, 64 * t:64 * t + 64].float().T
        slabs.append(fb.bf16_round(acc) if bf16_slabs else acc)
    if mutant == "slab_twice":
        slabs.append(slabs[-1])
    acc = slabs[0]
    for p in slabs[1:]:
        acc = acc + p
    if mutant == "bias_before_alpha":
        v = (acc + bias) * alpha
    else:
        v = acc * alpha + (bias if bias is not None else 0.0)
    if gelu:
        v = torch.nn.functional.gelu(v)
    if residual is not None:
        v = v + residual
    rows, cols = M, N
    if mutant == "skip_col_tail":
        cols = N - (N % 16 or 16)
    if mutant == "skip_row_tile":
        rows = (M - 1) // 64 * 64
    out[:rows, :cols] = v[:rows, :cols].to(out.dtype)


GEMM_CASES = [  # M, N, K, splits, bf16 slabs, alpha, bias, gelu, residual, out dtype
    (70, 136, 512, 3, True, 0.5, True, False, True, F32),
    (130, 1001, 256, 1, False, 1.0, True, True, False, BF16),
    (65, 200, 640, 4, False, 2.0, True, False, False, BF16),
]
GEMM_MUTANTS = ["drop_ktile", "skip_col_tail", "skip_row_tile", "slab_twice", "bias_before_alpha"]


def _gemm_case(M, N, K, splits, sbf, alpha, has_bias, gelu, has_res, dt, mutant):
    a = fb.rnd(M, K, seed=1).to(BF16)
    b = (fb.rnd(N, K, seed=2) * 0.05).to(BF16)
    bias = fb.rnd(N, seed=3) if has_bias else None
    res = fb.rnd(M, N, seed=4) if has_res else None
    ld = (N + 16 + 7) // 8 * 8
    buf = fb.poisoned((M + 2, ld), dt, "cpu")
    win = buf[1:M + 1, 8:8 + N]
    emu_gemm(a, b, win, alpha=alpha, bias=bias, residual=res, gelu=gelu, splits=splits, bf16_slabs=sbf, mutant=mutant)
    ref, bnd = fb.gemm_ref_bound(a, b, alpha=alpha, bias=bias, residual=res, gelu=gelu, out_bf16=dt == BF16, splits=splits,
                                 bf16_slabs=sbf)
    ratio = fb.assert_within(win, ref, bnd, f"gemm {M}x{N}x{K}")
    fb.assert_untouched(buf[0], "row above")
    fb.assert_untouched(buf[M + 1], "row below")
    fb.assert_untouched(buf[:, :8], "left columns")
    fb.assert_untouched(buf[:, 8 + N:], "right columns")
    return ratio


@pytest.mark.parametrize("case", GEMM_CASES)
def test_gemm_emulation_is_within_the_bound(case):
    ratio = _gemm_case(*case, None)
    assert ratio > 1e-3, "the bound is so loose that the emulation's rounding does not register"


# every mutant on every case where it changes the arithmetic (a slab counted twice needs a split, bias before alpha needs alpha != 1)
GEMM_MUTANT_CASES = [(c, m) for c in GEMM_CASES for m in GEMM_MUTANTS
                     if not (m == "slab_twice" and c[3] == 1) and not (m == "bias_before_alpha" and c[5] == 1.0)]


@pytest.mark.parametrize("case,mutant", GEMM_MUTANT_CASES)
def test_gemm_mutant_fails_the_bound(case, mutant):
    with pytest.raises(AssertionError):
        _gemm_case(*case, mutant)


# -------------------------------------------------------------------------------------------------------------- attention
def emu_attn_rope(q, k, v, pos, cos, sin, scale, kv_len, mutant=None):
    """Causal rotary attention as the kernels compute it: q / k rotated in fp32 and rounded to bf16 once, scores in fp32,
    online softmax over 64-key tiles (running max, rescale of the accumulator and the row sum), P rounded to bf16 before P V,
    output rounded to bf16.  q, k, v [B, H, S, D] bf16; returns (o [B, H, S, D] bf16, lse [B, H, S] f32)."""
    B, H, S, D = q.shape
    qr = fb.rope64(q.float(), pos, cos, sin).to(BF16).float()
    kr = fb.rope64(k.float(), pos, cos, sin)
    if mutant == "rope_sign":                               # the key of one position rotated the wrong way
        kr[:, :, 37] = fb.rope64(k.float(), pos, cos, sin, sign=-1.0)[:, :, 37]
    kr = kr.to(BF16).float()
    vf = v.float()
    o = torch.zeros(B, H, S, D)
    lse = torch.zeros(B, H, S)
    i = torch.arange(S)[:, None]
    for b in range(B):
        kvl = int(kv_len[b]) + (1 if mutant == "kv_len_off_by_one" else 0)
        m = torch.full((H, S, 1), float("-inf"))
        lsum = torch.zeros(H, S, 1)
        acc = torch.zeros(H, S, D)
        for t0 in range(0, S, 64):
            j = torch.arange(t0, min(S, t0 + 64))[None]
            s = (qr[b] @ kr[b, :, t0:t0 + 64].transpose(-1, -2)) * scale
            s = s.masked_fill(~((j <= i) & (j < kvl))[None], float("-inf"))
            m_new = torch.maximum(m, s.amax(-1, keepdim=True))
            alpha = torch.where(m_new == float("-inf"), torch.ones_like(m), torch.exp(m - m_new))
            if mutant == "skip_rescale" and t0 == 128:
                alpha = torch.ones_like(alpha)
            e = torch.where(m_new == float("-inf"), torch.zeros_like(s), torch.exp(s - m_new))
            lsum = lsum * alpha + e.sum(-1, keepdim=True)
            acc = acc * alpha + fb.bf16_round(e) @ vf[b, :, t0:t0 + 64]
            m = m_new
        o[b] = acc / lsum
        lse[b] = (m + torch.log(lsum))[..., 0]
    return o.to(BF16), lse


def emu_attn_bwd(qr, kr, v, o, lse, dout, scale, mask, mutant=None):
    """The backward as the kernels compute it from their inputs: P = exp(s - lse) in fp32, dP = dO v^T, delta = rowsum(o dO)
    from the bf16 o, dS = P (dP - delta) rounded to bf16, dq / dk accumulated in fp32 over 64-key / 64-query tiles, dv from P
    rounded to bf16; outputs rounded to bf16.  All [B, H, S, D]; qr / kr are the rotated bf16 operands."""
    qf, kf, vf, g = qr.float(), kr.float(), v.float(), dout.float()
    s = (qf @ kf.transpose(-1, -2)) * scale
    s = s.masked_fill(~mask, float("-inf"))
    P = torch.exp(s - lse[..., None])
    if mutant == "bwd_skip_rescale":                        # P of the third key tile left relative to the first two tiles' max
        m_pre = s[..., :128].amax(-1, keepdim=True)
        m_all = s.amax(-1, keepdim=True)
        P[..., 128:] = P[..., 128:] * torch.exp(m_all - m_pre)
    delta = (g * o.float()).sum(-1, keepdim=True)
    if mutant == "delta_2pct":
        delta = delta * 1.02
    dS = fb.bf16_round(P * (g @ vf.transpose(-1, -2) - delta))
    S = qr.shape[-2]
    dq = torch.zeros_like(qf)
    for t0 in range(0, S, 64):
        if mutant == "dq_drop_key_tile" and t0 == 64:
            continue
        dq = dq + scale * dS[..., t0:t0 + 64] @ kf[..., t0:t0 + 64, :]
    dSk = dS.clone()
    if mutant == "dk_missing_query":
        dSk[..., 120, :] = 0
    dk = torch.zeros_like(kf)
    for t0 in range(0, S, 64):
        dk = dk + scale * dSk[..., t0:t0 + 64, :].transpose(-1, -2) @ qf[..., t0:t0 + 64, :]
    dv = fb.bf16_round(P).transpose(-1, -2) @ g
    if mutant == "dq_zero_row":
        dq[0, 1, 100] = 0
    if mutant == "dk_zero_row":
        dk[1, 0, 96] = 0                                    # the last valid key of the ragged row
    return dq.to(BF16), dk.to(BF16), dv.to(BF16)


ATTN_MUTANTS = ["kv_len_off_by_one", "skip_rescale", "rope_sign"]
BWD_MUTANTS = ["dq_drop_key_tile", "dq_zero_row", "dk_zero_row", "dk_missing_query", "delta_2pct", "bwd_skip_rescale"]


def _attn_case(mutant):
    B, H, S, D = 2, 2, 150, 64
    q = fb.rnd(B, H, S, D, seed=11).to(BF16)
    k = fb.rnd(B, H, S, D, seed=12).to(BF16)
    v = fb.rnd(B, H, S, D, seed=13).to(BF16)
    kv_len = torch.tensor([150, 97])
    k[1, :, 97:] = 1e4                                      # keys / values past kv_len: large, so a mask off by one is decisive
    v[1, :, 97:] = -1e4
    k[0, :, 140] = (q[0, :, 139].float() * 4).to(BF16)      # a late score spike: the running max jumps in the last key tile
    pos = torch.arange(S)[None] + 5 * torch.arange(B)[:, None]
    cos, sin = fb.rope_tables(D)
    scale = D ** -0.5
    o, lse = emu_attn_rope(q, k, v, pos, cos, sin, scale, kv_len, None if mutant in BWD_MUTANTS else mutant)
    qr, qe = fb.rope_bf16(q.float(), pos, cos, sin)
    kr, ke = fb.rope_bf16(k.float(), pos, cos, sin)
    mask = fb.attn_mask(B, S, S, True, kv_len, "cpu")
    valid = (torch.arange(S)[None] < kv_len[:, None])[:, None, :, None]
    dout = (fb.rnd(B, H, S, D, seed=14) * valid).to(BF16)
    r = fb.attn_ref_bound(qr, kr, v, scale, mask, q_err=qe, k_err=ke, dout=dout, o_in=o, lse_in=lse)
    ratios = [fb.assert_within(o, r["o"], r["o_bound"], "attention o"), fb.assert_within(lse, r["lse"], r["lse_bound"], "lse")]
    # the backward reads the rotation the forward used (the same fp32 rounding as the kernels)
    qk = fb.rope64(q.float(), pos, cos, sin).to(BF16)
    kk = fb.rope64(k.float(), pos, cos, sin).to(BF16)
    grads = emu_attn_bwd(qk, kk, v, o, lse, dout, scale, mask, mutant if mutant in BWD_MUTANTS else None)
    for nm, got in zip(("dq", "dk", "dv"), grads):
        ratios.append(fb.assert_within(got, r[nm], r[nm + "_bound"], "attention " + nm))
    return ratios


def test_attention_emulation_is_within_the_bound():
    ratios = _attn_case(None)
    assert min(ratios) > 1e-3, ratios


@pytest.mark.parametrize("mutant", ATTN_MUTANTS + BWD_MUTANTS)
def test_attention_mutant_fails_the_bound(mutant):
    with pytest.raises(AssertionError, match="out of bound"):
        _attn_case(mutant)
