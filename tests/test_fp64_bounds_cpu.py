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


# ------------------------------------------------------------------------------------------------------------ row kernels
def emu_row_sum(terms, skip_last_chunk=False):
    """Sum over the last axis of fp32 terms [M, D] (D % 4 == 0) in the row kernels' order: thread t adds its float4 chunks
    (columns 4 t + 1024 k) serially, each chunk as ((a + b) + c) + d; a 64-lane butterfly; the four wave values in order."""
    M, D = terms.shape
    if skip_last_chunk:
        terms = terms.clone()
        terms[:, D - 4:] = 0
    K = -(-D // 1024)
    t = torch.zeros(M, K * 1024, dtype=F32)
    t[:, :D] = terms
    t = t.view(M, K, 256, 4)
    chunk = ((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3]
    s = torch.zeros(M, 256, dtype=F32)
    for k in range(K):
        s = s + chunk[:, k]
    v = s.view(M, 4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    out = torch.zeros(M, dtype=F32)
    for w in range(4):
        out = out + v[:, w, 0]
    return out[:, None]


def emu_block_sum(part):
    """block_sum of per-thread fp32 values [M, 64 NW]: a 64-lane butterfly in each wave, then the NW wave values in order."""
    M = part.shape[0]
    v = part.view(M, -1, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    out = torch.zeros(M, dtype=F32)
    for w in range(v.shape[1]):
        out = out + v[:, w, 0]
    return out[:, None]


def emu_strided_sum(terms, nt=256):
    """Thread t adds elements t, t + nt, ... serially (sum_kernel, pmax_kernel, the low-rank dot products); then block_sum."""
    M, n = terms.shape
    K = -(-n // nt)
    t = torch.zeros(M, K * nt, dtype=F32)
    t[:, :n] = terms
    t = t.view(M, K, nt)
    part = torch.zeros(M, nt, dtype=F32)
    for k in range(K):
        part = part + t[:, k]
    return emu_block_sum(part)


def emu_rmsnorm_fwd(x, w, eps, out, mutant=None):
    M, D = x.shape
    ss = emu_row_sum(x * x, mutant == "skip_last_float4")
    if mutant == "eps_dropped":
        r = torch.rsqrt(ss / D)
    elif mutant == "eps_outside":
        r = torch.rsqrt(ss / D) + eps
    else:
        r = torch.rsqrt(ss / D + eps)
    y = (w * (x * r)).to(BF16)
    rows = [m for m in range(M) if not (mutant == "skip_row" and m == M // 2)]
    if mutant == "ldy_as_D":                                  # row m lands at flat offset m * D of the window's storage
        flat = out.as_strided((M * D,), (1,), out.storage_offset())
        flat[:] = y.reshape(-1)
        return
    out[rows] = y[rows]


def emu_rmsnorm_bwd(dy, x, w, eps, dres, dx, dxb, mutant=None):
    M, D = x.shape
    ss = emu_row_sum(x * x, mutant == "skip_last_float4")
    dot = emu_row_sum(x * w * dy, mutant == "skip_last_float4")
    r = torch.rsqrt(ss / D + eps)
    cc = r * r * r * dot / D
    o = (r * w) * dy - x * cc
    ob = o + dres
    if mutant != "dres_not_added":
        o = o + dres
    if mutant != "bf16_before_dres":
        ob = o
    else:
        ob = ob - dres
    dx[:] = o
    dxb[:] = ob.to(BF16)


def emu_layernorm(x, w, b, eps, dy, dres, mutant=None):
    """(y f32, y bf16, dx f32, dx bf16) as layernorm_fwd_kernel / layernorm_bwd_kernel compute them."""
    M, D = x.shape
    skip = mutant == "skip_last_float4"
    mean = emu_row_sum(x, skip) / D
    if mutant == "mean_of_previous_row":
        mean = torch.roll(mean, 1, 0)
    d = x - mean
    var = emu_row_sum(d * d, skip) / D
    if mutant == "eps_dropped":
        r = torch.rsqrt(var)
    elif mutant == "eps_outside":
        r = torch.rsqrt(var) + eps
    else:
        r = torch.rsqrt(var + eps)
    y = d * r * w + b
    gw = dy * w
    sg = emu_row_sum(gw, skip) / D
    sgx = emu_row_sum(gw * d * r, skip) / D
    dx = r * (gw - sg - d * r * sgx)
    if mutant != "dres_not_added":
        dx = dx + dres
    return y, y.to(BF16), dx, dx.to(BF16)


NORM_EPS = [1e-6, 1e-5, 1e-12]
NORM_CPU_CASES = [(7, 252, 1e-6), (13, 1028, 1e-12), (6, 4100, 1e-5), (1, 4, 1e-6)]
RMS_FWD_MUTANTS = ["skip_last_float4", "eps_dropped", "eps_outside", "skip_row", "ldy_as_D"]
RMS_BWD_MUTANTS = ["skip_last_float4", "dres_not_added", "bf16_before_dres"]
LN_MUTANTS = ["skip_last_float4", "eps_dropped", "eps_outside", "mean_of_previous_row", "dres_not_added"]


def _rms_case(M, D, eps, mutant, which):
    x, w = fb.norm_rows(M, D, seed=21), fb.norm_weight(D, seed=22)
    dy, dres = fb.rnd(M, D, seed=23), fb.rnd(M, D, seed=24)
    r = fb.rmsnorm_ref_bound(x, w, eps, dy=dy, dres=dres)
    ratios = []
    if which == "fwd":
        buf = fb.poisoned((M + 2, D + 72), BF16, "cpu")
        win = buf[1:M + 1, 8:8 + D]
        emu_rmsnorm_fwd(x, w, eps, win, mutant)
        ratios.append(fb.assert_within(win, r["y"], r["y_bf16_bound"], "rmsnorm fwd"))
        fb.assert_frame_untouched(buf, slice(1, M + 1), slice(8, 8 + D), "rmsnorm fwd")
    else:
        dx, dxb = fb.poisoned((M, D), F32, "cpu"), fb.poisoned((M, D), BF16, "cpu")
        emu_rmsnorm_bwd(dy, x, w, eps, dres, dx, dxb, mutant)
        ratios.append(fb.assert_within(dx, r["dx"], r["dx_bound"], "rmsnorm bwd f32"))
        ratios.append(fb.assert_within(dxb, r["dx"], r["dx_bf16_bound"], "rmsnorm bwd bf16"))
    return ratios


def _ln_case(M, D, eps, mutant):
    x, w, b = fb.norm_rows(M, D, seed=31), fb.norm_weight(D, seed=32), 0.1 * fb.rnd(D, seed=33)
    dy, dres = fb.rnd(M, D, seed=34), fb.rnd(M, D, seed=35)
    r = fb.layernorm_ref_bound(x, w, b, eps, dy=dy, dres=dres)
    y, yb, dx, dxb = emu_layernorm(x, w, b, eps, dy, dres, mutant)
    return [fb.assert_within(y, r["y"], r["y_bound"], "layernorm y f32"),
            fb.assert_within(yb, r["y"], r["y_bf16_bound"], "layernorm y bf16"),
            fb.assert_within(dx, r["dx"], r["dx_bound"], "layernorm dx f32"),
            fb.assert_within(dxb, r["dx"], r["dx_bf16_bound"], "layernorm dx bf16")]


@pytest.mark.parametrize("M,D,eps", NORM_CPU_CASES)
def test_norm_emulations_are_within_the_bound(M, D, eps):
    ratios = _rms_case(M, D, eps, None, "fwd") + _rms_case(M, D, eps, None, "bwd") + _ln_case(M, D, eps, None)
    assert max(ratios) > 1e-3, "the bounds are so loose that the emulation's rounding does not register"


@pytest.mark.parametrize("mutant", RMS_FWD_MUTANTS)
def test_rmsnorm_fwd_mutant_fails(mutant):
    with pytest.raises(AssertionError):
        _rms_case(13, 1028, 1e-6, mutant, "fwd")


@pytest.mark.parametrize("mutant", RMS_BWD_MUTANTS)
def test_rmsnorm_bwd_mutant_fails(mutant):
    with pytest.raises(AssertionError):
        _rms_case(13, 1028, 1e-6, mutant, "bwd")


@pytest.mark.parametrize("mutant", LN_MUTANTS)
def test_layernorm_mutant_fails(mutant):
    with pytest.raises(AssertionError):
        _ln_case(13, 1028, 1e-6, mutant)


def test_norm_generators_keep_every_row_well_defined():
    """The condition on the inputs: no row's variance is lost to the mean's rounding unless the row is constant
    (layernorm_ref_bound raises otherwise), at every width and eps the GPU module uses."""
    for D in (4, 252, 256, 1028, 1408, 4096, 4100, 8192):
        for eps in NORM_EPS:
            x = fb.norm_rows(12, D, seed=D)
            fb.layernorm_ref_bound(x, fb.norm_weight(D, seed=1), torch.zeros(D), eps)


# -------------------------------------------------------------------------------------------------------------- clamp-CE
def emu_clamp_ce(x, labels, gscale, row_loss, dlog, V, mutant=None):
    """clamp_ce_wide_kernel's arithmetic on fp32 logits [R, V]; dlog is the [R, ldd] window (pad columns zeroed)."""
    R = x.shape[0]
    ldd = dlog.shape[1]
    Vs = V - V % 4 if mutant == "tail_dropped" else V
    m = x[:, :Vs].amax(1, keepdim=True)
    e = torch.exp(x - m)
    assert V <= 8 * 4096
    terms = torch.zeros(R, 8, 1024, 4, dtype=F32)            # chunk i of thread t: columns (i * 1024 + t) * 4 .. + 3
    terms.view(R, -1)[:, :Vs] = e[:, :Vs]
    part = torch.zeros(R, 1024, dtype=F32)
    for i in range(8):                                       # the thread's 32 exponentials, serially
        for q in range(4):
            part = part + terms[:, i, :, q]
    se = emu_block_sum(part)
    inv = 1.0 / se
    for i in range(R):
        t = int(labels[i])
        gate = 0.0
        if 0 <= t < V:
            pt = torch.exp(x[i, t] - m[i, 0]) * inv[i, 0]
            row_loss[i] = -torch.log(pt.clamp(fb.CE_LO, fb.CE_HI))
            gate = gscale if (fb.CE_LO <= float(pt) <= fb.CE_HI or mutant == "gate_not_applied") else 0.0
        else:
            row_loss[i] = 0.0
            if mutant == "ignored_row_gets_gradient":
                gate, t = gscale, 0
        g = torch.zeros(ldd, dtype=F32)
        if gate != 0.0:
            g[:V] = gate * (e[i] * inv[i, 0])
            g[t + (1 if mutant == "onehot_off_by_one" and t + 1 < V else 0)] -= gate
        n = V if mutant == "pad_not_zeroed" else ldd
        dlog[i, :n] = g[:n].to(BF16)


CE_MUTANTS = ["tail_dropped", "pad_not_zeroed", "gate_not_applied", "ignored_row_gets_gradient", "onehot_off_by_one"]


def _ce_case(V, ldd, mutant):
    R = 12
    x, y = fb.ce_case(R, V, seed=V)
    if mutant == "tail_dropped":
        x[9, V - 1] = x[9].max() + 3                          # the row's maximum sits in the scalar tail
    loss = fb.poisoned((R,), F32, "cpu")
    buf = fb.poisoned((R + 2, ldd + 16), BF16, "cpu")
    win = buf[1:R + 1, 8:8 + ldd]
    emu_clamp_ce(x, y, 0.125, loss, win, V, mutant)
    r = fb.clamp_ce_ref_bound(x, y, 0.125, ldd=ldd)
    assert int(r["amb"].sum()) == 0                          # the generator keeps every row decisively off the thresholds
    ratios = fb.clamp_ce_check(loss, win, r)
    fb.assert_frame_untouched(buf, slice(1, R + 1), slice(8, 8 + ldd), "clamp_ce")
    return ratios


@pytest.mark.parametrize("V,ldd", [(1001, 1024), (320, 320), (1003, 1007)])
def test_clamp_ce_emulation_is_within_the_bound(V, ldd):
    assert max(_ce_case(V, ldd, None)) > 1e-3


@pytest.mark.parametrize("mutant", CE_MUTANTS)
def test_clamp_ce_mutant_fails(mutant):
    with pytest.raises(AssertionError):
        _ce_case(1001, 1024, mutant)


def test_clamp_ce_threshold_row_may_take_either_branch_and_nothing_else():
    """A row with p_t on the lower threshold is ambiguous: gradient or zeros both pass; a wrong loss still fails."""
    V = 64
    x = torch.zeros(2, V)
    x[0, 5] = float(torch.log(torch.tensor(fb.CE_LO * (V - 1) / (1 - fb.CE_LO), dtype=torch.float64)))
    y = torch.tensor([5, 7])
    r = fb.clamp_ce_ref_bound(x, y, 1.0)
    assert r["amb"].tolist() == [True, False]
    for branch in ("live", "dead"):
        loss, d = fb.poisoned((2,), F32, "cpu"), fb.poisoned((2, V), BF16, "cpu")
        emu_clamp_ce(x, y, 1.0, loss, d, V)
        d[0] = (r["dlog"][0] if bool(r["inside"][0]) == (branch == "live") else r["dlog_alt"][0]).to(BF16)
        fb.clamp_ce_check(loss, d, r)
    loss[0] = loss[0] * 1.01
    with pytest.raises(AssertionError, match="neither branch"):
        fb.clamp_ce_check(loss, d, r)


@pytest.mark.parametrize("V", [320, 1001, 32000, 32001, 32768, 32772, 50000])
def test_clamp_ce_generator_has_no_threshold_rows(V):
    """The condition on the inputs: at every vocabulary size the GPU module uses, no generated row is a threshold row."""
    x, y = fb.ce_case(12, V, seed=V)
    r = fb.clamp_ce_ref_bound(x, y, 0.125)
    assert int(r["amb"].sum()) == 0
    assert r["has"].tolist() == [True] * 3 + [False] * 2 + [True] * 7 and not bool(r["inside"][6:9].any())


# ----------------------------------------------------------------------------------------------------------- elementwise
def emu_silu(gu, I, blk, dh=None, read_blk=None, drop_term=False, sweep_limit=None):
    """silu_mul fwd (dh None) or bwd on bf16 gu [M, 2 I] in the plain (blk 0) or interleaved layout, fp32 arithmetic."""
    read_blk = blk if read_blk is None else read_blk
    M = gu.shape[0]
    c = torch.arange(I)
    gc = c if read_blk == 0 else (c // read_blk) * 2 * read_blk + c % read_blk
    us = I if read_blk == 0 else read_blk
    g, u = gu[:, gc].float(), gu[:, gc + us].float()
    s = 1.0 / (1.0 + torch.exp(-g))
    if dh is None:
        out = fb.poisoned((M, I), BF16, "cpu")
        res = (g * s * u).to(BF16)
        n = M * I if sweep_limit is None else sweep_limit
        out.view(-1)[:n] = res.view(-1)[:n]
        return out
    d = dh.float()
    silu = g * s
    dgu = fb.poisoned((M, 2 * I), BF16, "cpu")
    dgu[:, gc] = (d * u * (s if drop_term else s + silu * (1 - s))).to(BF16)
    dgu[:, gc + us] = (d * silu).to(BF16)
    return dgu


def ew_values(*shape, seed):
    """bf16 values spanning +-30 (saturation on both sides) with N(0, 1) in between."""
    x = fb.rnd(*shape, seed=seed)
    flat = x.view(-1)
    flat[::7] *= 10
    flat[0], flat[1], flat[2], flat[3] = 30.0, -30.0, 0.0, -0.0
    return x.to(BF16)


def _silu_case(blk, mutant):
    M, I = 9, 256
    gu, dh = ew_values(M, 2 * I, seed=41), ew_values(M, I, seed=42)
    c = torch.arange(I)
    gc = c if blk == 0 else (c // blk) * 2 * blk + c % blk
    us = I if blk == 0 else blk
    h, hb, dg, dgb, du, dub = fb.silu_mul_ref_bound(gu[:, gc], gu[:, gc + us], dh)
    kw = dict(read_blk=0) if mutant == "blk_read_as_plain" else {}
    got = emu_silu(gu, I, blk, sweep_limit=M * I // 2 if mutant == "second_sweep_skipped" else None, **kw)
    ratios = [fb.assert_within(got, h, hb, "silu fwd")]
    dgu = emu_silu(gu, I, blk, dh, drop_term=mutant == "silu_grad_term_dropped", **kw)
    ratios.append(fb.assert_within(dgu[:, gc], dg, dgb, "silu bwd dg"))
    ratios.append(fb.assert_within(dgu[:, gc + us], du, dub, "silu bwd du"))
    return ratios


@pytest.mark.parametrize("blk", [0, 128])
def test_silu_emulation_is_within_the_bound(blk):
    assert max(_silu_case(blk, None)) > 1e-3


@pytest.mark.parametrize("blk,mutant", [(0, "second_sweep_skipped"), (0, "silu_grad_term_dropped"), (128, "blk_read_as_plain")])
def test_silu_mutant_fails(blk, mutant):
    with pytest.raises(AssertionError):
        _silu_case(blk, mutant)


def test_gelu_emulation_is_within_the_bound_and_a_tanh_form_is_not():
    x, dy = ew_values(16, 64, seed=43), ew_values(16, 64, seed=44)
    xf = x.float().requires_grad_(True)
    y = torch.nn.functional.gelu(xf)
    (y * dy.float()).sum().backward()
    ref, bnd = fb.gelu_ref_bound(x)
    fb.assert_within(y.detach().to(BF16), ref, bnd, "gelu fwd")
    rb, bb = fb.gelu_ref_bound(x, dy)
    fb.assert_within(xf.grad.to(BF16), rb, bb, "gelu bwd")
    with pytest.raises(AssertionError):
        fb.assert_within(torch.nn.functional.gelu(x.float(), approximate="tanh").to(BF16), ref, bnd, "gelu tanh")


def _rope_case(sign, mutant):
    n, nh, d, col0, ld = 37, 3, 88, 8, 3 * 88 + 24
    x = fb.rnd(n, ld, seed=51).to(BF16)
    cos, sin = fb.rope_tables(d, 64)
    pos = torch.randint(0, 64, (n,), generator=torch.Generator().manual_seed(5)).int()          # non-monotone, repeated
    ref, amb = fb.rope_rows_ref(x, col0, nh, d, pos, cos, sin, sign)
    assert float((amb > 0).double().mean()) <= 0.01
    xs = x[:, col0:col0 + nh * d].float().reshape(1, n, nh, d).transpose(1, 2)
    got = fb.rope64(xs, pos.long()[None], cos, sin, 1.0 if mutant == "sign_ignored" else sign).to(BF16)
    return fb.assert_within(got.transpose(1, 2).reshape(n, -1), ref, amb, "rope")


def test_rope_emulation_matches_and_an_ignored_sign_does_not():
    _rope_case(1.0, None)
    _rope_case(-1.0, None)
    with pytest.raises(AssertionError):
        _rope_case(-1.0, "sign_ignored")


# --------------------------------------------------------------------------------------------------------------- gathers
def emu_expand_rows(src, inv, M, mutant=None):
    out = fb.poisoned((M, src.shape[1]), src.dtype, "cpu")
    for m in range(M):
        i = int(inv[m * 2] if mutant == "index_stride" else inv[m])
        if i >= 0:
            out[m] = src[i]
        elif mutant != "negative_left_unwritten":
            out[m] = 0
    return out


@pytest.mark.parametrize("mutant", [None, "negative_left_unwritten", "index_stride"])
def test_expand_rows_reference_catches_unwritten_and_misindexed_rows(mutant):
    src = fb.rnd(5, 8, seed=61)
    inv = torch.tensor([3, -1, 0, 0, 4, -1, 2, 1, -1, 3, 3, -1, 0, 2], dtype=torch.int32)
    M = 7
    want = torch.where((inv[:M] >= 0)[:, None], src[inv[:M].clamp_min(0).long()], torch.zeros(M, 8))

    def check():
        got = emu_expand_rows(src, inv, M, mutant)
        assert not bool(fb.untouched(got).any()) and torch.equal(got, want)

    if mutant is None:
        check()
    else:
        with pytest.raises(AssertionError):
            check()


# ------------------------------------------------------------------------------- l2norm, sum, arg-max / p_max, dropout, GELU'
L2_MUTANTS = ["skip_last_float4", "eps_inside_sqrt", "clamp_omitted"]


def _l2norm_case(M, D, mutant):
    x = fb.norm_rows(M, D, seed=71)
    ss = emu_row_sum(x * x, mutant == "skip_last_float4")
    if mutant == "eps_inside_sqrt":
        n = torch.sqrt(ss + 1e-6)
    elif mutant == "clamp_omitted":
        n = torch.sqrt(ss)
    else:
        n = torch.sqrt(ss).clamp_min(1e-6)
    y = x * (1.0 / n)
    ref, e, eb = fb.l2norm_ref_bound(x, 1e-6)
    return [fb.assert_within(y, ref, e, "l2norm f32"), fb.assert_within(y.to(BF16), ref, eb, "l2norm bf16")]


@pytest.mark.parametrize("M,D", [(7, 252), (6, 1028), (1, 4)])
def test_l2norm_emulation_is_within_the_bound(M, D):
    assert max(_l2norm_case(M, D, None)) > 1e-3


@pytest.mark.parametrize("mutant", L2_MUTANTS)
def test_l2norm_mutant_fails(mutant):
    with pytest.raises(AssertionError):
        _l2norm_case(7, 252, mutant)


def _sum_case(mutant):
    n = 1003
    x = fb.rnd(n, seed=72)
    x[1::2] = -x[::2][:n // 2] * (1 + 2 ** -10)              # nearly cancelling pairs: |sum| << sum |x|
    terms = x[None].clone()
    if mutant == "tail_dropped":
        terms[:, n - n % 256:] = 0
    got = emu_strided_sum(terms)[0] * torch.tensor(3.0)
    ref, b = fb.sum_ref_bound(x, 3.0)
    return fb.assert_within(got, ref.reshape(1), b.reshape(1), "sum_f32")


def test_sum_emulation_is_within_the_bound_and_a_dropped_tail_is_not():
    assert _sum_case(None) > 1e-3
    with pytest.raises(AssertionError):
        _sum_case("tail_dropped")


def _pmax_case(mutant, inv_temp=0.7):
    R, V, ban = 4, 1001, 999
    x = fb.rnd(R, V, seed=73) * 3
    x[1, 300] = x[1].max() + 1.0
    x[1, 307] = x[1, 300]                                    # a tie
    x[2, ban] = x[2].max() + 5.0
    ids_r, mar_r, mar_b, pm_r, pm_b = fb.argmax_ref(x, ban, inv_temp)
    xb = x.clone()
    xb[:, ban] = float("-inf")
    top = xb.topk(2, 1).values
    ids = xb.argmax(1)
    if mutant == "tie_to_later_index":
        ids[1] = 307
    assert torch.equal(ids, ids_r), "arg-max ids"
    fb.assert_within(top[:, 0] - top[:, 1], mar_r, mar_b, "margin")
    a = (xb - top[:, :1]) * (1.0 if mutant == "inv_temp_ignored" else torch.tensor(inv_temp))
    if mutant == "ban_counted":
        a[:, ban] = (x[:, ban] - top[:, 0]) * inv_temp
    pm = 1.0 / emu_strided_sum(torch.exp(a))[:, 0]
    return fb.assert_within(pm, pm_r, pm_b, "p_max")


def test_pmax_emulation_is_within_the_bound():
    assert _pmax_case(None) > 1e-3 and int(fb.argmax_ref(fb.rnd(2, 8, seed=1) * 0, -1)[0][0]) == 0


@pytest.mark.parametrize("mutant", ["inv_temp_ignored", "tie_to_later_index", "ban_counted"])
def test_pmax_mutant_fails(mutant):
    with pytest.raises(AssertionError):
        _pmax_case(mutant)


def _dropout_case(mutant):
    p = 0.1
    x, acc, dy = ew_values(8, 64, seed=74), fb.rnd(8, 64, seed=75), fb.rnd(8, 64, seed=76)
    keep = (torch.rand(8, 64, generator=torch.Generator().manual_seed(7)) >= p).float() * torch.tensor(1 / (1 - p))
    used = (keep > 0).float() if mutant == "scale_missing" else (torch.roll(keep, 1, 1) if mutant == "mask_shifted" else keep)
    ref = x.double() * keep.double()
    r1 = fb.assert_within((x.float() * used).to(BF16), ref, fb.bf16_out(ref, fb.U32 * ref.abs()), "dropout_bf16")
    add = dy.double() * keep.double()
    ref2 = acc.double() + add
    r2 = fb.assert_within(acc + dy * used, ref2, fb.U32 * (add.abs() + ref2.abs()), "dropout_add_")
    return max(r1, r2)


def test_dropout_emulation_is_within_the_bound_and_wrong_masks_are_not():
    assert _dropout_case(None) > 1e-3
    for mutant in ("scale_missing", "mask_shifted"):
        with pytest.raises(AssertionError):
            _dropout_case(mutant)


def test_gelu_backward_mutants_fail():
    x, dy = ew_values(16, 64, seed=43), ew_values(16, 64, seed=44)
    ref, bnd = fb.gelu_ref_bound(x, dy)
    xf = x.float()
    cdf = 0.5 * torch.special.erfc(-xf / 2 ** 0.5)
    pdf = torch.exp(-xf * xf / 2) * 0.3989422804014327
    fb.assert_within((dy.float() * (cdf + xf * pdf)).to(BF16), ref, bnd, "gelu bwd")
    for wrong in (cdf, cdf + pdf, cdf - xf * pdf):           # the x pdf term dropped, without its x, with the wrong sign
        with pytest.raises(AssertionError):
            fb.assert_within((dy.float() * wrong).to(BF16), ref, bnd, "gelu bwd mutant")


# ------------------------------------------------------------------------------------------------ LayerNorm parameter gradients
def emu_param_grads(dy, x, eps, keep=None, prev=None, mutant=None):
    """layernorm_param_partial_kernel + reduce: the row statistics as the LayerNorm kernels compute them, a column summed
    serially over the 16 rows of a block, then the blocks in order."""
    M, D = x.shape
    mean = emu_row_sum(x) / D
    d = x - mean
    r = torch.rsqrt(emu_row_sum(d * d) / D + eps)
    if mutant == "mean_not_subtracted":
        d = x
    g = dy * keep if keep is not None and mutant != "mask_ignored" else dy
    tg, tb = g * (d * r), g
    dg, db = torch.zeros(D), torch.zeros(D)
    nblk = -(-M // 16)
    for blk in range(nblk - (1 if mutant == "last_block_dropped" else 0)):
        pg, pb = torch.zeros(D), torch.zeros(D)
        for m in range(16 * blk, min(M, 16 * blk + 16)):
            pg, pb = pg + tg[m], pb + tb[m]
        dg, db = dg + pg, db + pb
    if prev is not None and mutant != "accumulate_overwrites":
        dg, db = prev[0] + dg, prev[1] + db
    return dg, db


PG_MUTANTS = ["mean_not_subtracted", "mask_ignored", "last_block_dropped", "accumulate_overwrites"]


def _pg_case(M, D, eps, mutant):
    x, dy = fb.norm_rows(M, D, seed=81), fb.rnd(M, D, seed=82)
    keep = (torch.rand(M, D, generator=torch.Generator().manual_seed(8)) >= 0.1).float() * torch.tensor(1 / 0.9)
    prev = (fb.rnd(D, seed=83), fb.rnd(D, seed=84))
    dg, db = emu_param_grads(dy, x, eps, keep, prev, mutant)
    rg, eg, rb, eb = fb.layernorm_param_grads_ref_bound(dy, x, eps, keep, prev)
    return [fb.assert_within(dg, rg, eg, "dgamma"), fb.assert_within(db, rb, eb, "dbeta")]


@pytest.mark.parametrize("M,D,eps", [(37, 252, 1e-6), (1, 4, 1e-12), (20, 1028, 1e-5)])
def test_param_grads_emulation_is_within_the_bound(M, D, eps):
    assert max(_pg_case(M, D, eps, None)) > 1e-3


@pytest.mark.parametrize("mutant", PG_MUTANTS)
def test_param_grads_mutant_fails(mutant):
    with pytest.raises(AssertionError):
        _pg_case(37, 252, 1e-6, mutant)


# ------------------------------------------------------------------------------------------------------- low-rank adaptor
def lowrank_case_inputs(M, D, R, seed):
    """x, A, Bm, dy with a gradient that cancels over the rows: rows come in (g, -g (1 + 2^-10)) pairs."""
    x = fb.rnd(M, D, seed=seed)
    A, Bm = fb.rnd(R, D, seed=seed + 1) * 0.05, fb.rnd(D, R, seed=seed + 2) * 0.05
    dy = fb.rnd(M, D, seed=seed + 3)
    dy[1::2] = -dy[::2][:M // 2] * (1 + 2 ** -10)
    return x, A, Bm, dy


def emu_lowrank(x, A, Bm, dy, mutant=None):
    M, D = x.shape
    R = A.shape[0]
    t = torch.cat([emu_strided_sum(x * A[r]) for r in range(R)], 1)
    y = x.clone()
    for r in range(R):
        y = y + t[:, r:r + 1] * Bm[:, r]
    dt = torch.cat([emu_strided_sum(dy * Bm[:, r]) for r in range(R)], 1)
    dx = torch.zeros_like(dy) if mutant == "dx_without_dy" else dy.clone()
    for r in range(R):
        dx = dx + dt[:, r:r + 1] * A[r]
    rows_per = -(-M // 16)
    dA, dB = torch.zeros(R, D), torch.zeros(D, R)
    Dk = D - D % 64 if mutant == "ragged_columns_dropped" else D
    for c in range(16):
        if mutant == "last_chunk_dropped" and c == (M - 1) // rows_per:      # the last chunk that holds rows
            continue
        pa, pb = [torch.zeros(R, D) for _ in range(4)], [torch.zeros(D, R) for _ in range(4)]
        for m in range(c * rows_per, min(M, (c + 1) * rows_per)):
            ty = (m - c * rows_per) % 4
            pa[ty] = pa[ty] + dt[m][:, None] * x[m][None]
            pb[ty] = pb[ty] + dy[m][:, None] * t[m][None]
        dA = dA + (((pa[0] + pa[1]) + pa[2]) + pa[3])
        dB = dB + (((pb[0] + pb[1]) + pb[2]) + pb[3])
    dA[:, Dk:], dB[Dk:] = 0, 0
    return t, y, dx, dA, dB


LR_MUTANTS = ["dx_without_dy", "ragged_columns_dropped", "last_chunk_dropped"]


def _lowrank_case(M, D, R, mutant):
    x, A, Bm, dy = lowrank_case_inputs(M, D, R, seed=91)
    t, y, dx, dA, dB = emu_lowrank(x, A, Bm, dy, mutant)
    r = fb.lowrank_ref_bound(x, A, Bm, dy, t_in=t)
    return [fb.assert_within(got, r[k], r[k + "_bound"], "lowrank " + k)
            for k, got in (("t", t), ("y", y), ("dx", dx), ("dA", dA), ("dB", dB))]


@pytest.mark.parametrize("M,D,R", [(37, 300, 4), (1, 68, 2), (130, 1408, 4)])
def test_lowrank_emulation_is_within_the_bound(M, D, R):
    assert max(_lowrank_case(M, D, R, None)) > 1e-3


@pytest.mark.parametrize("mutant", LR_MUTANTS)
def test_lowrank_mutant_fails(mutant):
    with pytest.raises(AssertionError):
        _lowrank_case(37, 300, 4, mutant)


def test_attention_case_rope_ambiguity_stays_rare():
    q = fb.rnd(2, 2, 150, 64, seed=11).to(BF16)
    pos = torch.arange(150)[None] + 5 * torch.arange(2)[:, None]
    cos, sin = fb.rope_tables(64)
    fb.assert_rope_exempt_share(fb.rope_bf16(q.float(), pos, cos, sin)[1], "q")


# ------------------------------------------------------------------------------------------------------------- conv stack
def _raises(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def emu_im2col(x, kh, kw, pad, Kpad, bias_col, mutant=None):
    """im2col_kernel's index arithmetic on a poisoned output: item (m, 4-column group), k -> (tap, c) -> (ky, kx) -> (iy, ix)."""
    B, H, W, C = x.shape
    OH, OW = fb.conv_out_hw(H, W, kh, kw, pad)
    K, M = kh * kw * C, B * OH * OW
    col = fb.poisoned((M, Kpad), BF16, "cpu")
    groups = Kpad // 4 - (1 if mutant == "last_group_unwritten" else 0)
    m, k = torch.arange(M)[:, None], torch.arange(groups * 4)[None]
    ox, oy, b = m % OW, (m // OW) % OH, m // (OW * OH)
    tap = k // C
    c = k - tap * C
    ky, kx = tap // kw, tap - (tap // kw) * kw
    if mutant == "kxky_swapped":
        ky, kx = kx, ky
    iy, ix = oy + ky - pad, ox + kx - pad
    if mutant == "pad_ignored_at_top":
        iy = iy.clamp_min(0)
    ok = (k < K) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    flat = ((b * H + iy.clamp(0, H - 1)) * W + ix.clamp(0, W - 1)) * C + c
    val = torch.where(ok, x.reshape(-1)[flat.clamp(0, x.numel() - 1)], torch.zeros((), dtype=BF16))
    ones_at = K - 1 if mutant == "ones_at_K_minus_1" else K
    if bias_col or mutant == "ones_without_bias_col":
        val = torch.where(k == ones_at, torch.ones((), dtype=BF16), val)
    col[:, :groups * 4] = val
    return col


IM2COL_CPU_CASES = [(2, 6, 10, 8, 3, 3, 1), (1, 8, 8, 1, 3, 3, 1), (2, 7, 7, 16, 5, 5, 0), (1, 2, 2, 4, 3, 3, 1), (1, 5, 5, 64, 5, 5, 0)]
IM2COL_MUTANTS = ["pad_ignored_at_top", "kxky_swapped", "ones_at_K_minus_1", "ones_without_bias_col", "last_group_unwritten"]


def _im2col_case(B, H, W, C, kh, kw, pad, bias_col, mutant=None):
    x = fb.rnd(B, H, W, C, seed=31).to(BF16)
    K = kh * kw * C
    Kpad = (K + 64) // 64 * 64                        # a padded row in both forms, as a caller with K % 64 != 0 would get
    got = emu_im2col(x, kh, kw, pad, Kpad, bias_col, mutant)
    ref = fb.im2col_ref(x, kh, kw, pad, Kpad, bias_col)
    assert torch.equal(got, ref), "im2col differs"
    assert bool((ref[:, K + 1:] == 0).all()) and bool((ref[:, K] == (1.0 if bias_col else 0.0)).all())


@pytest.mark.parametrize("case", IM2COL_CPU_CASES)
@pytest.mark.parametrize("bias_col", [True, False])
def test_im2col_emulation_equals_the_gather(case, bias_col):
    _im2col_case(*case, bias_col)


@pytest.mark.parametrize("mutant", IM2COL_MUTANTS)
def test_im2col_mutant_fails(mutant):
    # the non-square 3x3 case; (kx, ky) swapped needs a non-symmetric image, the ones column the form without a bias column
    _raises(_im2col_case, 2, 6, 10, 8, 3, 3, 1, mutant != "ones_without_bias_col", mutant)


def test_im2col_reference_is_not_unfold_order():
    """F.unfold's columns are channel-major (c, ky, kx); the kernel's are (ky, kx, c): the reference must be the latter."""
    x = fb.rnd(1, 4, 4, 3, seed=32).to(BF16)
    ref = fb.im2col_ref(x, 3, 3, 1, 28, False)[:, :27].float()
    unf = torch.nn.functional.unfold(x.float().permute(0, 3, 1, 2), 3, padding=1)[0].T
    assert not torch.equal(ref, unf)
    assert torch.equal(ref.view(16, 9, 3).permute(0, 2, 1).reshape(16, 27), unf)


def emu_col2im(dcol, B, H, W, C, kh, kw, pad, mutant=None):
    """col2im_kernel: the gather form, taps added serially in fp32 in (ky, kx) order onto 0."""
    OH, OW = fb.conv_out_hw(H, W, kh, kw, pad)
    ld = dcol.shape[1]
    K = kh * kw * C
    it = torch.arange(B * H * W * C)
    c, p = it % C, it // C
    ix, iy, b = p % W, (p // W) % H, p // (W * H)
    s = torch.zeros(it.numel(), dtype=F32)
    flat = dcol.reshape(-1)
    for ky in range(kh):
        for kx in range(kw):
            oy, ox = iy + pad - ky, ix + pad - kx
            if mutant == "correlation":
                oy, ox = iy - pad + ky, ix - pad + kx
            elif mutant == "ox_plus_pad_plus_kx":
                ox = ix + pad + kx
            ok = (oy >= 0) & (oy < OH) & (ox >= 0) & (ox < OW)
            if mutant == "corner_tap_dropped" and (ky, kx) == (kh - 1, kw - 1):
                ok = ok & ~((iy == H - 1) & (ix == W - 1))
            kcol = (ky * kw + kx) * C + c
            if mutant == "bias_column_as_tap" and (ky, kx) == (kh - 1, kw - 1):
                kcol = torch.where(c == C - 1, torch.full_like(kcol, K), kcol)
            idx = ((b * OH + oy.clamp(0, OH - 1)) * OW + ox.clamp(0, OW - 1)) * ld + kcol
            s = s + torch.where(ok, flat[idx].float(), torch.zeros(()))
    return s.view(B, H, W, C)


COL2IM_MUTANTS = ["correlation", "ox_plus_pad_plus_kx", "corner_tap_dropped", "bias_column_as_tap"]


def _col2im_case(B, H, W, C, kh, kw, pad, mutant=None):
    d = fb.col2im_input(B, H, W, C, kh, kw, pad, seed=33)
    ref, bound = fb.col2im_ref_bound(d, B, H, W, C, kh, kw, pad)
    return fb.assert_within(emu_col2im(d, B, H, W, C, kh, kw, pad, mutant), ref, bound, "col2im")


@pytest.mark.parametrize("case", IM2COL_CPU_CASES)
def test_col2im_emulation_is_within_the_bound(case):
    assert _col2im_case(*case) <= 0.5        # often 0: a few bf16 values of like size add exactly in fp32


@pytest.mark.parametrize("mutant", COL2IM_MUTANTS)
@pytest.mark.parametrize("case", [(2, 6, 10, 8, 3, 3, 1), (2, 7, 7, 16, 5, 5, 0)])
def test_col2im_mutant_fails(case, mutant):
    _raises(_col2im_case, *case, mutant)


def emu_relu_pool(dp, y2d, B, H, W, C, cpad, mutant=None):
    """relu_pool_fwd / _bwd kernels on y2d [M, >= C] (fp32 or bf16): fmaxf from the 0 floor; strict > scan from the first cell,
    gradient iff the maximum is > 0; the wrapper's dy buffer is zero-filled when it has pad columns, else the kernel owns all of it."""
    w = fb.pool_windows(y2d.float(), B, H, W, C)
    if mutant == "y_rounded_to_bf16":
        w = w.to(BF16).float()
    m = torch.zeros(w.shape[:-1])
    for e in range(4):
        m = torch.maximum(m, w[..., e])
    p = m.to(BF16)
    best, arg = w[..., 0].clone(), torch.zeros(w.shape[:-1], dtype=torch.long)
    for e in range(1, 4):
        take = w[..., e] >= best if mutant == "last_maximum_wins" else w[..., e] > best
        best, arg = torch.where(take, w[..., e], best), torch.where(take, torch.full_like(arg, e), arg)
    live = best >= 0 if mutant == "gradient_at_zero" else best > 0
    g = torch.where(live, dp.reshape(best.shape), torch.zeros(())).to(BF16)
    d4 = torch.zeros(w.shape, dtype=BF16).scatter_(-1, arg[..., None], g[..., None])
    full = fb.poisoned((B * H * W, cpad), BF16, "cpu")
    if cpad != C and mutant != "pad_columns_unwritten":
        full.zero_()
    full[:, :C] = d4.reshape(B, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B * H * W, C)
    return p, full


POOL_MUTANTS = ["last_maximum_wins", "gradient_at_zero", "y_rounded_to_bf16", "pad_columns_unwritten"]


def _pool_case(dtype, C, cpad, mutant=None):
    B, H, W = 2, 4, 6
    y = fb.pool_edge_windows(B, H, W, C, seed=34, dtype=dtype)
    wide = fb.rnd(B * H * W, C + 8, seed=35).to(dtype)                  # y as a column window of a wider buffer
    wide[:, :C] = y
    dp = fb.rnd(B, H // 2, W // 2, C, seed=36) + 3.0                    # no zero gradients: a wrong route or gate always shows
    p, dy = emu_relu_pool(dp, wide[:, :C], B, H, W, C, cpad, mutant)
    assert torch.equal(p, fb.relu_pool_fwd_ref(y, B, H, W, C)), "relu_pool_fwd differs"
    assert torch.equal(dy, fb.relu_pool_bwd_ref(dp, y, B, H, W, C, cpad)), "relu_pool_bwd differs"


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C,cpad", [(4, 4), (4, 64), (16, 64), (64, 64)])
def test_relu_pool_emulation_equals_the_reference(dtype, C, cpad):
    _pool_case(dtype, C, cpad)


@pytest.mark.parametrize("mutant", POOL_MUTANTS)
def test_relu_pool_mutant_fails(mutant):
    _raises(_pool_case, F32, 4, 64, mutant)


def test_pool_edge_windows_hold_every_constructed_case():
    for dtype in (F32, BF16):
        w = fb.pool_windows(fb.pool_edge_windows(2, 4, 6, 4, seed=34, dtype=dtype).float(), 2, 4, 6, 4).reshape(-1, 4)
        top = w.amax(1, keepdim=True)
        ties = (w == top).sum(1)
        assert bool((ties == 4).any()) and bool((top[:, 0] < 0).any())
        for a, b in [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]:
            assert bool(((ties == 2) & (w[:, a] == top[:, 0]) & (w[:, b] == top[:, 0]) & (top[:, 0] > 0)).any()), (a, b)
        zero = (top[:, 0] == 0)
        neg0 = zero & torch.signbit(w).any(1) & ~(w == 0).logical_and(~torch.signbit(w)).any(1)
        assert bool((zero & ~neg0).any()) and bool(neg0.any())
        if dtype == F32:
            second = w.topk(2, 1).values[:, 1:2]
            assert bool(((top > second) & (top.to(BF16) == second.to(BF16)) & (top > 0)).any())


def emu_conv_pack(Wm, bias, Kpad, mutant=None):
    """conv_pack_kernel: 8-element chunks; two float4 loads where K % 4 == 0 and the chunk lies inside the row, else the scalar
    form, which also places the bias and the zeros."""
    Cout, K = Wm.shape
    out = fb.poisoned((Cout, Kpad), BF16, "cpu")
    vec = K % 4 == 0
    for k0 in range(0, Kpad, 8):
        v = torch.zeros(Cout, 8)
        if vec and k0 + 8 <= K:
            v = Wm[:, k0:k0 + 8].clone()
        else:
            for e in range(8):
                k = k0 + e
                if k < K:
                    v[:, e] = Wm[:, k]
                elif k == K and bias is not None and not (mutant == "bias_lost_in_tail_chunk" and vec and k0 < K):
                    v[:, e] = bias
        if mutant == "truncation":
            out[:, k0:k0 + 8] = (v.view(torch.int32) & -65536).view(F32).to(BF16)
        else:
            out[:, k0:k0 + 8] = v.to(BF16)
    return out


def _pack_case(K, Cout, with_bias, mutant=None):
    Wm, bias = fb.rnd(Cout, K, seed=37), (fb.rnd(Cout, seed=38) + 2.0 if with_bias else None)
    Kpad = (K + 64) // 64 * 64
    assert torch.equal(emu_conv_pack(Wm, bias, Kpad, mutant), fb.conv_pack_ref(Wm, bias, Kpad)), "conv_pack differs"


@pytest.mark.parametrize("K", [9, 36, 63, 64, 144])
@pytest.mark.parametrize("with_bias", [True, False])
def test_conv_pack_emulation_equals_the_reference(K, with_bias):
    _pack_case(K, 5, with_bias)


def test_conv_pack_mutants_fail():
    _raises(_pack_case, 36, 5, True, "bias_lost_in_tail_chunk")            # K % 4 == 0, K % 8 != 0: the bias sits in the tail chunk
    _pack_case(64, 5, True, "bias_lost_in_tail_chunk")                      # ... and only there: at K % 8 == 0 the mutant is the kernel
    _raises(_pack_case, 36, 5, True, "truncation")


def test_conv_unpack_reference_and_a_bias_read_one_column_early():
    for K in (9, 36):
        dWp = fb.rnd(5, 64, seed=39)
        for col, ok in ((K, True), (K - 1, False)):
            dW, db = fb.poisoned((5, K), F32, "cpu"), fb.poisoned((5,), F32, "cpu")
            dW.copy_(dWp[:, :K]), db.copy_(dWp[:, col])
            assert torch.equal(dW, dWp[:, :K]) and torch.equal(db, dWp[:, K]) == ok


@pytest.mark.parametrize("case", fb.CHAIN_CASES)
def test_stem_chain_reference_is_consistent_and_decisions_are_rare(case):
    """The chain test's fp64 pieces are the autograd's (the wgrad GEMM of the routed dy is conv2d's weight gradient, its bias
    column the bias gradient, the fold of the dgrad GEMM the input gradient), and the windows whose routing is a decision are at
    most 1 % -- from the fp64 reference and the bf16-rounded operands alone."""
    r = fb.stem_chain_ref(*fb.stem_chain_case(*case), wgrad_splits=8)
    K = r["K"]
    share = float(r["decisions"].double().mean())
    assert share <= 0.01, f"{share:.3%} of the windows are decisions"
    assert float((r["dp_used"] != 0).double().mean()) > 0.98
    for a, b in ((r["y"], r["y_gemm"]), (r["dwp"][:, :K], r["dW"]), (r["dwp"][:, K], r["db"]), (r["dx_fold"], r["dx"])):
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    assert bool((r["dwp"][:, K + 1:] == 0).all())


def test_pool_decisions_flags_close_runner_ups_and_maxima_near_zero():
    y = torch.tensor([[1.0], [1.0 - 1e-7], [0.2], [0.1],     # window 0 (H = W = 2, C = 1): runner-up within the bounds
                      [1.0], [0.5], [0.2], [0.1],            # 1: clear
                      [1e-8], [-1.0], [-2.0], [-3.0],        # 2: maximum within its bound of 0
                      [-1.0], [-1.0], [-2.0], [-3.0]]).double()   # 3: a tie below zero -- no gradient either way, but flagged
    y = y.reshape(4, 2, 2, 1).reshape(16, 1)
    dec = fb.pool_decisions(y, torch.full_like(y, 6e-8), 4, 2, 2, 1)
    assert dec.reshape(-1).tolist() == [True, False, True, True]


# ---------------------------------------------------------------------------------------------------------------- map heads
def emu_pair_logits(p, text, rpb, scale, mutant=None):
    """pair_logits_kernel: lane l adds the products of its float4 chunks (columns 4 l + 256 j) serially, a 64-lane butterfly, then
    scale / sqrtf(nn) and one product."""
    rows, C = p.shape
    tidx = torch.arange(rows) // (rpb + 1 if mutant == "pair_index_off" else rpb)
    t = text[tidx.clamp(max=text.shape[0] - 1)]
    J = -(-C // 256)
    if mutant == "last_float4_dropped" and C % 256:
        J -= 1

    def lanes(a, b):
        prod = torch.zeros(rows, J * 256 if J else 256)
        n = min(C, J * 256)
        prod[:, :n] = (a * b)[:, :n]
        prod = prod.view(rows, max(J, 1), 64, 4)
        s = torch.zeros(rows, 64)
        for j in range(max(J, 1)):
            for e in range(4):
                s = s + prod[:, j, :, e]
        lane = torch.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lane ^ o]
        return s[:, 0]

    d0, d1 = lanes(p, t[:, 0]), lanes(p, t[:, 1])
    nn = lanes(t[:, 0], t[:, 0]) if mutant == "norm_of_text" else lanes(p, p)
    inv = torch.tensor(scale, dtype=F32) / torch.sqrt(nn)
    return torch.stack([d0 * inv, d1 * inv], 1)


PAIR_MUTANTS = ["pair_index_off", "last_float4_dropped", "norm_of_text"]


def _pair_case(rows, C, rpb, mutant=None):
    p, text = fb.pair_inputs(rows, C, rpb, seed=41)
    ref, bound = fb.pair_logits_ref_bound(p, text, rpb, 100.0)
    return fb.assert_within(emu_pair_logits(p, text, rpb, 100.0, mutant), ref, bound, "pair_logits")


@pytest.mark.parametrize("rows,C,rpb", [(7, 4, 1), (9, 252, 3), (13, 772, 3), (5, 1024, 257)])
def test_pair_logits_emulation_is_within_the_bound(rows, C, rpb):
    assert 1e-3 < _pair_case(rows, C, rpb) <= 0.5


@pytest.mark.parametrize("mutant", PAIR_MUTANTS)
def test_pair_logits_mutant_fails(mutant):
    _raises(_pair_case, 13, 772, 3, mutant)


def emu_bilinear(x, H, W, one_minus=False, mutant=None, quotient=True):
    """bilinear_ac_kernel in fp32: position fl(o (n_in - 1) / (n_out - 1)), one division of exact integers (quotient=False:
    zs_accumulate_kernel's o * fl((n_in - 1) / (n_out - 1))), truncated and clamped to the last cell."""
    B, h, w = x.shape
    if mutant == "h_w_swapped":
        x = x.reshape(B, w, h)
        h, w = w, h

    def axis(n_in, n_out):
        o = torch.arange(n_out, dtype=F32)
        if mutant == "align_corners_false":
            f = ((o + 0.5) * torch.tensor(n_in / n_out, dtype=F32) - 0.5).clamp_min(0.0)
        else:
            step = torch.tensor(float(n_in - 1), dtype=F32) / torch.tensor(float(n_out - 1), dtype=F32) if n_out > 1 else torch.zeros(())
            f = (o * float(n_in - 1)) / torch.tensor(float(max(n_out - 1, 1)), dtype=F32) if quotient else o * step
        i0 = f.to(torch.int32).long()
        i0 = torch.where(i0 < n_in - 1, i0, torch.full_like(i0, n_in - 2 if n_in > 1 else 0))
        return i0, i0 + (1 if n_in > 1 else 0), f - i0.float()

    y0, y1, wy = axis(h, H)
    x0, x1, wx = axis(w, W)
    wy, wx = wy[None, :, None], wx[None, None, :]
    g = lambda yi, xi: x[:, yi][:, :, xi]
    v = (1 - wy) * ((1 - wx) * g(y0, x0) + wx * g(y0, x1)) + wy * ((1 - wx) * g(y1, x0) + wx * g(y1, x1))
    return 1 - v if one_minus else v


BILINEAR_CASES = [(5, 9, 33, 20), (16, 16, 224, 224), (16, 16, 7, 7), (1, 1, 7, 7), (2, 2, 3, 3), (7, 7, 7, 7), (5, 9, 1, 20), (5, 9, 33, 1)]


def _bilinear_case(h, w, H, W, one_minus, mutant=None):
    x = fb.rnd(2, h, w, seed=42)
    ref, bound = fb.bilinear_ref_bound(x, H, W, one_minus)
    return fb.assert_within(emu_bilinear(x, H, W, one_minus, mutant), ref, bound, "bilinear_ac")


@pytest.mark.parametrize("case", BILINEAR_CASES)
@pytest.mark.parametrize("one_minus", [False, True])
def test_bilinear_emulation_is_within_the_bound(case, one_minus):
    assert _bilinear_case(*case, one_minus) <= 0.5


@pytest.mark.parametrize("mutant", ["align_corners_false", "h_w_swapped"])
def test_bilinear_mutant_fails(mutant):
    _raises(_bilinear_case, 5, 9, 33, 20, False, mutant)


def test_bilinear_reference_is_torch_interpolate_in_fp64():
    x = fb.rnd(2, 5, 9, seed=43)
    ref, _ = fb.bilinear_ref_bound(x, 33, 20)
    it = torch.nn.functional.interpolate(x.double()[:, None], size=(33, 20), mode="bilinear", align_corners=True)[:, 0]
    assert float((ref - it).abs().max()) < 1e-13


def emu_zs(logits, mask, amap, w, mutant=None):
    B, h, S = mask.shape[0], mask.shape[-1], amap.shape[-1]
    d = (logits[..., 1] - logits[..., 0]).reshape(B, h, h)
    sig = lambda v: 1.0 / (1.0 + torch.exp(-v))
    wt = torch.tensor(w, dtype=F32)
    geo = "align_corners_false" if mutant == "align_corners_false" else None
    si = (emu_bilinear(sig(d), S, S, quotient=False) if mutant == "softmax_before_interpolation"
          else sig(emu_bilinear(d, S, S, mutant=geo, quotient=False)))
    if mutant == "overwrite":
        return wt * sig(d), wt * si
    return mask + wt * sig(d), amap + wt * si


ZS_CASES = [(16, 224), (16, 16), (1, 7), (2, 3), (7, 224)]
ZS_MUTANTS = ["align_corners_false", "softmax_before_interpolation", "overwrite"]


def _zs_case(h, S, mutant=None):
    lg, mask, amap = fb.zs_inputs(2, h, S, seed=44)
    rm, em, ra, ea = fb.zs_accumulate_ref_bound(lg, mask, amap, 0.37)
    gm, ga = emu_zs(lg, mask, amap, 0.37, mutant)
    return max(fb.assert_within(gm, rm, em, "zs mask"), fb.assert_within(ga, ra, ea, "zs map"))


@pytest.mark.parametrize("h,S", ZS_CASES)
def test_zs_accumulate_emulation_is_within_the_bound(h, S):
    assert (1e-3 if h > 1 else 0.0) <= _zs_case(h, S) <= 1.0     # h = 1: its one difference is -60, sigmoid ~ 1e-26 onto O(1)


@pytest.mark.parametrize("mutant", ZS_MUTANTS)
def test_zs_accumulate_mutant_fails(mutant):
    _raises(_zs_case, 7, 224, mutant)


def emu_rowmax(s, acc, period, w, mutant=None):
    rows, cols = s.shape
    c = torch.arange(cols)
    keep = (c % period != 0) if period > 0 else torch.ones(cols, dtype=torch.bool)
    if mutant == "column_0_kept":
        keep[0] = True
    if mutant == "only_first_64":
        keep = keep & (c < 64)
    m = s.masked_fill(~keep[None], float("-inf")).amax(1) if cols else torch.full((rows,), float("-inf"))
    return acc + torch.tensor(w, dtype=F32) * m


def _rowmax_case(rows, cols, period, mutant=None):
    full, acc = fb.rowmax_inputs(rows, cols, cols + 8, seed=45)
    ref, bound = fb.rowmax_skip_ref_bound(full[:, :cols], acc, period, 0.61)
    return fb.rowmax_check(emu_rowmax(full[:, :cols], acc, period, 0.61, mutant), ref, bound)


@pytest.mark.parametrize("cols", [1, 63, 64, 65, 514])
@pytest.mark.parametrize("period", [0, 257, 5])
def test_rowmax_emulation_is_within_the_bound(cols, period):
    _rowmax_case(7, cols, period)          # an accumulate form: the bound is its two roundings and nothing else


@pytest.mark.parametrize("mutant", ["column_0_kept", "only_first_64"])
def test_rowmax_mutant_fails(mutant):
    _raises(_rowmax_case, 7, 514, 257, mutant)


# ------------------------------------------------------------------------------------------------------------------- LoRA
LORA_SEED = 0x7A5C3E1F90B2D486            # 63 bits, high bits set
LORA_S = 2.0


def _fma(a, b, c):
    """One fp32 rounding of a * b + c (the product of two fp32 values is exact in fp64)."""
    return (torch.as_tensor(a).double() * b.double() + c.double()).float()


def _ik32(p):
    one = torch.tensor(1.0, dtype=F32)
    return one / (one - torch.tensor(p, dtype=F32))


def _lora_masks(M, D, p, seed=LORA_SEED):
    return fb.keep_mask_ref(seed, M, D, p), fb.keep_mask_ref(seed, M, D, p, second=True)


def emu_lora_down(x, A, out, s, p, kq, kv, R2, mutant=None):
    """lora_down_kernel's arithmetic: a workgroup per (16 rows, group); wave w of 8 owns ceil(steps/8) 32-element k-steps of the
    group's range and adds one 32-product block per step to its fp32 accumulator (dropped elements zeroed, A rounded to bf16); the
    8 wave sums are added in order, scaled by s ik and rounded to bf16.  out: a [>= M, >= 64] window of a poisoned buffer."""
    M, D = x.shape
    r, G = R2 // 2, fb.lora_groups(D, R2)
    a = A.to(BF16).float()
    xf = x.float()
    xq = torch.where(kq > 0, xf, torch.zeros_like(xf))
    xv = xq if mutant == "v_rows_use_q_mask" else torch.where(kv > 0, xf, torch.zeros_like(xf))
    scale = torch.tensor(s, dtype=F32) * _ik32(p) if (p > 0 and mutant != "scale_without_ik") else torch.tensor(s, dtype=F32)
    steps = D // 32 // G
    per = -(-steps // 8)

    def block(st):
        c = slice(st * 32, st * 32 + 32)
        return torch.cat([xq[:, c] @ a[:r, c].T, xv[:, c] @ a[r:, c].T], 1)

    for g in range(G):
        tot = torch.zeros(M, R2, dtype=F32)
        for w in range(8):
            s0 = g * steps + w * per
            s1 = min(s0 + per, g * steps + steps)
            acc = torch.zeros(M, R2, dtype=F32)
            for st in range(s0, s1):
                acc = acc + block(st)
            if mutant == "tail_step_counted" and s1 > s0:              # the UN = 4 tail re-reads the last step: not zeroed
                for _ in range(-(s1 - s0) % 4):
                    acc = acc + block(s1 - 1)
            tot = tot + acc
        val = (scale * tot).to(BF16)
        col = 0 if mutant == "group_into_group_0" else g * R2
        out[:M, col:col + R2] = val
        if mutant == "row_clamp_written":                              # rows >= M of the last 16-row block store row M - 1
            out[M:min(out.shape[0], -(-M // 16) * 16), col:col + R2] = val[M - 1]


LORA_DOWN_CPU_CASES = [(5, 64, 16, 0.0), (17, 96, 32, 0.25), (33, 1152, 16, 0.25), (3, 5120, 16, 0.25), (16, 2048, 32, 0.0)]
LORA_DOWN_MUTANTS = ["tail_step_counted", "v_rows_use_q_mask", "row_clamp_written", "group_into_group_0", "scale_without_ik"]


def _lora_down_case(M, D, R2, p, mutant=None):
    x = fb.lora_rows(M, D, seed=11).to(BF16)
    A = fb.lora_adaptor(R2, D, seed=12)
    kq, kv = _lora_masks(M, D, p)
    G = fb.lora_groups(D, R2)
    buf = fb.poisoned((M + 3, 64 + 8), BF16, "cpu")
    emu_lora_down(x, A, buf, LORA_S, p, kq, kv, R2, mutant)
    r = fb.lora_down_ref_bound(x, A, LORA_S, p, kq, kv, R2, G)
    ratio = fb.assert_within(buf[:M, :G * R2], r["part"], r["part_bound"], f"lora_down {M}x{D} R2={R2}")
    fb.assert_within(buf[:M, :G * R2].double().reshape(M, G, R2).sum(1), r["total"], r["total_bound"], "lora_down sum of groups")
    fb.assert_untouched(buf[M:], "rows past M")
    fb.assert_untouched(buf[:M, G * R2:], "groups past G")
    return ratio


@pytest.mark.parametrize("case", LORA_DOWN_CPU_CASES)
def test_lora_down_emulation_is_within_the_bound(case):
    assert _lora_down_case(*case) > 1e-3


@pytest.mark.parametrize("mutant", LORA_DOWN_MUTANTS)
def test_lora_down_mutant_fails(mutant):
    with pytest.raises(AssertionError):
        _lora_down_case(33, 1152, 16, 0.25, mutant)


def emu_lora_dx(base, g, A, out, s, p, kq, kv, mutant=None):
    """lora_dx_kernel: r serial FMAs per half against bf16(A), then fma(s, fma(acc_q, kq, acc_v * kv), base)."""
    M, D = base.shape
    r = A.shape[0] // 2
    a = A if mutant == "A_not_rounded" else A.to(BF16).float()
    acc, accv = torch.zeros(M, D, dtype=F32), torch.zeros(M, D, dtype=F32)
    for j in range(r):
        acc = _fma(g[:, j:j + 1], a[j][None], acc)
        if mutant != "v_half_dropped":
            accv = _fma(g[:, r + j:r + j + 1], a[r + j][None], accv)
    inner = _fma(acc, kq, accv * kv)
    b = base * (kq > 0) if mutant == "mask_on_base" else base
    o = _fma(torch.tensor(s, dtype=F32), inner, b)
    w = D - 4 if mutant == "last_float4_dropped" else D
    out[:, :w] = o[:, :w]


LORA_DX_MUTANTS = ["A_not_rounded", "mask_on_base", "v_half_dropped", "last_float4_dropped"]


def _lora_dx_case(M, D, R2, p, mutant=None):
    ext = fb.lora_rows(M, D + R2, seed=21)
    base, g = ext[:, :D].contiguous(), ext[:, D:].contiguous()
    A = fb.lora_adaptor(R2, D, seed=22)
    kq, kv = _lora_masks(M, D, p)
    buf = fb.poisoned((M + 1, D), F32, "cpu")
    emu_lora_dx(base, g, A, buf[:M], LORA_S, p, kq, kv, mutant)
    ref, bnd = fb.lora_dx_ref_bound(base, g, A, LORA_S, p, kq, kv)
    ratio = fb.assert_within(buf[:M], ref, bnd, f"lora_dx {M}x{D} R2={R2}")
    fb.assert_untouched(buf[M:], "row past M")
    return ratio


@pytest.mark.parametrize("case", [(1, 4, 16, 0.25), (7, 68, 16, 0.0), (9, 132, 32, 0.25)])
def test_lora_dx_emulation_is_within_the_bound(case):
    assert _lora_dx_case(*case) > 1e-3


@pytest.mark.parametrize("mutant", LORA_DX_MUTANTS)
def test_lora_dx_mutant_fails(mutant):
    with pytest.raises(AssertionError):
        _lora_dx_case(9, 132, 32, 0.25, mutant)


def emu_lora_wgrad(x, kq, kv, sg_in, border, dq, dv, s, p, R2, mfma, mutant=None):
    """(dA [R2, D], dBq [D, r], dBv [D, r]) as mh_lora_wgrad forms them.  Thread-per-column kernel: 64 row chunks, a chunk's rows
    added serially in fp32, the chunks added in order.  MFMA kernel (R2 = 16): 16 row chunks, per 32-row step two products per
    sum -- the per-row scalars' bf16 heads, then their bf16 remainders -- against x with its dropped elements zeroed; 1 / (1 - p)
    multiplies the chunk's finished sum."""
    M, D = x.shape
    r = R2 // 2
    grp = border.float().reshape(M, 64 // R2, R2)
    st = torch.zeros(M, R2, dtype=F32)
    for g in range(1 if mutant == "border_group_0_only" else 64 // R2):
        st = st + grp[:, g]
    sg = torch.tensor(s, dtype=F32) * sg_in
    xf, qf, vf = x.float(), dq.float(), dv.float()
    ik = _ik32(p) if (p > 0 and mutant != "ik_missing") else torch.tensor(1.0, dtype=F32)
    nch = 16 if mfma else 64
    rows_per = -(-M // nch)
    chunks = [(c * rows_per, min(c * rows_per + rows_per, M)) for c in range(nch)]
    live = [c for c, (m0, m1) in enumerate(chunks) if m1 > m0]
    parts = []
    for c, (m0, m1) in enumerate(chunks):
        a, bq, bv = torch.zeros(R2, D, dtype=F32), torch.zeros(D, r, dtype=F32), torch.zeros(D, r, dtype=F32)
        if mutant == "last_chunk_dropped" and c == live[-1]:
            m1 = m0
        if mfma:
            xq = torch.where(kq > 0, xf, torch.zeros_like(xf))
            xv = torch.where(kv > 0, xf, torch.zeros_like(xf))
            gh, th = fb.bf16_round(sg), fb.bf16_round(st)
            gl, tl = fb.bf16_round(sg - gh), fb.bf16_round(st - th)
            if mutant == "remainder_dropped":
                gl, tl = torch.zeros_like(gl), torch.zeros_like(tl)
            for mb in range(m0, m1, 32):
                rs = slice(mb, min(mb + 32, m1))
                for sc_g, sc_t in ((gh, th), (gl, tl)):
                    a[:r] = a[:r] + sc_g[rs, :r].T @ xq[rs]
                    a[r:] = a[r:] + sc_g[rs, r:].T @ xv[rs]
                    bq = bq + qf[rs].T @ sc_t[rs, :r]
                    bv = bv + vf[rs].T @ sc_t[rs, r:]
            a = a * ik
        else:
            rows = list(range(m0, m1))
            if mutant == "clamped_row_counted_twice" and rows:          # the trip of three's clamped loads are not skipped
                rows += [m1 - 1] * (-len(rows) % 3)
            for m in rows:
                xd, xw = xf[m] * (ik * (kq[m] > 0)), xf[m] * (ik * (kv[m] > 0))
                a[:r] = a[:r] + sg[m, :r, None] * xd[None]
                a[r:] = a[r:] + sg[m, r:, None] * xw[None]
                bq = bq + qf[m][:, None] * st[m, None, :r]
                bv = bv + vf[m][:, None] * st[m, None, r:]
        parts.append((a, bq, bv))
    out = [torch.zeros_like(t) for t in parts[0]]
    for pa in parts:
        out = [o + t for o, t in zip(out, pa)]
    return out


LORA_WGRAD_CPU_CASES = [(1, 128, 16, 1, 0.25), (37, 128, 16, 1, 0.0), (530, 128, 16, 1, 0.25), (37, 128, 16, 0, 0.25),
                        (71, 132, 16, 0, 0.25), (200, 68, 32, 0, 0.0)]
LORA_WGRAD_MUTANTS = [("last_chunk_dropped", 0), ("last_chunk_dropped", 1), ("clamped_row_counted_twice", 0), ("border_group_0_only", 0),
                      ("border_group_0_only", 1), ("remainder_dropped", 1), ("ik_missing", 0), ("ik_missing", 1)]


def _lora_wgrad_case(M, D, R2, mfma, p, mutant=None):
    r = R2 // 2
    x = fb.lora_rows(M, D, seed=31).to(BF16)
    sg_in = fb.rnd(M, R2, seed=32) * 0.1
    border = fb.rnd(M, 64, seed=33).to(BF16)
    dq, dv = fb.rnd(M, D, seed=34).to(BF16), fb.rnd(M, D, seed=35).to(BF16)
    kq, kv = _lora_masks(M, D, p)
    dA, dBq, dBv = emu_lora_wgrad(x, kq, kv, sg_in, border, dq, dv, LORA_S, p, R2, mfma, mutant)
    ref = fb.lora_wgrad_ref_bound(x, kq, kv, sg_in, border, dq, dv, LORA_S, R2, bool(mfma))
    what = f"lora_wgrad {M}x{D} R2={R2} mfma={mfma}"
    return max(fb.assert_within(dA[:r], ref["dA"][:r], ref["dA_bound"][:r], what + " dA_q"),
               fb.assert_within(dA[r:], ref["dA"][r:], ref["dA_bound"][r:], what + " dA_v"),
               fb.assert_within(dBq, ref["dBq"], ref["dBq_bound"], what + " dB_q"),
               fb.assert_within(dBv, ref["dBv"], ref["dBv_bound"], what + " dB_v"))


@pytest.mark.parametrize("case", LORA_WGRAD_CPU_CASES)
def test_lora_wgrad_emulation_is_within_the_bound(case):
    assert _lora_wgrad_case(*case) > 1e-3


@pytest.mark.parametrize("mutant,mfma", LORA_WGRAD_MUTANTS)
def test_lora_wgrad_mutant_fails(mutant, mfma):
    with pytest.raises(AssertionError):
        _lora_wgrad_case(71, 128, 16, mfma, 0.25, mutant)


def emu_lora_refresh(Bq, Bv, ext, extT, W, D, r, mutant=None):
    q, v = Bq.to(BF16), Bv.to(BF16)
    for g in range(1 if mutant == "one_group_only" else 64 // (2 * r)):
        c = D + g * 2 * r
        ext[:W, c:c + r] = q
        vc = c if mutant == "v_into_q_columns" else c + r
        ext[2 * W:3 * W, vc:vc + r] = v
        if extT is not None:
            extT[c:c + r, :W] = q.reshape(r, W) if mutant == "transpose_missing" else q.T
            extT[vc:vc + r, 2 * W:3 * W] = v.reshape(r, W) if mutant == "transpose_missing" else v.T


def _lora_refresh_case(W, D, r, mutant=None, with_T=True):
    Bq, Bv = fb.rnd(W, r, seed=41), fb.rnd(W, r, seed=42)
    ext = fb.poisoned((3 * W + 1, D + 64 + 8), BF16, "cpu")
    extT = fb.poisoned((D + 64 + 1, 3 * W + 8), BF16, "cpu") if with_T else None
    emu_lora_refresh(Bq, Bv, ext, extT, W, D, r, mutant)
    fb.lora_refresh_check(ext, extT, Bq, Bv, W, D, r)


@pytest.mark.parametrize("W,D,r", [(12, 32, 8), (100, 64, 16)])
@pytest.mark.parametrize("with_T", [True, False])
def test_lora_refresh_emulation_passes_the_check(W, D, r, with_T):
    _lora_refresh_case(W, D, r, with_T=with_T)


@pytest.mark.parametrize("mutant", ["v_into_q_columns", "one_group_only", "transpose_missing"])
def test_lora_refresh_mutant_fails(mutant):
    with pytest.raises(AssertionError):
        _lora_refresh_case(12, 32, 8, mutant)


def test_keep_mask_ref_is_a_deterministic_fair_draw_with_two_streams():
    n, p = 1 << 20, 0.25
    q = fb.keep_mask_ref(LORA_SEED, 1024, 1024, p)
    assert torch.equal(q, fb.keep_mask_ref(LORA_SEED, 1024, 1024, p))
    assert torch.equal(q.reshape(-1), fb.keep_mask_ref(LORA_SEED, 1, n, p).reshape(-1)), "the mask is a function of the flat index"
    v = fb.keep_mask_ref(LORA_SEED, 1024, 1024, p, second=True)
    assert torch.equal(v, fb.keep_mask_ref(LORA_SEED | fb.LORA_V_TAG, 1024, 1024, p)), "bit 63 of the seed selects the second draw"
    assert not torch.equal(q, v)
    both = float(((q > 0) & (v > 0)).double().mean())
    tol = 4 * (p * (1 - p) / n) ** 0.5
    for m in (q, v):
        assert set(m.unique().tolist()) == {0.0, float(_ik32(p))}
        assert abs(float((m > 0).double().mean()) - (1 - p)) <= tol
    assert abs(both - (1 - p) ** 2) <= 2 * tol, "the two draws are not independent"
    assert not torch.equal(q, fb.keep_mask_ref(LORA_SEED ^ 1, 1024, 1024, p))
    for second in (False, True):
        assert bool((fb.keep_mask_ref(LORA_SEED, 7, 36, 0.0, second=second) == 1.0).all())


def test_rmsnorm_bound_carries_an_error_of_dy_and_leaves_the_default_unchanged():
    x, w = fb.norm_rows(7, 252, seed=51), fb.norm_weight(252, seed=52)
    dy, dres = fb.rnd(7, 252, seed=53), fb.rnd(7, 252, seed=54)
    r0 = fb.rmsnorm_ref_bound(x, w, 1e-6, dy=dy, dres=dres)
    e = 1e-3 * dy.abs() + 1e-6
    r1 = fb.rmsnorm_ref_bound(x, w, 1e-6, dy=dy, dres=dres, dy_err=e)
    assert torch.equal(r0["dx"], r1["dx"]) and bool((r1["dx_bound"] >= r0["dx_bound"]).all())
    assert torch.equal(fb.rmsnorm_ref_bound(x, w, 1e-6, dy=dy, dres=dres, dy_err=torch.zeros_like(dy))["dx_bound"], r0["dx_bound"])
    # a dy moved by its whole allowance, with either sign per element, stays inside the widened bound around the original dx
    sign = torch.where(fb.rnd(7, 252, seed=55) > 0, 1.0, -1.0)
    moved = fb.rmsnorm_ref_bound(x, w, 1e-6, dy=dy.double() + sign * e.double(), dres=dres)["dx"]
    # (the allowance is attained exactly on an all-zero row: 1e-9 relative for the fp64 evaluation of the two sides)
    fb.assert_within(moved, r1["dx"], (r1["dx_bound"] - r0["dx_bound"]) * (1 + 1e-9) + 1e-300, "dy_err")


def test_layernorm_bound_carries_an_error_of_dy_and_leaves_the_default_unchanged():
    x, w = fb.norm_rows(7, 252, seed=56), fb.norm_weight(252, seed=57)
    dy, dres = fb.rnd(7, 252, seed=58), fb.rnd(7, 252, seed=59)
    r0 = fb.layernorm_ref_bound(x, w, None, 1e-12, dy=dy, dres=dres)
    e = 1e-3 * dy.abs() + 1e-6
    r1 = fb.layernorm_ref_bound(x, w, None, 1e-12, dy=dy, dres=dres, dy_err=e)
    assert torch.equal(r0["dx"], r1["dx"]) and bool((r1["dx_bound"] >= r0["dx_bound"]).all())
    assert torch.equal(fb.layernorm_ref_bound(x, w, None, 1e-12, dy=dy, dres=dres, dy_err=torch.zeros_like(dy))["dx_bound"],
                       r0["dx_bound"])
    # a dy moved by its whole allowance, with either sign per element, stays inside the widened bound around the original dx
    sign = torch.where(fb.rnd(7, 252, seed=60) > 0, 1.0, -1.0)
    moved = fb.layernorm_ref_bound(x, w, None, 1e-12, dy=dy.double() + sign * e.double(), dres=dres)["dx"]
    fb.assert_within(moved, r1["dx"], (r1["dx_bound"] - r0["dx_bound"]) * (1 + 1e-9) + 1e-300, "dy_err")


# -------------------------------------------------------------------------------------- Q-Former training: attention dropout
QF_SEED = 0x3C5A7E1F90B2D486              # 62 bits; | 1 << 63 takes the second draw


def _flat_keep(idx, p, seed=QF_SEED):
    """The keep factor at the flat mask indices idx (any shape, int64)."""
    return fb.keep_mask_ref(seed, 1, int(idx.max()) + 1, p).reshape(-1)[idx]


def _attn_mask_index(B, H, Sq, Sk, head=True, stride=None):
    b, h, i, j = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(Sq), torch.arange(Sk), indexing="ij")
    return ((b * H + (h if head else 0)) * Sq + i) * (Sk if stride is None else stride) + j


ATTN_DROP_MASK_MUTANTS = ["stride_rounded_to_64", "head_dropped", "transposed", "last_key_tile_unmasked", "last_query_rows_unmasked"]
ATTN_DROP_MUTANTS = ATTN_DROP_MASK_MUTANTS + ["rowsum_after_mask", "dq_unmasked", "dk_unmasked", "dv_unmasked", "delta_from_undropped_o",
                                              "one_element_flipped"]


def emu_attn_dropout(q, k, v, dout, scale, p, mutant=None):
    """The DROP instances of the tiled kernels (attn_fwd_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel) in fp32: online softmax
    over 64-key tiles, the row sum of the undropped exponentials, e z one fp32 product rounded to bf16 before P V; the backward
    from the bf16 o: delta = rowsum(dO o), dS = P (dP z - delta) scale rounded to bf16, dq / dk summed over 64-row tiles,
    dv from bf16(P z).  q, k, v, dout [B, H, S, D] bf16.  Returns (o, lse, dq, dk, dv)."""
    B, H, Sq, D = q.shape
    Sk = k.shape[-2]
    qf, kf, vf, g = q.float(), k.float(), v.float(), dout.float()
    Z = _flat_keep(_attn_mask_index(B, H, Sq, Sk), p)
    Zm = Z
    if mutant == "stride_rounded_to_64":
        Zm = _flat_keep(_attn_mask_index(B, H, Sq, Sk, stride=-(-Sk // 64) * 64), p)
    elif mutant == "head_dropped":
        Zm = _flat_keep(_attn_mask_index(B, H, Sq, Sk, head=False), p)
    elif mutant == "transposed":
        Zm = _flat_keep(_attn_mask_index(B, H, Sk, Sq), p).transpose(-1, -2)
    elif mutant == "last_key_tile_unmasked":
        Zm = Z.clone()
        Zm[..., (Sk - 1) // 64 * 64:] = 1.0
    elif mutant == "last_query_rows_unmasked":
        Zm = Z.clone()
        Zm[..., (Sq - 1) // 64 * 64:, :] = 1.0
    m = torch.full((B, H, Sq, 1), float("-inf"))
    lsum = torch.zeros(B, H, Sq, 1)
    acc = torch.zeros(B, H, Sq, D)
    accu = torch.zeros(B, H, Sq, D)                            # the undropped output (for the delta mutant)
    for t0 in range(0, Sk, 64):
        s = (qf @ kf[..., t0:t0 + 64, :].transpose(-1, -2)) * scale
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp(m - m_new)
        e = torch.exp(s - m_new)
        ez = e * Zm[..., t0:t0 + 64]
        lsum = lsum * alpha + (ez if mutant == "rowsum_after_mask" else e).sum(-1, keepdim=True)
        acc = acc * alpha + fb.bf16_round(ez) @ vf[..., t0:t0 + 64, :]
        accu = accu * alpha + fb.bf16_round(e) @ vf[..., t0:t0 + 64, :]
        m = m_new
    o = (acc / lsum).to(BF16)
    lse = (m + torch.log(lsum))[..., 0]
    # backward, from the o and lse above
    Zb = Zm
    if mutant == "one_element_flipped":                        # where the row's probability is largest: the visible place
        Zb = Z.clone()
        j = int(torch.exp((qf[0, 1, 7] @ kf[0, 1].T) * scale - lse[0, 1, 7]).argmax())
        Zb[0, 1, 7, j] = 0.0 if float(Zb[0, 1, 7, j]) > 0 else float(Z.max())
    one = torch.ones_like(Z)
    Zq, Zk, Zv = (one if mutant == f"d{n}_unmasked" else Zb for n in "qkv")
    P = torch.exp((qf @ kf.transpose(-1, -2)) * scale - lse[..., None])
    dp = g @ vf.transpose(-1, -2)
    o_delta = (accu / lsum).to(BF16) if mutant == "delta_from_undropped_o" else o
    delta = (g * o_delta.float()).sum(-1, keepdim=True)
    dSq = fb.bf16_round(P * (dp * Zq - delta) * scale)
    dSk = fb.bf16_round(P * (dp * Zk - delta) * scale)
    Pv = fb.bf16_round(P * Zv)
    dq = torch.zeros_like(qf)
    for t0 in range(0, Sk, 64):
        dq = dq + dSq[..., t0:t0 + 64] @ kf[..., t0:t0 + 64, :]
    dk, dv = torch.zeros_like(kf), torch.zeros_like(vf)
    for t0 in range(0, Sq, 64):
        dk = dk + dSk[..., t0:t0 + 64, :].transpose(-1, -2) @ qf[..., t0:t0 + 64, :]
        dv = dv + Pv[..., t0:t0 + 64, :].transpose(-1, -2) @ g[..., t0:t0 + 64, :]
    return o, lse, dq.to(BF16), dk.to(BF16), dv.to(BF16)


def _attn_dropout_case(B, H, Sq, Sk, D, p, mutant=None):
    q, k, v, dout = (fb.rnd(B, H, S, D, seed=91 + n).to(BF16) for n, S in enumerate((Sq, Sk, Sk, Sq)))
    scale = D ** -0.5
    o, lse, dq, dk, dv = emu_attn_dropout(q, k, v, dout, scale, p, mutant)
    keep = fb.keep_mask_ref(QF_SEED, B * H * Sq, Sk, p).view(B, H, Sq, Sk)
    r = fb.attn_ref_bound(q, k, v, scale, fb.attn_mask(B, Sq, Sk, False, None, "cpu"), dout=dout, o_in=o, lse_in=lse, keep=keep)
    got = dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)
    ratios, fails = {}, []
    for nm in got:
        try:
            ratios[nm] = fb.assert_within(got[nm], r[nm], r[nm + "_bound"], "attention dropout " + nm)
        except AssertionError as e:
            fails.append(str(e))
    if fails:
        raise AssertionError(" | ".join(fails))
    return ratios


ATTN_DROP_CPU_CASES = [(2, 3, 33, 65, 64), (2, 3, 81, 257, 64), (1, 2, 65, 65, 88), (2, 3, 1, 31, 128)]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("case", ATTN_DROP_CPU_CASES)
def test_attention_dropout_emulation_is_within_the_bound(case, p):
    ratios = _attn_dropout_case(*case, p)
    assert min(ratios.values()) > 1e-3, ratios


@pytest.mark.parametrize("mutant", ATTN_DROP_MUTANTS)
def test_attention_dropout_mutant_fails_the_bound(mutant):
    with pytest.raises(AssertionError, match="out of bound"):
        _attn_dropout_case(2, 3, 65, 65, 64, 0.1, mutant)


def test_attention_bound_without_a_mask_is_unchanged_and_a_mask_of_ones_adds_only_its_roundings():
    B, H, Sq, Sk, D = 2, 2, 33, 65, 64
    q, k, v, dout = (fb.rnd(B, H, S, D, seed=95 + n).to(BF16) for n, S in enumerate((Sq, Sk, Sk, Sq)))
    mask = fb.attn_mask(B, Sq, Sk, False, None, "cpu")
    e = 1e-3 * dout.float().abs()
    r0 = fb.attn_ref_bound(q, k, v, D ** -0.5, mask, dout=dout, dout_err=e)
    rn = fb.attn_ref_bound(q, k, v, D ** -0.5, mask, dout=dout, dout_err=e, keep=None)
    r1 = fb.attn_ref_bound(q, k, v, D ** -0.5, mask, dout=dout, dout_err=e, keep=torch.ones(B, H, Sq, Sk))
    assert set(r0) == set(rn) == set(r1)
    for nm in r0:
        assert torch.equal(r0[nm], rn[nm]), nm
        if nm.endswith("_bound") or nm.endswith("_bound_acc"):
            assert bool((r1[nm] >= r0[nm]).all()) and bool((r1[nm] <= r0[nm] * (1 + 1e-3)).all()), nm
        else:
            assert torch.equal(r0[nm], r1[nm]), nm


# ------------------------------------------------------------------------------------ Q-Former training: LayerNorm dropout
LN_DROP_FWD_MUTANTS = ["mask_on_the_sum", "statistics_of_the_unmasked_x", "mask_before_bias", "seed_in_for_the_output_mask",
                       "mask_stride_256"]
LN_DROP_BWD_MUTANTS = ["seed_in_for_the_output_mask", "mask_stride_256", "dx_masked", "dz_unmasked"]
LN_SEED_IN, LN_SEED_OUT = QF_SEED ^ 0x1111, QF_SEED ^ 0x2222


def _ln_masks(M, D, p_in, p_out, mutant=None):
    idx = torch.arange(M)[:, None] * (256 if mutant == "mask_stride_256" else D) + torch.arange(D)[None]
    ki = _flat_keep(idx, p_in, LN_SEED_IN)
    ko = _flat_keep(idx, p_out, LN_SEED_IN if mutant == "seed_in_for_the_output_mask" else LN_SEED_OUT)
    return ki, ko


def emu_ln_dropout_fwd(z, res, w, b, eps, p_in, p_out, mutant=None):
    """layernorm_fwd_dropout_kernel: thread t of 256 sums elements t, t + 256, ... serially, then block_sum; the statistics from
    the x it wrote.  Returns (x, y f32, y bf16)."""
    M, D = z.shape
    ki, ko = _ln_masks(M, D, p_in, p_out, mutant)
    x = z
    if res is not None:
        x = (z + res) * ki if mutant == "mask_on_the_sum" else z * ki + res
    xs = z + res if mutant == "statistics_of_the_unmasked_x" else x
    mean = emu_strided_sum(xs) / D
    r = torch.rsqrt(emu_strided_sum((xs - mean) * (xs - mean)) / D + eps)
    if mutant == "mask_before_bias":
        y = (x - mean) * r * w * ko + b
    else:
        y = ((x - mean) * r * w + b) * ko
    return x, y, y.to(BF16)


def emu_ln_dropout_bwd(dy, x, w, eps, p_in, p_out, mutant=None):
    """layernorm_bwd_dropout_kernel: (dx f32, dz bf16)."""
    M, D = x.shape
    ki, ko = _ln_masks(M, D, p_in, p_out, mutant)
    mean = emu_strided_sum(x) / D
    d = x - mean
    r = torch.rsqrt(emu_strided_sum(d * d) / D + eps)
    g = dy * ko * w
    sg = emu_strided_sum(g) / D
    sgx = emu_strided_sum(g * d * r) / D
    o = r * (g - sg - d * r * sgx)
    dx = o * ki if mutant == "dx_masked" else o
    dz = o if mutant == "dz_unmasked" else o * ki
    return dx, dz.to(BF16)


def _ln_dropout_case(M, D, p_in, p_out, with_res=True, mutant=None, which="fwd"):
    eps = 1e-12
    res = fb.norm_rows(M, D, seed=101) if with_res else None
    z = fb.rnd(M, D, seed=102) if with_res else fb.norm_rows(M, D, seed=101)
    w = fb.norm_weight(D, seed=103) if D >= 8 else 1 + 0.5 * fb.rnd(D, seed=103)
    b, dy = 0.1 * fb.rnd(D, seed=104), fb.rnd(M, D, seed=105)
    ki = fb.keep_mask_ref(LN_SEED_IN, M, D, p_in) if with_res else None
    ko = fb.keep_mask_ref(LN_SEED_OUT, M, D, p_out)
    ratios = []
    if which == "fwd":
        x, yf, yb = emu_ln_dropout_fwd(z, res, w, b, eps, p_in if with_res else 0.0, p_out, mutant)
        r = fb.ln_dropout_fwd_ref_bound(z, res, w, b, eps, ki, ko, x_out=x)
        if with_res:
            ratios.append(fb.assert_within(x, r["x"], r["x_bound"], "ln dropout x"))
        ratios.append(fb.assert_within(yf, r["y"], r["y_bound"], "ln dropout y f32"))
        ratios.append(fb.assert_within(yb, r["y"], r["y_bf16_bound"], "ln dropout y bf16"))
    else:
        x = z * ki + res if with_res else z
        dx, dz = emu_ln_dropout_bwd(dy, x, w, eps, p_in if with_res else 0.0, p_out, mutant)
        r = fb.ln_dropout_bwd_ref_bound(dy, x, w, eps, ki, ko)
        fails = []
        for nm, got in (("dx", dx), ("dz", dz)):
            try:
                ratios.append(fb.assert_within(got, r[nm], r[nm + "_bound"], "ln dropout " + nm))
            except AssertionError as e:
                fails.append(str(e))
        if fails:
            raise AssertionError(" | ".join(fails))
    return ratios


@pytest.mark.parametrize("M,D,p_in,p_out,with_res", [(13, 300, 0.1, 0.25, True), (13, 768, 0.1, 0.0, True), (7, 257, 0.0, 0.1, False),
                                                     (13, 8, 0.5, 0.5, True), (1, 1030, 0.0, 0.0, True)])
def test_layernorm_dropout_emulation_is_within_the_bound(M, D, p_in, p_out, with_res):
    ratios = _ln_dropout_case(M, D, p_in, p_out, with_res, None, "fwd") + _ln_dropout_case(M, D, p_in, p_out, with_res, None, "bwd")
    assert min(ratios) > 1e-3, ratios


@pytest.mark.parametrize("mutant", LN_DROP_FWD_MUTANTS)
def test_layernorm_dropout_forward_mutant_fails(mutant):
    with pytest.raises(AssertionError, match="out of bound"):
        _ln_dropout_case(13, 300, 0.1, 0.25, True, mutant, "fwd")


@pytest.mark.parametrize("mutant", LN_DROP_BWD_MUTANTS)
def test_layernorm_dropout_backward_mutant_fails(mutant):
    with pytest.raises(AssertionError, match="out of bound"):
        _ln_dropout_case(13, 300, 0.1, 0.25, True, mutant, "bwd")


# ------------------------------------------------------------------------------------- Q-Former training: TN weight gradient
TN_MUTANTS = ["rows_past_M_counted", "split_boundary_row_twice", "empty_split_unwritten", "bias_by_every_k_tile", "accumulate_overwrites"]


def emu_tn_wgrad(dyp, xp, M, splits, prev=None, prev_bias=None, mutant=None):
    """gemm_tn_wgrad_kernel + tn_split_reduce_kernel: split z covers rows [z rows_per, min(M, (z + 1) rows_per)), one 32-row
    product added per step in fp32; a staging thread adds its dy values over the steps, the 32 staging rows are added in order;
    the splits' partials (poisoned workspace) are added in split order.  dyp / xp: the parent buffers, whose rows past M hold
    +-1e4.  Returns (dW, db)."""
    N, K = dyp.shape[1], xp.shape[1]
    rows_per = fb.tn_rows_per(M, splits)
    ws, wsb = fb.poisoned((splits, N, K), F32, "cpu"), fb.poisoned((splits, N), F32, "cpu")
    for z in range(splits):
        m0 = z * rows_per
        m1 = min(M, m0 + rows_per)
        if mutant == "empty_split_unwritten" and m0 >= m1:
            continue
        if mutant == "split_boundary_row_twice":               # the split's end row belongs to the next split as well
            m1 = min(M, m1 + 1)
        acc, stage = torch.zeros(N, K), torch.zeros(fb.TN_BM, N)
        for mb in range(m0, m1, fb.TN_BM):
            hi = mb + fb.TN_BM if mutant == "rows_past_M_counted" else min(m1, mb + fb.TN_BM)
            acc = acc + dyp[mb:hi].float().T @ xp[mb:hi].float()
            stage[:hi - mb] = stage[:hi - mb] + dyp[mb:hi].float()
        bs = torch.zeros(N)
        for rr in range(fb.TN_BM):
            bs = bs + stage[rr]
        ws[z], wsb[z] = acc, bs * (K // 64 if mutant == "bias_by_every_k_tile" else 1)
    dW, db = ws[0], wsb[0]
    for z in range(1, splits):
        dW, db = dW + ws[z], db + wsb[z]
    if prev is not None and mutant != "accumulate_overwrites":
        dW, db = prev + dW, prev_bias + db
    return dW, db


def _tn_case(M, N, K, splits, accumulate, mutant=None):
    dyp = fb.lora_rows(M + 40, N, seed=111).to(BF16)
    xp = fb.rnd(M + 40, K, seed=112).to(BF16)
    dyp[M:], xp[M:] = 1e4, -1e4
    prev, prev_bias = (fb.rnd(N, K, seed=113), fb.rnd(N, seed=114)) if accumulate else (None, None)
    dW, db = emu_tn_wgrad(dyp, xp, M, splits, prev, prev_bias, mutant)
    rW, eW, rb, eb = fb.tn_wgrad_ref_bound(dyp[:M], xp[:M], splits, prev, prev_bias)
    fails, ratios = [], []
    for nm, got, ref, bnd in (("dW", dW, rW, eW), ("db", db, rb, eb)):
        try:
            ratios.append(fb.assert_within(got, ref, bnd, "tn_wgrad " + nm))
        except AssertionError as e:
            fails.append(str(e))
    if fails:
        raise AssertionError(" | ".join(fails))
    return ratios


@pytest.mark.parametrize("M,N,K,splits,accumulate", [(40, 64, 128, 3, True), (33, 128, 64, 8, False), (257, 64, 64, 2, False),
                                                     (1, 64, 64, 1, True), (31, 64, 192, 1, False)])
def test_tn_wgrad_emulation_is_within_the_bound(M, N, K, splits, accumulate):
    ratios = _tn_case(M, N, K, splits, accumulate)
    assert min(ratios) > 1e-3, ratios


@pytest.mark.parametrize("mutant", TN_MUTANTS)
def test_tn_wgrad_mutant_fails(mutant):
    with pytest.raises(AssertionError, match="out of bound"):
        _tn_case(40, 64, 128, 3, True, mutant)


def test_layernorm_dropout_generator_keeps_every_row_well_defined():
    """The condition on the GPU module's inputs: with the residual and the masks applied (forms b - d) no row's variance is lost
    to the mean's rounding unless the row is constant -- layernorm_ref_bound raises otherwise -- at every shape used there."""
    for M in (13, 1):
        for D in (1, 8, 255, 256, 257, 768, 1030):
            for form in "abcd":
                z, res, w, b, dy, p_in, p_out = fb.ln_dropout_inputs(M, D, form, seed=700 + D)
                ki, ko = fb.keep_mask_ref(0x1234567811111111, M, D, p_in), fb.keep_mask_ref(0x7ABCDEF022222222, M, D, p_out)
                x = z if res is None else z * ki + res
                fb.ln_dropout_fwd_ref_bound(z, res, w, b, 1e-12, ki, ko, x_out=x)
                fb.ln_dropout_bwd_ref_bound(dy, x, w, 1e-12, ki, ko)


# ------------------------------------------------------------------------------------------- one-query decode attention
def _xor_sum(x, steps):
    """The butterfly v += shfl_xor(v, o) over the last axis (the lanes), for o in steps."""
    idx = torch.arange(x.shape[-1])
    for o in steps:
        x = x + x[..., idx ^ o]
    return x


def _emu_scores(q, k, scale):
    """fp32 scores of one query per row as the decode kernels form them: qf = q * scale, 16 lanes of 8 serial multiply-adds per
    key, the xor butterfly 1, 2, 4, 8.  q [N, D], k [N, n, D] fp32 (bf16-valued) -> [N, n]."""
    N, n, D = k.shape
    qf = torch.zeros(N, 128)
    qf[:, :D] = q * torch.tensor(scale, dtype=F32)
    kp = torch.zeros(N, n, 128)
    kp[..., :D] = k
    qf, kp = qf.view(N, 1, 16, 8), kp.view(N, n, 16, 8)
    s = torch.zeros(N, n, 16)
    for e in range(8):
        s = s + qf[..., e] * kp[..., e]
    return _xor_sum(s, (1, 2, 4, 8))[..., 0]


def _emu_softmax_stats(s, n_sum=None):
    """(mx [N], e [N, n], sum [N]): every lane adds its keys j = lane, lane + 64, ... serially, then the 6-step butterfly.
    n_sum: keys the normaliser covers (a mutant's; default all)."""
    N, n = s.shape
    mx = s.amax(-1)
    e = torch.exp(s - mx[:, None])
    n_sum = n if n_sum is None else n_sum
    steps = -(-n // 64)
    ep = torch.zeros(N, steps * 64)
    ep[:, :n_sum] = e[:, :n_sum]
    ep = ep.view(N, steps, 64)
    acc = torch.zeros(N, 64)
    for t in range(steps):
        acc = acc + ep[:, t]
    return mx, e, _xor_sum(acc, (32, 16, 8, 4, 2, 1))[:, 0]


def _emu_pv(e, v, waves):
    """Wave w adds the keys w, w + waves, ... serially: [N, waves, D] partial outputs."""
    N, n, D = v.shape
    steps = -(-n // waves)
    ep = torch.zeros(N, steps * waves)
    ep[:, :n] = e
    vp = torch.zeros(N, steps * waves, D)
    vp[:, :n] = v
    ep, vp = ep.view(N, steps, waves), vp.view(N, steps, waves, D)
    o = torch.zeros(N, waves, D)
    for t in range(steps):
        o = o + ep[:, t, :, None] * vp[:, t]
    return o


def emu_decode_one_row(q, k, v, scale, n, mutant=None):
    """attn_decode_kernel's phases 1 to 3 for n keys: 16 waves, the wave partials added in order, the product by 1 / sum, one
    bf16 rounding; lse = mx + log(sum).  q [N, D], k / v [N, T, D] fp32 -> (o [N, D] bf16, lse [N] f32)."""
    N, D = q.shape
    n = n + {"kv_len_plus_one": 1, "kv_len_minus_one": -1}.get(mutant, 0)
    if n <= 0:
        return torch.zeros(N, D).to(BF16), torch.full((N,), float("-inf"))
    s = _emu_scores(q, k[:, :n], scale)
    mx, e, tot = _emu_softmax_stats(s, 64 * (n // 64) if mutant == "normaliser_without_its_tail" else None)
    if mutant == "last_key_dropped":
        e = e.clone()
        e[:, n - 1] = 0
    part = _emu_pv(e, v[:, :n], 16)
    if mutant == "one_wave_dropped":
        part[:, 5] = 0                                      # the keys j % 16 == 5
    r = torch.zeros(N, D)
    for w in range(16):
        r = r + part[:, w]
    return (r * (1.0 / tot)[:, None]).to(BF16), mx + torch.log(tot)


def emu_decode_split(q, k, v, scale, n, chunk, mutant=None):
    """attn_decode_split_kernel per chunk (4 waves, ((p0 + p1) + p2) + p3, the chunk's own m and l) and the in-order merge of
    attn_decode_combine_kernel.  Returns o [N, D] bf16."""
    N, D = q.shape
    nc = -(-n // chunk)
    recs = []
    for c in range(nc):
        j0, j1 = c * chunk, min(n, (c + 1) * chunk)
        mx, e, tot = _emu_softmax_stats(_emu_scores(q, k[:, j0:j1], scale))
        p = _emu_pv(e, v[:, j0:j1], 4)
        recs.append((mx, tot, ((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]))
    M = torch.stack([r[0] for r in recs]).amax(0)
    L, o = torch.zeros(N), torch.zeros(N, D)
    for c, (mx, tot, oc) in enumerate(recs):
        if mutant == "chunk_record_skipped" and c == nc - 1:
            continue
        if mutant == "wrong_chunk_max":
            mx = recs[(c + 1) % nc][0]
        w = torch.exp(mx - M)
        L = L + w * tot
        o = o + w[:, None] * oc
    return (o * (1.0 / L)[:, None]).to(BF16)


def _decode_operands(D, H, T, lens, pos, seed, unrotated_key=False):
    """One launch of the decode grid on the host: row b appends at cache row n_b - 1 (n_b = min(kv_len, T); row 0 when it has no
    key) with the rotary at pos[b].  Returns the fp32 operands an emulation multiplies (its own fp32 rotation, rounded once), the
    reference's (rope_bf16) with their uncertainties, and the clamped lengths.  Rows at and past n_b hold NaN."""
    B, W = len(lens), H * D
    qkv, cache, cos, sin = fb.decode_attn_inputs(B, H, D, T, seed)
    pl = torch.tensor(pos)[:, None]
    heads = lambda t: t.float().view(B, 1, H, D).transpose(1, 2)
    q, kn, vn = heads(qkv[:, :W]), heads(qkv[:, W:2 * W]), heads(qkv[:, 2 * W:3 * W])
    qr, qe = fb.rope_bf16(q, pl, cos, sin)
    kr, ke_new = fb.rope_bf16(kn, pl, cos, sin)
    q32 = fb.rope64(q, pl, cos, sin).to(BF16).float()
    k32 = kn if unrotated_key else fb.rope64(kn, pl, cos, sin).to(BF16).float()
    k = cache[..., :W].float().view(B, T, H, D).transpose(1, 2).clone()
    v = cache[..., W:].float().view(B, T, H, D).transpose(1, 2).clone()
    ns = [min(n, T) for n in lens]
    kref, ke = k.double(), torch.zeros(B, H, T, D, dtype=torch.float64)
    for b, n in enumerate(ns):
        k[b, :, n:], v[b, :, n:], kref[b, :, n:] = float("nan"), float("nan"), float("nan")
        a = max(n - 1, 0)
        k[b, :, a], v[b, :, a], kref[b, :, a], ke[b, :, a] = k32[b, :, 0], vn[b, :, 0], kr[b, :, 0], ke_new[b, :, 0]
    return dict(q=q32[:, :, 0], k=k, v=v, qr=qr[:, :, 0], qe=qe[:, :, 0], kref=kref, ke=ke, ns=ns, ke_new=ke_new)


def _decode_check(D, H, T, lens, pos, seed, chunk=None, mutant=None):
    c = _decode_operands(D, H, T, lens, pos, seed, unrotated_key=mutant == "appended_key_unrotated")
    scale = D ** -0.5
    r = fb.decode_attn_ref_bound(c["qr"], c["kref"], c["v"], scale, lens, q_err=c["qe"], k_err=c["ke"], chunk=chunk)
    ratios = []
    for b, n in enumerate(c["ns"]):
        if chunk is None:
            o, lse = emu_decode_one_row(c["q"][b], c["k"][b], c["v"][b], scale, n, mutant)
            if n == 0 and mutant is None:
                assert bool((o == 0).all()) and bool((lse == float("-inf")).all()) and bool((r["lse"][b] == float("-inf")).all())
            else:
                ratios.append(fb.assert_within(lse, r["lse"][b], r["lse_bound"][b], f"decode lse, row {b}"))
        else:
            o = emu_decode_split(c["q"][b], c["k"][b], c["v"][b], scale, n, chunk, mutant)
        ratios.append(fb.assert_within(o, r["o"][b], r["o_bound"][b], f"decode o, row {b} of kv_len {lens}"))
    return max(ratios)


@pytest.mark.parametrize("D,H", [(8, 1), (40, 3), (64, 1), (128, 3)])
def test_decode_one_row_emulation_is_within_the_bound_over_the_length_grid(D, H):
    worst = max(_decode_check(D, H, T, lens, pos, fb.decode_seed(D, H)) for T, lens, pos in fb.decode_launches())
    print(f"one-row emulation D={D} H={H}: largest err / bound {worst:.3f}")
    assert worst > 1e-3


def test_decode_one_row_emulation_is_within_the_bound_at_8192_keys():
    worst = _decode_check(128, 1, 8192, [8192], [8191], fb.decode_seed(128, 1) + 5)
    print(f"one-row emulation at 8192 keys: largest err / bound {worst:.3f}")


@pytest.mark.parametrize("chunk", fb.SPLIT_CHUNKS)
@pytest.mark.parametrize("D", [8, 128])
def test_decode_split_emulation_is_within_the_bound_over_the_length_grid(D, chunk):
    lens, T = fb.split_lens(chunk), fb.split_t_cap(chunk)
    worst = max(_decode_check(D, 2, T, lens[i:i + 4], [min(n, T) - 1 for n in lens[i:i + 4]], fb.split_seed(D, chunk), chunk=chunk)
                for i in (0, 4))
    print(f"split emulation D={D} chunk={chunk}: largest err / bound {worst:.3f}")
    assert worst > 1e-3


DECODE_MUTANTS = ["last_key_dropped", "one_wave_dropped", "normaliser_without_its_tail", "appended_key_unrotated", "kv_len_plus_one",
                  "kv_len_minus_one"]


@pytest.mark.parametrize("mutant", DECODE_MUTANTS)
def test_decode_one_row_mutant_fails_the_bound(mutant):
    with pytest.raises(AssertionError, match="out of bound"):
        _decode_check(64, 2, fb.DECODE_T, [200, 145, 113], [199, 150, 3], fb.decode_seed(64, 2), mutant=mutant)


@pytest.mark.parametrize("mutant", ["chunk_record_skipped", "wrong_chunk_max"])
def test_decode_split_mutant_fails_the_bound(mutant):
    with pytest.raises(AssertionError, match="out of bound"):
        _decode_check(64, 2, 293, [257, 129, 293], [256, 128, 292], fb.split_seed(64, 128), chunk=128, mutant=mutant)


def test_decode_bound_is_tighter_than_the_tiled_bound_it_replaces():
    """On the inputs of test_attn_decode_rope_per_row_positions_and_lengths (tests/test_attention_edges_gpu.py): the new o bound is
    element-wise <= attn_ref_bound's o_bound, with the same rope uncertainties handed to both."""
    B, H, D, T = 3, 4, 128, 200
    W = H * D
    pos_b, kv_b, app = [5, 63, 130], [65, 128, 200], 64
    qkv = fb.rnd(B, 3 * W + 64, seed=500).to(BF16)
    cache = fb.rnd(B, T, 2 * W, seed=501).to(BF16)
    cos, sin = fb.rope_tables(D)
    pl = torch.tensor(pos_b)[:, None]
    qr, qe = fb.rope_bf16(qkv[:, :W].float().view(B, 1, H, D).transpose(1, 2), pl, cos, sin)
    kr, ke_new = fb.rope_bf16(qkv[:, W:2 * W].float().view(B, 1, H, D).transpose(1, 2), pl, cos, sin)
    k = cache[:, :, :W].float().view(B, T, H, D).transpose(1, 2).double()
    ke = torch.zeros_like(k)
    k[:, :, app], ke[:, :, app] = kr[:, :, 0], ke_new[:, :, 0]
    v = cache[:, :, W:].float().view(B, T, H, D).transpose(1, 2).clone()
    v[:, :, app] = qkv[:, 2 * W:3 * W].float().view(B, H, D)
    kv_len = torch.tensor(kv_b)
    old = fb.attn_ref_bound(qr, k, v, D ** -0.5, fb.attn_mask(B, 1, T, False, kv_len, "cpu"), q_err=qe, k_err=ke)
    new = fb.decode_attn_ref_bound(qr[:, :, 0], k, v, D ** -0.5, kv_b, q_err=qe[:, :, 0], k_err=ke)
    assert torch.allclose(new["o"], old["o"][:, :, 0], rtol=0, atol=1e-7)        # the same reference but for scale as the launcher's float
    assert bool((new["o_bound"] <= old["o_bound"][:, :, 0]).all())
    print(f"new / old o bound: median {float((new['o_bound'] / old['o_bound'][:, :, 0]).median()):.3f}")


def test_decode_generators_keep_the_rope_ambiguity_rare():
    """The seeds and positions tests/test_decode_attention_edges_gpu.py uses: over the launches of a case at most 1 % of the
    rotated q and appended k elements are ambiguous, and never a whole head row."""
    for D in fb.DECODE_DS:
        for H in fb.DECODE_HS:
            qe, ke = [], []
            for T, lens, pos in fb.decode_launches():
                c = _decode_operands(D, H, T, lens, pos, fb.decode_seed(D, H))
                qe.append(c["qe"]), ke.append(c["ke_new"][:, :, 0])
            fb.assert_rope_exempt_share(torch.stack(qe), f"decode q D={D} H={H}")
            fb.assert_rope_exempt_share(torch.stack(ke), f"decode appended k D={D} H={H}")
    for chunk in fb.SPLIT_CHUNKS:
        for D in fb.SPLIT_DS:
            lens, T = fb.split_lens(chunk), fb.split_t_cap(chunk)
            qe, ke = [], []
            for i in (0, 4):
                c = _decode_operands(D, 2, T, lens[i:i + 4], [min(n, T) - 1 for n in lens[i:i + 4]], fb.split_seed(D, chunk))
                qe.append(c["qe"].reshape(-1, D)), ke.append(c["ke_new"].reshape(-1, D))
            fb.assert_rope_exempt_share(torch.cat(qe), f"split q D={D} chunk={chunk}")
            fb.assert_rope_exempt_share(torch.cat(ke), f"split appended k D={D} chunk={chunk}")
    # the 8192-key case, the score / value edges (q scaled or zeroed) and the draft rows at p0 + j
    share = lambda qkv, H, D, pos, cos, sin, what, q=True: [fb.assert_rope_exempt_share(m, f"{what} {nm}") for nm, m in
                                                            zip(("q", "k"), fb.decode_rope_pair(qkv, H, D, pos, cos, sin)[1::2]) if q or nm == "k"]
    qkv, _, cos, sin = fb.decode_attn_inputs(1, 1, 128, 8192, fb.decode_seed(128, 1) + 5)
    share(qkv, 1, 128, [8191], cos, sin, "8192 keys")
    pos = [n - 1 for n in fb.DECODE_EDGE_LENS]
    for D in (64, 128):
        for kind in fb.DECODE_EDGE_KINDS:
            qkv, _, cos, sin = fb.decode_edge_inputs(kind, 3, 2, D, fb.DECODE_T, fb.decode_seed(D, 2) + 7, pos)
            share(qkv, 2, D, pos, cos, sin, f"{kind} D={D}", q=kind != "q_zero")
    for chunk in fb.SPLIT_CHUNKS:
        _, lens, pos = fb.split_launches(chunk)[1]
        for D in fb.SPLIT_DS:
            qkv, _, cos, sin = fb.decode_edge_inputs("spike_50", 3, fb.SPLIT_HEADS, D, fb.split_t_cap(chunk), fb.split_seed(D, chunk), pos,
                                                     spike_row=chunk + 5, spike=80.0)
            share(qkv, fb.SPLIT_HEADS, D, pos, cos, sin, f"split spike D={D} chunk={chunk}")
    for K in fb.DRAFT_KS:
        for D in fb.DRAFT_DS:
            qkv, _, cos, sin = fb.decode_attn_inputs(3 * K, fb.DRAFT_HEADS, D, fb.DECODE_T, fb.draft_seed(D, K))
            masks = [fb.decode_rope_pair(qkv, fb.DRAFT_HEADS, D, [p + j for p in p0 for j in range(K)], cos, sin)[1::2] for p0 in fb.draft_p0(K)]
            fb.assert_rope_exempt_share(torch.cat([m[0] for m in masks]), f"draft q K={K} D={D}")
            fb.assert_rope_exempt_share(torch.cat([m[1] for m in masks]), f"draft k K={K} D={D}")
