"""Poisoned buffers and element-wise fp64 error bounds for the GEMM and attention kernels (shared by the CPU mutation tests and
the GPU edge tests).

Poison: a fixed NaN bit pattern (bf16 0x7FA5, f32 0x7FC0DEAD, int32 0xDEADBEEF).  A kernel that skips an element it owns leaves
the pattern there (NaN: never within a bound); a kernel that writes outside what it owns destroys it (`untouched` is False).

Bounds.  u16 = 2^-8 is bf16's unit roundoff (8 significant bits: round to nearest is within half an ulp, 2^-8 |x| at the
bottom of a binade), u32 = 2^-24 fp32's.  Every bound is a sum of (rounding points) x (the magnitude product the rounded value
is bounded by), never |ref| alone, so a row or head whose values are small next to the tensor's maximum gets a bound of its own
size:

GEMM, |got - ref| <= e with, for P = A B^T and |P| := |A| |B|^T,
    e_acc = alpha * g_acc(K, s) * |P|,  g_acc = (K/16 + s + 2) * u32
        fp32 accumulation of exact bf16 x bf16 products (16 x 8 significant bits fit fp32's 24): every MFMA adds at most 32
        products to the accumulator with one rounding of a partial sum bounded by |P| -- K/16 counts two per instruction, a
        margin of 2 over K/32 -- and the split reduce adds s - 1 slab roundings; + 2 for alpha and the slab read-out.
    + alpha * u16 * |P| when the split partials are bf16 slabs (one rounding per slab, each bounded by its part of |P|),
    + u32-sized roundings of bias / residual additions (2 u32 (|v| + |bias|)),
    gelu: the pre-activation bound times max|gelu'| = 1.13 plus the erf evaluation's error (the
        Abramowitz-Stegun erfc form, |err| <= 1.5e-7: 2e-7 |v| + 4 u32 |gelu(v)|),
    bf16 output: e' = e + u16 (|ref| + e).
Attention (the kernels round rotated q / k to bf16 once, P = exp(s - m) to bf16 before P V and dS to bf16 before dS K / dS^T Q):
    scores: ds_ij = scale g_acc(D) (|q||k|^T)_ij + 2 u32 |s_ij| + the rotation's rounding ambiguity, per element: an fp32
         rotation whose value lies within its own arithmetic error of a bf16 rounding midpoint may round either way, so such an
         element carries one bf16 ulp of uncertainty (rope_bf16: dq_e, dk_e; every other element is exact), giving
         scale (dq_e |k|^T + |q| dk_e^T + dq_e dk_e^T)_ij;
    o:   c_o,i (P|V|)_i with c_o,i = 2 u16 (P and the output rounded) + g_acc(Sk) + 2 max_j ds_ij;
    lse: max_j ds_ij + g_acc(Sk) + 4 u32 (|lse| + 1);
    backward, as a function of its inputs (q, k, v, the o and lse it is handed, dO): P = exp(s - lse) with relative error
         rho_ij = ds_ij + 2 u32 |s_ij - lse_i| + 4 u32; T = dP - delta, dP = dO v^T (error g_acc(D) |dO||v|^T), delta = rowsum(o dO)
         (error g_acc(D) rowsum(|o||dO|)); dS = P T with error e_dS = rho P |T| + P (e_dP + e_delta), then rounded to bf16
         (+ u16 (|dS| + e_dS));
         dq = scale dS k:   scale (e_dS |k| + g_acc(Sk) |dS||k| + |dS| dk_e),  dk likewise with q;
         dv = bf16(P)^T dO: ((u16 + rho) P)^T |dO| + g_acc(Sq) P^T |dO|;  each + u16 (|ref| + e) for the bf16 output.
         The dS error is bounded by P |dP - delta| -- the size of dS itself -- not by P |dO||v|^T: an error in one key tile
         or one row is then out of bound (tests/test_fp64_bounds_cpu.py shows it on an emulation of the kernels).

Row kernels (norm.hip, loss.hip, expert.hip l2norm): one 256-thread workgroup per row sums D terms in fp32 as per-thread serial
sums of float4 chunks (4 ceil(D/1024) terms a thread), a 64-lane butterfly (6 additions), then the wave values in order:
    g_sum(n_thread, n_waves) = (n_thread + 6 + n_waves + 4) * u32 on sum |terms|   (+ 4: the terms' own products / differences),
    g_row(D) = g_sum(4 ceil(D/1024), 4).
Math functions are not correctly rounded.  No HIP math accuracy table is installed next to the compiler this suite was written
against, so these are stated assumptions, not documented figures: expf, logf, rsqrtf, sqrtf and a division are each allowed
C_FN = 4 ulp (c_fn * u32 relative); the fast __expf(a) (an exp2 of a rounded a log2 e) is allowed (4 + 2 |a|) u32.
    rmsnorm: v = mean(x^2) + eps has relative error rho = g_row + 2 u32 (all terms positive), r = rsqrt(v) then
        rel_r = rho/2 (1 + 2 rho) + (C_FN + 1) u32; y = w x r: |y| (rel_r + 3 u32).  Backward dx = r w g - x cc + dres with
        cc = r^3 sum(x w g) / D: e_cc = r^3/D (g_row + 2 u32) sum|x w g| + (3 rel_r + 4 u32) |cc| -- the sum of magnitudes, so a row
        whose gradient cancels keeps a bound of its own size -- and e = (rel_r + 4 u32) |r w g| + |x| (e_cc + 2 u32 |cc|) + 2 u32 |dx|.
    layernorm: e_mean = g_row mean|x| + u32 |mean|; sum (x - m')^2 = sum (x - m)^2 + D (m - m')^2 exactly, so the mean's error
        enters the variance squared: e_var = e_mean^2 + (g_row + 6 u32) var, rho = e_var / (var + eps) (a row with rho > 1/2 must
        be constant: its reference deviation is exactly 0 and r' <= rsqrt(eps) still bounds the output), rel_r as above.
        y = d r w + b, d = x - m: |r w| e_mean + |d r w| (rel_r + 4 u32) + 2 u32 |y|.  Backward dx = r (gw - sg - xh sgx) + dres:
        e_xh = r e_mean + |xh| (rel_r + 2 u32), e_sg = (g_row + 2 u32) mean|gw|, e_sgx = (g_row + 4 u32) mean|gw xh| + mean(|gw| e_xh),
        e = r (e_sg + |sgx| e_xh + |xh| e_sgx + 4 u32 (|gw| + |sg| + |xh sgx|)) + |dx - dres| (rel_r + u32) + 2 u32 (|dx| + |dres|).
    layernorm_param_grads: dgamma = sum_m g xhat, dbeta = sum_m g: sum_m |g| e_xh + (16 + ceil(M/16) + 3) u32 sum_m |g xhat|
        (a column is summed serially over a block's 16 rows, then over the blocks), dbeta without the e_xh term.
    lowrank: see lowrank_ref_bound (block-sum dot products, R serial FMAs, chunked column sums over the rows).
    l2norm_rows: y = x / max(sqrt(sum x^2), eps): |y| (g_row / 2 + (2 C_FN + 2) u32).
    clamp_ce: p_j = exp(x_j - m) / se.  The difference x_j - m is rounded (u32 |x_j - m| absolute, so relative in the exponential),
        rel_se = g_sum + u32 sum_j p_j (C_FN + 1 + |x_j - m|), rho_j = rel_se + (C_FN + 4 + |x_j - m|) u32;
        dlogits_j = gs (p_j - [j = t]): gs (rho_j p_j + u32 |p_j - [j = t]|) + u32 |ref|, then the bf16 rounding; row_loss =
        -log(clamp(p_t)): rho_t + (C_FN + 1) u32 |loss|.  The clamp is a decision: a row whose p_t lies within rho_t p_t + 4 u32 of
        a threshold (fp32 1e-7, or fp32 1 - 1e-7 with 2 u32 more) may take either branch (clamp_ce_check accepts both for that
        row) -- but a row whose label holds the maximum while all other exponentials sum to < u32 / 2 has p_t = 1 in fp32 in
        any summation order (1 + d rounds to 1) and is saturated for certain.  Rows without
        a label (t < 0 or t >= V) and the pad columns V..ldd are exactly zero.
    sum_f32: g_sum(ceil(n/256), 4) sum|x| + u32 |ref|; argmax margin: u32 |margin| (ids exact, first index on ties);
        p_max = 1 / sum __expf(a_j): g_sum + u32 sum_j p_j (4 + 2 |a_j|) + (C_FN + 1) u32, relative.
Elementwise (elementwise.hip; bf16 in, fp32 arithmetic, one bf16 rounding out):
    silu_mul: s = 1 / (1 + __expf(-g)) has rel_s = (4 + 2 |g|) u32 (1 - s) + 3 u32; h = g s u: |h| (rel_s + 3 u32).  Backward
        du = d g s likewise; dg = d u f, f = s + g s (1 - s): e_f = s rel_s + |g| s (1 - s) (rel_s + 2 u32) + |g| s (s rel_s + u32)
        + u32 (|f| + |g s (1 - s)|), e = |d u| e_f + 3 u32 |dg|.  (+ 2^-126 absolute: fp32 underflow of the far negative tail.)
    gelu: the erfc form's allowance of the GEMM epilogue (4 u32 |gelu| + 2e-7 |x|); backward dy (cdf + x pdf):
        |dy| (2e-7 + |x| pdf (4 + x^2) u32 + 4 u32 |gelu'|) + u32 |ref|.
    rope_: rope_bf16 (sign = -1 for the backward): a bf16-valued reference plus a one-ulp ambiguity mask.
    dropout_bf16 / dropout_add_: the keep mask regenerated by the library, then one fp32 product and the output rounding
        (u32 |ref| then bf16) or the sum's (u32 |dy keep| + u32 |ref|).
    Data movement (copies, gathers, scatters, casts, transposes, patchify, decode records): no bound, torch.equal; accumulate
        forms u32 (|a| + |b|).
"""
from __future__ import annotations

import contextlib

import torch

U16 = 2.0 ** -8
U32 = 2.0 ** -24

_INT_VIEW = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.int32: torch.int32}
POISON = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FC0DEAD, torch.int32: -0x21524111}     # -0x21524111 == 0xDEADBEEF as int32


def poison_(t: torch.Tensor) -> torch.Tensor:
    """Fill t (any strides) with its dtype's poison bits; returns t."""
    t.view(_INT_VIEW[t.dtype]).fill_(POISON[t.dtype])
    return t


def poisoned(shape, dtype, device) -> torch.Tensor:
    return poison_(torch.empty(shape, dtype=dtype, device=device))


def untouched(t: torch.Tensor) -> torch.Tensor:
    """Boolean mask: True where t still holds the exact poison bits."""
    return t.view(_INT_VIEW[t.dtype]) == POISON[t.dtype]


def assert_untouched(t: torch.Tensor, what: str = ""):
    ok = untouched(t)
    if not bool(ok.all()):
        idx = tuple(int(i) for i in (~ok).nonzero()[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} element(s) outside the owned window were written, first at {idx} "
                             f"= {t[idx].item()!r}")


@contextlib.contextmanager
def poisoned_allocations(monkeypatch, device_type: str = "cuda"):
    """While active, torch.empty / torch.empty_like return poisoned tensors on `device_type` (bf16, f32, int32): the outputs and
    scratch a wrapper allocates start as NaN, not as whatever the caching allocator last held there.  Build references outside."""
    empty, empty_like = torch.empty, torch.empty_like

    def fill(t):
        if t.device.type == device_type and t.dtype in POISON:
            poison_(t)
        return t

    with monkeypatch.context() as m:
        m.setattr(torch, "empty", lambda *a, **k: fill(empty(*a, **k)))
        m.setattr(torch, "empty_like", lambda *a, **k: fill(empty_like(*a, **k)))
        yield


def assert_within(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str = "") -> float:
    """|got - ref| <= bound element by element (NaN fails).  Returns max err / bound; on failure names the worst element."""
    got64, ref64 = got.double(), ref.double()
    bound64 = torch.broadcast_to(bound.double(), ref64.shape)
    err = (got64 - ref64).abs()
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / bound64.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not worst <= 1.0:
        flat = int(ratio.reshape(-1).argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
        nbad = int((ratio > 1.0).sum())
        raise AssertionError(f"{what}: {nbad} of {ratio.numel()} elements out of bound; worst at {idx}: got {got64[idx].item():.8g} "
                             f"ref {ref64[idx].item():.8g} err {err[idx].item():.3g} bound {bound64[idx].item():.3g} "
                             f"err/bound {ratio[idx].item():.3g}")
    return worst


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


# ---------------------------------------------------------------------------------------------------------------- GEMM
def g_acc(K: int, splits: int = 1) -> float:
    return (K / 16 + splits + 2) * U32


def gemm_ref_bound(a, b, *, alpha=1.0, bias=None, residual=None, gelu=False, out_bf16=False, splits=1, bf16_slabs=False):
    """(ref, bound) in fp64 for out = [residual +] act(alpha * a @ b^T [+ bias]) from bf16 operands (see the module docstring)."""
    a64, b64 = a.double(), b.double()
    P = a64 @ b64.T
    Pabs = a64.abs() @ b64.abs().T
    K = a.shape[1]
    v = alpha * P
    e = abs(alpha) * (g_acc(K, splits) + (U16 if bf16_slabs else 0.0)) * Pabs + U32 * v.abs()
    if bias is not None:
        v = v + bias.double()
        e = e + 2 * U32 * (v.abs() + bias.double().abs())
    if gelu:
        pre = v
        v = torch.nn.functional.gelu(v)
        e = 1.13 * e + 4 * U32 * v.abs() + 2e-7 * pre.abs()
    if residual is not None:
        v = v + residual.double()
        e = e + 2 * U32 * v.abs()
    if out_bf16:
        e = e + U16 * (v.abs() + e)
    return v, e


# ---------------------------------------------------------------------------------------------------------------- attention
def rope64(x, pos, cos, sin, sign=1.0):
    """Rotate-half rotary (modeling_llama.py:109-123) in x's dtype: x [B, H, S, D], pos [B, S] long, tables [max_pos, D/2]."""
    D = x.shape[-1]
    c = torch.cat([cos[pos], cos[pos]], -1)[:, None].to(x.dtype)
    s = torch.cat([sin[pos], sin[pos]], -1)[:, None].to(x.dtype) * sign
    rot = torch.cat([-x[..., D // 2:], x[..., :D // 2]], -1)
    return x * c + rot * s


def rope_abs_map(bnd, pos, cos, sin):
    """Bound of R^T g given a bound of g (element-wise): |c| b_d + |s| b_partner."""
    D = bnd.shape[-1]
    c = torch.cat([cos[pos], cos[pos]], -1)[:, None].to(bnd.dtype).abs()
    s = torch.cat([sin[pos], sin[pos]], -1)[:, None].to(bnd.dtype).abs()
    partner = torch.cat([bnd[..., D // 2:], bnd[..., :D // 2]], -1)
    return c * bnd + s * partner


def rope_bf16(x, pos, cos, sin, sign=1.0):
    """(bf16-valued fp64 rotation of bf16 x, per-element uncertainty): a kernel rotates in fp32 and rounds once.  Where the fp64
    value lies within 8 u32 of the magnitudes (|x c| + |x' s|) of a rounding midpoint, the kernel's fp32 value may round to the
    other neighbour: that element carries one ulp; every other element rounds as the reference does -- except where x c and
    x' s cancel so far that the arithmetic error is no longer small against the result's own ulp (see below)."""
    x64 = x.double()
    c64, s64 = cos.double(), sin.double()
    r = rope64(x64, pos, c64, s64, sign)
    mag = rope_abs_map(x64.abs(), pos, c64, s64)
    rb = r.float().to(torch.bfloat16).double()
    lo = torch.ldexp(torch.ones_like(r), torch.frexp(r.abs().clamp_min(1e-30))[1] - 8)      # ulp of r's binade (8 bits)
    near_mid = torch.zeros_like(r, dtype=torch.bool)
    for ulp in (lo / 2, lo, 2 * lo):                                                      # a rounding across a binade edge too
        near_mid |= ((r - rb).abs() - ulp / 2).abs() <= 8 * U32 * mag
    ulp = 2 * lo
    unc = torch.where(near_mid, ulp, torch.zeros_like(r))
    # cancellation: where the fp32 arithmetic error itself reaches a quarter of the value's bf16 ulp the result can land several
    # ulps away -- such an element carries that error plus the rounding of wherever it lands
    arith = 8 * U32 * mag
    return rb, torch.where(arith >= lo / 4, arith * (1 + 2 * U16) + ulp, unc)


def attn_mask(B, Sq, Sk, causal, kv_len, device):
    """True where key j is visible to query i: [B, 1, Sq, Sk] (causal aligns the last query with the last key)."""
    i = torch.arange(Sq, device=device)[:, None] + (Sk - Sq)
    j = torch.arange(Sk, device=device)[None]
    m = torch.ones(B, 1, Sq, Sk, dtype=torch.bool, device=device)
    if causal:
        m = m & (j <= i)[None, None]
    if kv_len is not None:
        m = m & (j[None, None] < kv_len.to(device).long()[:, None, None, None])
    return m


def _out_round(ref, e):
    return e + U16 * (ref.abs() + e)


def attn_ref_bound(q, k, v, scale, mask, q_err=None, k_err=None, dout=None, dout_err=None, o_in=None, lse_in=None):
    """fp64 attention of bf16-valued q, k, v [B, H, S, D] (q, k as the kernel multiplies them: rotated and rounded, with the
    per-element uncertainties q_err / k_err of rope_bf16) and the visibility mask [B, 1, Sq, Sk].  Returns a dict: o, lse and
    their bounds; with dout [B, H, Sq, D] also dq, dk, dv (w.r.t. the given q, k, v) and their bounds -- the backward of the
    o / lse it is handed (o_in, lse_in: what the kernel's backward reads; default the exact ones).  dout_err bounds an error
    dout itself carries (a product rounded to bf16).  *_bound_acc: the bounds before the output's bf16 rounding."""
    q, k, v = q.double(), k.double(), v.double()
    qe = torch.zeros_like(q) if q_err is None else q_err.double()
    ke = torch.zeros_like(k) if k_err is None else k_err.double()
    D, Sq, Sk = q.shape[-1], q.shape[-2], k.shape[-2]
    kT = k.transpose(-1, -2)
    s = (q @ kT) * scale
    s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    o = P @ v
    Vabs = v.abs()
    PV = P @ Vabs
    ds = (g_acc(D) * (q.abs() @ k.abs().transpose(-1, -2)) + qe @ k.abs().transpose(-1, -2) + q.abs() @ ke.transpose(-1, -2)
          + qe @ ke.transpose(-1, -2)) * scale
    ds = (ds + 2 * U32 * s.abs().masked_fill(~mask, 0.0)).masked_fill(~mask, 0.0)
    ds_row = ds.amax(-1)                                                             # [B, H, Sq]
    c_o = 2 * U16 + g_acc(Sk) + 2 * ds_row
    out = dict(o=o, lse=lse, o_bound=c_o[..., None] * PV + U32 * U16 * PV,
               lse_bound=ds_row + g_acc(Sk) + 4 * U32 * (lse.abs() + 1))
    if dout is None:
        return out
    o_b = o if o_in is None else o_in.double()
    lse_b = lse if lse_in is None else lse_in.double()
    g = dout.double()
    gabs = g.abs()
    Pb = torch.exp(s - lse_b[..., None])                                            # masked: exp(-inf) = 0
    rho = (ds + 2 * U32 * (s - lse_b[..., None]).abs().masked_fill(~mask, 0.0) + 4 * U32).masked_fill(~mask, 0.0)
    dP = g @ v.transpose(-1, -2)
    delta = (g * o_b).sum(-1, keepdim=True)
    T = dP - delta
    dS = Pb * T
    e_dP = g_acc(D) * (gabs @ Vabs.transpose(-1, -2))
    e_delta = g_acc(D) * (gabs * o_b.abs()).sum(-1, keepdim=True)
    if dout_err is not None:                                                         # dS is linear in dO
        e = dout_err.double()
        e_dP = e_dP + e @ Vabs.transpose(-1, -2)
        e_delta = e_delta + (e * o_b.abs()).sum(-1, keepdim=True)
    e_dS = rho * Pb * T.abs() + Pb * (e_dP + e_delta)
    e_dS = e_dS + U16 * (dS.abs() + e_dS)                                            # dS rounded to bf16
    dSa = dS.abs()
    dq = scale * dS @ k
    dk = scale * dS.transpose(-1, -2) @ q
    dv = Pb.transpose(-1, -2) @ g
    e_dq = scale * (e_dS @ k.abs() + g_acc(Sk) * (dSa @ k.abs()) + dSa @ ke)
    e_dk = scale * (e_dS.transpose(-1, -2) @ q.abs() + g_acc(Sq) * (dSa.transpose(-1, -2) @ q.abs()) + dSa.transpose(-1, -2) @ qe)
    e_dv = (((U16 + rho * (1 + U16)) * Pb).transpose(-1, -2) @ gabs + g_acc(Sq) * (Pb.transpose(-1, -2) @ gabs))
    if dout_err is not None:
        e_dv = e_dv + Pb.transpose(-1, -2) @ dout_err.double()
    out.update(dq=dq, dk=dk, dv=dv, dq_bound_acc=e_dq, dk_bound_acc=e_dk, dv_bound_acc=e_dv,
               dq_bound=_out_round(dq, e_dq), dk_bound=_out_round(dk, e_dk), dv_bound=_out_round(dv, e_dv))
    return out


# ---------------------------------------------------------------------------------------------------------------- shared
def rnd(*shape, seed, scale=1.0):
    """Seeded N(0, scale^2) fp32 on the host."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rope_tables(D, max_pos=512, device="cpu"):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(torch.arange(max_pos).float(), inv)
    return fr.cos().contiguous().to(device), fr.sin().contiguous().to(device)


class lib_options:
    """Set library options (include/myriad_hip.h mh_set_option) for a block; the previous values come back in any case."""

    def __init__(self, **opts):
        self.opts, self.prev = opts, {}

    def __enter__(self):
        from myriad_amd import _lib
        for k, v in self.opts.items():
            self.prev[k] = _lib.load().mh_set_option(k.encode(), int(v))
            assert self.prev[k] in (0, 1), k
        return self

    def __exit__(self, *exc):
        from myriad_amd import _lib
        for k, v in self.prev.items():
            _lib.load().mh_set_option(k.encode(), int(v))


# ---------------------------------------------------------------------------------------------------------------- row kernels
C_FN = 4.0                 # assumed ulp allowance of expf / logf / rsqrtf / sqrtf / a division (see the module docstring)
F32_TINY = 2.0 ** -126


def g_sum(n_thread: int, n_waves: int = 4) -> float:
    return (n_thread + 6 + n_waves + 4) * U32


def g_row(D: int) -> float:
    return g_sum(4 * -(-D // 1024), 4)


def f32_value(v: float) -> float:
    """The fp32 value a launcher's float argument takes."""
    return float(torch.tensor(v, dtype=torch.float32))


def _rel_rsqrt(rho):
    rho = rho.clamp(max=0.5)
    return 0.5 * rho * (1 + 2 * rho) + (C_FN + 1) * U32


def bf16_out(ref, e):
    return e + U16 * (ref.abs() + e)


def norm_rows(M: int, D: int, seed: int) -> torch.Tensor:
    """fp32 [M, D] test rows, by row index mod 6: N(0,1); N(0,1) + 1e3; all zeros; constant 0.75; 1e-4 N(0,1); 1e4 N(0,1)
    (the last two adjacent: a small row next to a large one)."""
    x = rnd(M, D, seed=seed)
    k = torch.arange(M) % 6
    x[k == 1] += 1e3
    x[k == 2] = 0.0
    x[k == 3] = 0.75
    x[k == 4] *= 1e-4
    x[k == 5] *= 1e4
    return x


def norm_weight(D: int, seed: int) -> torch.Tensor:
    """A norm weight with a zero and negative entries."""
    w = 1 + 0.5 * rnd(D, seed=seed)
    w[0] = 0.0
    w[1] = -1.3
    w[D - 1] = -0.4
    return w


def rmsnorm_ref_bound(x, w, eps, dy=None, dres=None):
    """fp64 RMSNorm of fp32 x [M, D]: dict y, y_bound (fp32 value), y_bf16_bound; with dy also dx, dx_bound, dx_bf16_bound."""
    x, w = x.double(), w.double()
    D = x.shape[1]
    eps = f32_value(eps)
    v = (x * x).mean(1, keepdim=True) + eps
    r = v.rsqrt()
    rel_r = _rel_rsqrt(torch.full_like(v, g_row(D) + 2 * U32))
    y = w * x * r
    e = y.abs() * (rel_r + 3 * U32)
    out = dict(y=y, y_bound=e, y_bf16_bound=bf16_out(y, e))
    if dy is None:
        return out
    g = dy.double()
    t1 = r * w * g
    dot = (x * w * g).sum(1, keepdim=True)
    cc = r ** 3 * dot / D
    e_cc = r ** 3 / D * (g_row(D) + 2 * U32) * (x * w * g).abs().sum(1, keepdim=True) + (3 * rel_r + 4 * U32) * cc.abs()
    dx = t1 - x * cc
    if dres is not None:
        dx = dx + dres.double()
    e = (rel_r + 4 * U32) * t1.abs() + x.abs() * (e_cc + 2 * U32 * cc.abs()) + 2 * U32 * dx.abs()
    out.update(dx=dx, dx_bound=e, dx_bf16_bound=bf16_out(dx, e))
    return out


def layernorm_ref_bound(x, w, b, eps, dy=None, dres=None):
    """fp64 LayerNorm of fp32 x [M, D] (b may be None for the backward only): dict y, y_bound, y_bf16_bound; with dy also dx,
    dx_bound, dx_bf16_bound.  Raises if a row's variance is lost to the mean's rounding although the row is not constant."""
    x, w = x.double(), w.double()
    D = x.shape[1]
    eps = f32_value(eps)
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    r = (var + eps).rsqrt()
    e_mean = g_row(D) * x.abs().mean(1, keepdim=True) + U32 * mean.abs()
    rho = (e_mean ** 2 + (g_row(D) + 6 * U32) * var) / (var + eps)
    if not bool(((rho <= 0.5) | (d.abs().amax(1, keepdim=True) == 0)).all()):
        raise ValueError("layernorm_ref_bound: a non-constant row whose variance is below the mean's rounding error")
    rel_r = _rel_rsqrt(rho)
    xh = d * r
    e_xh = r * e_mean + xh.abs() * (rel_r + 2 * U32)
    out = dict(xhat=xh, xhat_bound=e_xh)
    if b is not None:
        y = d * r * w + b.double()
        e = (r * w).abs() * e_mean + (d * r * w).abs() * (rel_r + 4 * U32) + 2 * U32 * y.abs()
        out.update(y=y, y_bound=e, y_bf16_bound=bf16_out(y, e))
    if dy is None:
        return out
    gw = dy.double() * w
    sg = gw.mean(1, keepdim=True)
    sgx = (gw * xh).mean(1, keepdim=True)
    e_sg = (g_row(D) + 2 * U32) * gw.abs().mean(1, keepdim=True)
    e_sgx = (g_row(D) + 4 * U32) * (gw * xh).abs().mean(1, keepdim=True) + (gw.abs() * e_xh).mean(1, keepdim=True)
    inner = gw - sg - xh * sgx
    e_inner = e_sg + sgx.abs() * e_xh + xh.abs() * e_sgx + 4 * U32 * (gw.abs() + sg.abs() + (xh * sgx).abs())
    core = r * inner
    dr = dres.double() if dres is not None else torch.zeros_like(core)
    dx = core + dr
    e = r * e_inner + core.abs() * (rel_r + U32) + 2 * U32 * (dx.abs() + dr.abs())
    out.update(dx=dx, dx_bound=e, dx_bf16_bound=bf16_out(dx, e))
    return out


LNP_ROWS = 16              # rows a partial block of mh_layernorm_param_grads sums serially


def layernorm_param_grads_ref_bound(dy, x, eps, keep=None, prev=None):
    """fp64 (dgamma, bound, dbeta, bound) of dgamma = sum_m g xhat, dbeta = sum_m g with g = dy * keep (keep: the dropout mask on
    the LayerNorm's output, or None) (+ prev = (dgamma0, dbeta0) for the accumulate form).  A column is summed serially over the
    16 rows of a block, then over the ceil(M/16) blocks: n = 16 + ceil(M/16) additions, + 3 for the products' roundings;
    xhat's own error (layernorm_ref_bound's e_xh, from the row statistics) enters weighted by |g|."""
    M, D = x.shape
    r = layernorm_ref_bound(x, torch.ones(D, dtype=torch.float64, device=x.device), None, eps)
    xh, e_xh = r["xhat"], r["xhat_bound"]
    g = dy.double() * (keep.double() if keep is not None else 1.0)
    n = (LNP_ROWS + -(-M // LNP_ROWS) + 3) * U32
    dg, db = (g * xh).sum(0), g.sum(0)
    e_g = (g.abs() * e_xh).sum(0) + n * (g * xh).abs().sum(0)
    e_b = n * g.abs().sum(0)
    if prev is not None:
        dg, db = dg + prev[0].double(), db + prev[1].double()
        e_g = e_g + U32 * dg.abs()
        e_b = e_b + U32 * db.abs()
    return dg, e_g, db, e_b


LR_CHUNKS = 16             # row chunks of the low-rank adaptor's weight-gradient partials


def lowrank_ref_bound(x, A, Bm, dy=None, t_in=None):
    """fp64 rank-R adaptor y = x + (x A^T) Bm^T (A [R, D], Bm [D, R], all fp32): dict t, t_bound, y, y_bound; with dy also dx, dA,
    dB and bounds, dB from the t it is handed (t_in, default the exact one).  The R dot products of a row are block sums of D
    terms (g_sum(ceil(D/256), 4) on |x||A|^T); the rank-R update is R serial FMAs; a weight-gradient column sums its chunk's rows
    in four interleaved serial sums, adds those, then the 16 chunks in order: (ceil(ceil(M/16)/4) + 3 + 16 + 2) u32 on the
    magnitudes |dt|^T |x| and |dy|^T |t| -- a gradient that cancels over the rows keeps the bound of its terms."""
    x, A, Bm = x.double(), A.double(), Bm.double()
    M, D = x.shape
    R = A.shape[0]
    gd = g_sum(-(-D // 256), 4)
    t = x @ A.T
    e_t = gd * (x.abs() @ A.abs().T)
    y = x + t @ Bm.T
    e_y = e_t @ Bm.abs().T + (R + 2) * U32 * (x.abs() + t.abs() @ Bm.abs().T)
    out = dict(t=t, t_bound=e_t, y=y, y_bound=e_y)
    if dy is None:
        return out
    g = dy.double()
    tt = t if t_in is None else t_in.double()
    dt = g @ Bm
    e_dt = gd * (g.abs() @ Bm.abs())
    dx = g + dt @ A
    e_dx = e_dt @ A.abs() + (R + 2) * U32 * (g.abs() + dt.abs() @ A.abs())
    n = (-(-(-(-M // LR_CHUNKS)) // 4) + 3 + LR_CHUNKS + 2) * U32
    dA = dt.T @ x
    e_dA = e_dt.T @ x.abs() + n * (dt.abs().T @ x.abs())
    dB = g.T @ tt
    e_dB = n * (g.abs().T @ tt.abs())
    out.update(dx=dx, dx_bound=e_dx, dA=dA, dA_bound=e_dA, dB=dB, dB_bound=e_dB)
    return out


def assert_rope_exempt_share(unc, what=""):
    """The condition on rope_bf16's uncertainty mask: at most 1 % of the elements carry any, and no whole head row does."""
    amb = unc > 0
    share = float(amb.double().mean())
    assert share <= 0.01, f"{what}: {share:.3%} of the rotated elements are ambiguous"
    assert not bool(amb.all(-1).any()), f"{what}: a whole row is ambiguous"


def l2norm_ref_bound(x, eps):
    x = x.double()
    D = x.shape[1]
    n = (x * x).sum(1, keepdim=True).sqrt().clamp_min(f32_value(eps))
    y = x / n
    e = y.abs() * (g_row(D) / 2 + (2 * C_FN + 2) * U32)
    return y, e, bf16_out(y, e)


def sum_ref_bound(x, scale=1.0):
    x = x.double().reshape(-1)
    ref = x.sum() * f32_value(scale)
    return ref, abs(f32_value(scale)) * g_sum(-(-x.numel() // 256), 4) * x.abs().sum() + U32 * ref.abs()


CE_LO = f32_value(1e-7)
CE_HI = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(1e-7, dtype=torch.float32))


def clamp_ce_ref_bound(logits, labels, gscale, ldd=None, n_thread=None, n_waves=16):
    """fp64 clamp-CE of fp32 logits [R, V] (-inf allowed) and labels [R] (-100 / out of range: no label).  Returns a dict:
    loss, loss_bound [R]; dlog, dlog_bound [R, ldd] (bf16 output, pad columns exactly 0); amb [R]: rows whose p_t is within its
    bound of a clamp threshold -- for these loss_alt / dlog_alt hold the other branch.  n_thread / n_waves: the kernel's
    summation shape (default covers both kernels: max(32, ceil(V/256)) terms a thread, 16 waves)."""
    x = logits.double()
    R, V = x.shape
    ldd = V if ldd is None else ldd
    gs = f32_value(gscale)
    n_thread = max(32, -(-V // 256)) if n_thread is None else n_thread
    m = x.amax(1, keepdim=True)
    a = x - m
    ex = a.exp()
    se = ex.sum(1, keepdim=True)
    p = ex / se
    absa = torch.where(p > 0, a.abs(), torch.zeros_like(a))
    rel_se = g_sum(n_thread, n_waves) + U32 * (p * (C_FN + 1 + absa)).sum(1, keepdim=True)
    rho = rel_se + (C_FN + 4 + absa) * U32
    t = labels.long()
    has = (t >= 0) & (t < V)
    tc = t.clamp(0, V - 1)[:, None]
    pt, rho_t = p.gather(1, tc)[:, 0], rho.gather(1, tc)[:, 0]
    slack = rho_t * pt
    # p_t = 1 in fp32 for certain: the label's logit is the maximum (exp(0) = 1) and everything else sums to less than half an
    # ulp of 1, so every partial sum that holds the 1 rounds back to 1 whatever the order, 1 / 1 = 1 and the row is saturated
    a_t = a.gather(1, tc)[:, 0]
    sure_one = (a_t == 0) & ((se[:, 0] - 1) * 1.001 < U32 / 2)
    amb = has & (((pt - CE_LO).abs() <= slack) | (((pt - CE_HI).abs() <= slack + 2 * U32) & ~sure_one))
    inside = (pt >= CE_LO) & (pt <= CE_HI)
    onehot = torch.zeros_like(p).scatter_(1, tc, 1.0)
    g_in = gs * (p - onehot)
    e_in = abs(gs) * (rho * p + U32 * (p - onehot).abs()) + U32 * g_in.abs()
    e_in = bf16_out(g_in, e_in)
    loss_in = -pt.clamp(CE_LO, CE_HI).log()
    loss_in_b = rho_t + (C_FN + 1) * U32 * loss_in.abs()
    # the other side of the nearest threshold
    near_lo = (pt - CE_LO).abs() <= (pt - CE_HI).abs()
    loss_out = -torch.where(near_lo, torch.full_like(pt, CE_LO), torch.full_like(pt, CE_HI)).log()
    loss_out_b = (C_FN + 1) * U32 * loss_out.abs()

    def pick(cond, a_, b_):
        return torch.where(cond if a_.dim() == 1 else cond[:, None], a_, b_)

    zero = torch.zeros_like(g_in)
    live = has & inside
    dlog = pick(live, g_in, zero)
    dlog_b = pick(live, e_in, zero)
    dlog_alt = pick(has & ~inside, g_in, zero)
    dlog_alt_b = pick(has & ~inside, e_in, zero)
    z1 = torch.zeros_like(pt)
    loss = pick(has, pick(inside, loss_in, loss_out), z1)
    loss_b = pick(has, pick(inside, loss_in_b, loss_out_b), z1)
    # the clamp is continuous in p_t: either branch's loss is within the other's bound of the threshold value
    loss_alt, loss_alt_b = loss, loss_b + loss_in_b

    def pad(v):
        return torch.nn.functional.pad(v, (0, ldd - V))

    return dict(loss=loss, loss_bound=loss_b, dlog=pad(dlog), dlog_bound=pad(dlog_b), amb=amb, loss_alt=loss_alt,
                loss_alt_bound=loss_alt_b, dlog_alt=pad(dlog_alt), dlog_alt_bound=pad(dlog_alt_b), p=p, has=has, inside=inside)


def clamp_ce_check(row_loss, dlog, r, what="clamp_ce"):
    """Assert row_loss [R] and dlog [R, ldd] (or None) against clamp_ce_ref_bound's dict; a threshold row may take either
    branch.  Returns (worst loss ratio, worst dlogits ratio) over the unambiguous rows."""
    amb = r["amb"]
    keep = ~amb
    w_loss = assert_within(row_loss[keep], r["loss"][keep], r["loss_bound"][keep], what + " row_loss")
    w_d = 0.0
    if dlog is not None:
        w_d = assert_within(dlog[keep], r["dlog"][keep], r["dlog_bound"][keep], what + " dlogits")
    for i in amb.nonzero()[:, 0].tolist():
        errs = []
        for sfx in ("", "_alt"):
            try:
                assert_within(row_loss[i:i + 1], r["loss" + sfx][i:i + 1], r["loss" + sfx + "_bound"][i:i + 1], f"{what} row {i} loss")
                if dlog is not None:
                    assert_within(dlog[i], r["dlog" + sfx][i], r["dlog" + sfx + "_bound"][i], f"{what} row {i} dlogits")
                break
            except AssertionError as e:
                errs.append(str(e))
        else:
            raise AssertionError(f"{what}: threshold row {i} matches neither branch: " + " | ".join(errs))
    return w_loss, w_d


def ce_case(R: int, V: int, seed: int):
    """Logits [R, V] (R >= 10) and labels for the clamp-CE edge rows: 0 label 0; 1 label V-1; 2 a label in the last partial
    float4 (or V-2); 3 no label (-100); 4 label >= V; 5 a -inf logit elsewhere; 6 the label's own logit -inf; 7 p_t far below
    1e-7; 8 p_t far above 1 - 1e-7; the rest random labels."""
    x = rnd(R, V, seed=seed) * 2
    g = torch.Generator().manual_seed(seed + 1)
    y = torch.randint(0, V, (R,), generator=g)
    y[0], y[1], y[2], y[3], y[4] = 0, V - 1, (V // 4) * 4 if V % 4 else V - 2, -100, V + 3
    x[5, (int(y[5]) + 7) % V] = float("-inf")
    x[5, V - 1 if int(y[5]) != V - 1 else V - 2] = float("-inf")
    x[6, y[6]] = float("-inf")
    x[7, y[7]] = x[7].min() - 30
    x[8, y[8]] = x[8].max() + 40
    return x, y


def argmax_ref(x, ban_id=-1, inv_temp=1.0):
    """(ids, margin, margin bound, p_max, p_max relative bound) in fp64; ids: first index on ties, the banned id counts as -inf."""
    x = x.double().clone()
    if ban_id >= 0:
        x[:, ban_id] = float("-inf")
    ids = x.argmax(1)                                   # torch: first index on ties
    top = x.topk(2, 1).values
    margin = top[:, 0] - top[:, 1]
    a = (x - top[:, :1]) * f32_value(inv_temp)
    ex = a.exp()
    s = ex.sum(1)
    p = ex / s[:, None]
    absa = torch.where(p > 0, a.abs(), torch.zeros_like(a))
    rel = max(g_sum(32, 16), g_sum(-(-x.shape[1] // 256), 4)) + U32 * (p * (4 + 2 * absa)).sum(1) + (C_FN + 1) * U32
    return ids, margin, U32 * margin.abs(), 1.0 / s, rel / s


# ---------------------------------------------------------------------------------------------------------------- elementwise
def _sigmoid_rel(g):
    s = torch.sigmoid(g)
    return s, (4 + 2 * g.abs()) * U32 * (1 - s) + 3 * U32


def silu_mul_ref_bound(g, u, dh=None):
    """fp64 h = silu(g) u of bf16-valued g, u (bound incl. the bf16 output rounding); with dh also (dg, bound), (du, bound)."""
    g, u = g.double(), u.double()
    s, rel_s = _sigmoid_rel(g)
    h = g * s * u
    out = [h, bf16_out(h, h.abs() * (rel_s + 3 * U32) + F32_TINY)]
    if dh is None:
        return out
    d = dh.double()
    f = s + g * s * (1 - s)
    e_f = (s * rel_s + g.abs() * s * (1 - s) * (rel_s + 2 * U32) + g.abs() * s * (s * rel_s + U32)
           + U32 * (f.abs() + (g * s * (1 - s)).abs()))
    dg = d * u * f
    du = d * g * s
    out += [dg, bf16_out(dg, (d * u).abs() * e_f + 3 * U32 * dg.abs() + F32_TINY),
            du, bf16_out(du, du.abs() * (rel_s + 3 * U32) + F32_TINY)]
    return out


def gelu_ref_bound(x, dy=None):
    """fp64 erf-GELU of bf16-valued x (bf16 output); with dy the backward dy gelu'(x) instead."""
    x = x.double()
    cdf = 0.5 * torch.special.erfc(-x / 2 ** 0.5)
    if dy is None:
        y = x * cdf
        return y, bf16_out(y, 4 * U32 * y.abs() + 2e-7 * x.abs() + F32_TINY)
    pdf = torch.exp(-x * x / 2) * 0.39894228040143267794
    gp = cdf + x * pdf
    ref = dy.double() * gp
    e = dy.double().abs() * (2e-7 + (x * pdf).abs() * (4 + x * x) * U32 + 4 * U32 * gp.abs()) + U32 * ref.abs() + F32_TINY
    return ref, bf16_out(ref, e)


def rope_rows_ref(x2d, col0, n_heads, head_dim, pos, cos, sin, sign=1.0):
    """rope_bf16 for the in-place layout: x2d [n_tok, ld] bf16, heads at col0.  Returns (ref, ambiguity) as [n_tok, nh * d]."""
    n = x2d.shape[0]
    xs = x2d[:, col0:col0 + n_heads * head_dim].float().reshape(1, n, n_heads, head_dim).transpose(1, 2)
    rb, amb = rope_bf16(xs, pos.long().reshape(1, n), cos, sin, sign)
    return rb.transpose(1, 2).reshape(n, -1), amb.transpose(1, 2).reshape(n, -1)


EW_WRAP = 2 * 4096 * 256      # items a 4096 x 256 elementwise grid covers in two sweeps: more than this needs a third


def frame_of(buf, win_rows: slice, win_cols: slice):
    """The parts of a 2-D (or [.., rows, cols]) buffer outside the window, as a list of views."""
    r0, r1, c0, c1 = win_rows.start, win_rows.stop, win_cols.start, win_cols.stop
    return [buf[..., :r0, :], buf[..., r1:, :], buf[..., r0:r1, :c0], buf[..., r0:r1, c1:]]


def assert_frame_untouched(buf, win_rows: slice, win_cols: slice, what=""):
    for i, f in enumerate(frame_of(buf, win_rows, win_cols)):
        assert_untouched(f, f"{what} frame part {i}")
