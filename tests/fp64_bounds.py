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


def rope_bf16(x, pos, cos, sin):
    """(bf16-valued fp64 rotation of bf16 x, per-element uncertainty): a kernel rotates in fp32 and rounds once.  Where the fp64
    value lies within 8 u32 of the magnitudes (|x c| + |x' s|) of a rounding midpoint, the kernel's fp32 value may round to the
    other neighbour: that element carries one ulp; every other element rounds as the reference does."""
    x64 = x.double()
    c64, s64 = cos.double(), sin.double()
    r = rope64(x64, pos, c64, s64)
    mag = rope_abs_map(x64.abs(), pos, c64, s64)
    rb = r.float().to(torch.bfloat16).double()
    lo = torch.ldexp(torch.ones_like(r), torch.frexp(r.abs().clamp_min(1e-30))[1] - 8)      # ulp of r's binade (8 bits)
    near_mid = torch.zeros_like(r, dtype=torch.bool)
    for ulp in (lo / 2, lo, 2 * lo):                                                      # a rounding across a binade edge too
        near_mid |= ((r - rb).abs() - ulp / 2).abs() <= 8 * U32 * mag
    ulp = 2 * lo
    return rb, torch.where(near_mid, ulp, torch.zeros_like(r))


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
