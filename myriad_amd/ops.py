"""Thin tensor->pointer wrappers over the C ABI (include/myriad_hip.h).  torch is used only for device memory
and the current HIP stream; all arithmetic happens in libmyriad_hip.so.  No fallbacks."""
from __future__ import annotations

import ctypes
import math
import numbers
from typing import NamedTuple, Optional, Sequence

import os

import torch

from . import _lib

BF16 = torch.bfloat16
F32 = torch.float32

GEMM_OUT_F32 = 1
GEMM_GELU = 2
GEMM_REGSTAGE = 4
GEMM_VARIANT = 0      # 0 = library default; 1..5 force a kernel variant (tools/gemm_bench.py A/B tests)


def _L():
    return _lib.load()


_DEV_IDX = None


def _s() -> int:
    """Raw handle of torch's current HIP stream.  `torch.cuda.current_stream().cuda_stream` builds a Stream object per
    call (~8 us, 1200 times per step = the largest single host cost of a batch-1 step); the raw getter is a C call."""
    global _DEV_IDX
    if _DEV_IDX is None:
        _DEV_IDX = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(_DEV_IDX)


class _PinnedRing:
    """Small host->device uploads (index vectors, lengths, labels) without stalling the launch thread: `.to(device)` from
    pageable memory blocks until the stream drains (12 such stalls per step cost ~14 ms at batch 1).  The payload is
    staged in a slot of a pinned ring and copied with non_blocking=True; a slot is reused only after its copy event."""

    def __init__(self, slots: int = 64, slot_bytes: int = 1 << 16):
        self.buf = torch.empty((slots, slot_bytes), dtype=torch.uint8).pin_memory()
        self.events = [None] * slots
        self.slots, self.slot_bytes, self.i = slots, slot_bytes, 0

    def upload(self, t: torch.Tensor, device) -> torch.Tensor:
        t = t.contiguous()
        nbytes = t.numel() * t.element_size()
        if nbytes == 0 or nbytes > self.slot_bytes or t.is_cuda:
            return t.to(device)
        k = self.i
        self.i = (k + 1) % self.slots
        if self.events[k] is not None:
            self.events[k].synchronize()
        stage = self.buf[k, :nbytes].view(t.dtype).view(t.shape)
        stage.copy_(t)
        out = torch.empty(t.shape, dtype=t.dtype, device=device)
        out.copy_(stage, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[k] = ev
        return out


_RING = None


def h2d(t: torch.Tensor, device) -> torch.Tensor:
    """Asynchronous upload of a small host tensor (see _PinnedRing)."""
    global _RING
    if _RING is None:
        _RING = _PinnedRing()
    return _RING.upload(t, device)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _chk2d(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
        raise _lib.MyriadHipError(f"{name}: need cuda {dtype} 2-D tensor with unit inner stride, got "
                                  f"{t.dtype} {tuple(t.shape)} strides {t.stride()} cuda={t.is_cuda}")


_WS = {}


def ensure_workspace(device, nbytes: int = 256 << 20):
    """Register a split-K scratch buffer with the library (once per device)."""
    key = str(device)
    if key not in _WS:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _lib.check(_L().mh_set_workspace(buf.data_ptr(), nbytes), "mh_set_workspace")
        _WS[key] = buf
    return _WS[key]


_SIDE = {}


def side_stream(device, name: str) -> "torch.cuda.Stream":
    """A named side stream of the device with its OWN split-K scratch (two streams that both split K must not share one;
    mh_set_stream_workspace).  One per (device, name) for the whole process: every model instance shares them."""
    key = (str(device), name)
    if key not in _SIDE:
        main_ws = ensure_workspace(device)
        st = torch.cuda.Stream(device=device)
        ws = torch.empty(main_ws.numel(), dtype=torch.uint8, device=device)
        _lib.check(_L().mh_set_stream_workspace(st.cuda_stream, ws.data_ptr(), ws.numel()), "mh_set_stream_workspace")
        _SIDE[key] = (st, ws)
    return _SIDE[key][0]


def drop_workspace():
    """Unregister the split-K scratch (tests: the no-workspace paths).  ensure_workspace() registers it again."""
    torch.cuda.synchronize()
    _lib.check(_L().mh_set_workspace(None, 0), "mh_set_workspace")     # also drops every side-stream scratch
    _WS.clear()
    _SIDE.clear()


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# --------------------------------------------------------------------------- GEMM
# One GEMM backend: every product below is the library's own kernels.  (The vendor-library comparison lives in
# tools/gemm_vendor_calib.py, outside the product.)


def gemm(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
         residual: Optional[torch.Tensor] = None, out_dtype=BF16, gelu: bool = False, alpha: float = 1.0,
         regstage: bool = False, variant: int = -1) -> torch.Tensor:
    """out[M,N] = alpha * a[M,K] @ b[N,K]^T (+bias) (gelu) (+residual f32)."""
    _chk2d(a, BF16, "gemm.a")
    _chk2d(b, BF16, "gemm.b")
    M, K = a.shape
    N, K2 = b.shape
    if K != K2:
        raise _lib.MyriadHipError(f"gemm: K mismatch {K} vs {K2}")
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    else:
        _chk2d(out, out.dtype, "gemm.out")
        if out.shape != (M, N):
            raise _lib.MyriadHipError(f"gemm: out shape {tuple(out.shape)} != {(M, N)}")
    flags = (GEMM_OUT_F32 if out.dtype == F32 else 0) | (GEMM_GELU if gelu else 0) | (GEMM_REGSTAGE if regstage else 0)
    flags |= (GEMM_VARIANT if variant < 0 else variant) << 8
    if bias is not None and (bias.dtype != F32 or bias.numel() != N):
        raise _lib.MyriadHipError("gemm: bias must be f32 [N]")
    ldr = 0
    if residual is not None:
        _chk2d(residual, F32, "gemm.residual")
        ldr = residual.stride(0)
    rc = _L().mh_gemm_bf16_nt(_p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N, K, _p(bias),
                              _p(residual), ldr, flags, float(alpha), _s())
    _lib.check(rc, f"mh_gemm_bf16_nt M={M} N={N} K={K}")
    return out


GEMM_KERNEL_NAMES = {0: "gemv_kernel", 1: "gemm_nt_kernel", 2: "gemm_x8_kernel", 3: "gemm_nt_kernel", 4: "gemm_nt_kernel",
                     5: "gemm_nt_kernel", 6: "gemm_nt_kernel"}   # 3: 128x64 tile; 4 / 5: 160x128 / 160x96 row tile (M <= 320); 6: 64x64, 8-deep ring


def gemm_plan(M: int, N: int, K: int, out_f32: bool = False, gelu: bool = False):
    """(kernel id, K splits) the library will use for this shape -- mh_gemm_plan."""
    import ctypes
    kernel, splits = ctypes.c_int(0), ctypes.c_int(0)
    flags = (1 if out_f32 else 0) | (2 if gelu else 0)
    _lib.check(_L().mh_gemm_plan(M, N, K, flags, ctypes.addressof(kernel), ctypes.addressof(splits)), "mh_gemm_plan")
    return kernel.value, splits.value


class PackedWeight:
    """Stream-ordered copy of a frozen [N, K] bf16 weight for the decode kernel (mh_gemv_pack)."""
    __slots__ = ("data", "N", "K")

    def __init__(self, data: torch.Tensor, N: int, K: int):
        self.data, self.N, self.K = data, N, K


def gemv_pack(w: torch.Tensor, out: Optional[PackedWeight] = None) -> PackedWeight:
    """Permute w [N, K] into the order the skinny-M kernel streams it in; `out` re-uses an earlier copy's storage."""
    _chk2d(w, BF16, "gemv_pack.w")
    N, K = w.shape
    n = _L().mh_gemv_pack_elems(N, K)
    if n < 0:
        raise _lib.MyriadHipError(f"gemv_pack: unsupported dims N={N} K={K}")
    if out is None:
        out = PackedWeight(torch.empty((n,), dtype=BF16, device=w.device), N, K)
    elif (out.N, out.K) != (N, K):
        raise _lib.MyriadHipError("gemv_pack: out was packed for another shape")
    _lib.check(_L().mh_gemv_pack(_p(w), w.stride(0), N, K, _p(out.data), _s()), "mh_gemv_pack")
    return out


class PackedFp8Weight:
    """FP8 weight-only copy of a frozen [N, K] bf16 weight for the decode kernel (mh_gemv_pack_fp8): e4m3fn codes in the stream
    order of PackedWeight at one byte per weight (`data`, uint8) and one fp32 scale per output row (`scales` [N])."""
    __slots__ = ("data", "scales", "N", "K")

    def __init__(self, data: torch.Tensor, scales: torch.Tensor, N: int, K: int):
        self.data, self.scales, self.N, self.K = data, scales, N, K


def gemv_pack_fp8(w: torch.Tensor, out: Optional[PackedFp8Weight] = None) -> PackedFp8Weight:
    """Quantise w [N, K] per output row (s_n = amax_n / 448, q = e4m3fn(w / s_n), nearest even, saturated) and permute q into the
    order the skinny-M kernel streams it in; `out` re-uses an earlier copy's storage."""
    _chk2d(w, BF16, "gemv_pack_fp8.w")
    N, K = w.shape
    n = _L().mh_gemv_pack_fp8_elems(N, K)
    if n < 0:
        raise _lib.MyriadHipError(f"gemv_pack_fp8: unsupported dims N={N} K={K}")
    if out is None:
        out = PackedFp8Weight(torch.empty((n,), dtype=torch.uint8, device=w.device), torch.empty((N,), dtype=F32, device=w.device),
                              N, K)
    elif (out.N, out.K) != (N, K):
        raise _lib.MyriadHipError("gemv_pack_fp8: out was packed for another shape")
    _lib.check(_L().mh_gemv_pack_fp8(_p(w), w.stride(0), N, K, _p(out.data), _p(out.scales), _s()), "mh_gemv_pack_fp8")
    return out


class PackedFp4Weight:
    """MXFP4 weight-only copy of a frozen [N, K] bf16 weight for the decode kernel (mh_gemv_pack_fp4): e2m1 codes, two per byte,
    in the stream order of PackedWeight at 128-deep steps (`data`, uint8) and one power-of-two scale byte per 32 consecutive k of
    a row beside them (`scales`, uint8, in the stream order of include/myriad_hip.h)."""
    __slots__ = ("data", "scales", "N", "K")

    def __init__(self, data: torch.Tensor, scales: torch.Tensor, N: int, K: int):
        self.data, self.scales, self.N, self.K = data, scales, N, K


def gemv_pack_fp4(w: torch.Tensor, out: Optional[PackedFp4Weight] = None) -> PackedFp4Weight:
    """Quantise w [N, K] (finite, K % 128 == 0) to MXFP4 -- per block of 32 k the scale byte b = max(2, E - 2) of the block's
    largest exponent field E and the e2m1 codes of w / 2^(b-127), nearest, ties to the even code, saturated at +-6 -- and permute
    codes and scale bytes into the order the skinny-M kernel streams them in; `out` re-uses an earlier copy's storage."""
    _chk2d(w, BF16, "gemv_pack_fp4.w")
    N, K = w.shape
    n, ns = _L().mh_gemv_pack_fp4_elems(N, K), _L().mh_gemv_pack_fp4_scale_elems(N, K)
    if n < 0 or ns < 0:
        raise _lib.MyriadHipError(f"gemv_pack_fp4: unsupported dims N={N} K={K} (K must be a multiple of 128)")
    if out is None:
        out = PackedFp4Weight(torch.empty((n,), dtype=torch.uint8, device=w.device),
                              torch.empty((ns,), dtype=torch.uint8, device=w.device), N, K)
    elif not isinstance(out, PackedFp4Weight) or (out.N, out.K) != (N, K):
        raise _lib.MyriadHipError("gemv_pack_fp4: out was packed for another shape")
    _lib.check(_L().mh_gemv_pack_fp4(_p(w), w.stride(0), N, K, _p(out.data), _p(out.scales), _s()), "mh_gemv_pack_fp4")
    return out


def _packed_entry(base: str, pw) -> str:
    """The library entry of a packed product for this weight class: base, base with _fp8 or with _fp4 after mh_gemv_packed."""
    kind = "_fp8" if isinstance(pw, PackedFp8Weight) else "_fp4" if isinstance(pw, PackedFp4Weight) else ""
    return "mh_gemv_packed" + kind + base


def _lora_merge_args(w: torch.Tensor, a_qv: torch.Tensor, b_q: torch.Tensor, b_v: torch.Tensor, name: str):
    """(D, r) of a merge: w [3D, D] bf16 (unit inner stride, any leading dimension: the frozen columns of wqkv_ext), a_qv [2r, D]
    and b_q / b_v [D, r] fp32 with contiguous rows."""
    _chk2d(w, BF16, name + ".w")
    N, D = w.shape
    if N != 3 * D:
        raise _lib.MyriadHipError(f"{name}: w must be [3D, D], got {tuple(w.shape)}")
    r = a_qv.shape[0] // 2 if a_qv.dim() == 2 else 0
    for t, shape, what in ((a_qv, (2 * r, D), "a_qv"), (b_q, (D, r), "b_q"), (b_v, (D, r), "b_v")):
        if t.dtype != F32 or not t.is_cuda or tuple(t.shape) != shape or t.stride() != (shape[1], 1):
            raise _lib.MyriadHipError(f"{name}: {what} must be a contiguous cuda f32 {shape}, got {t.dtype} {tuple(t.shape)} "
                                      f"strides {t.stride()}")
    return D, r


def lora_merge(w: torch.Tensor, a_qv: torch.Tensor, b_q: torch.Tensor, b_v: torch.Tensor, s: float,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The q / v LoRA folded into the frozen qkv weight (PEFT merge_adapter), row-major bf16 [3D, D]: q rows
    bf16(w + s * sum_j b_q[:, j] a_q[j]), v rows the same with b_v / a_v, k rows w (the rule: include/myriad_hip.h mh_lora_merge)."""
    D, r = _lora_merge_args(w, a_qv, b_q, b_v, "lora_merge")
    if out is None:
        out = torch.empty((3 * D, D), dtype=BF16, device=w.device)
    else:
        _chk2d(out, BF16, "lora_merge.out")
        if out.shape != (3 * D, D):
            raise _lib.MyriadHipError(f"lora_merge: out shape {tuple(out.shape)} != {(3 * D, D)}")
    _lib.check(_L().mh_lora_merge(_p(w), w.stride(0), _p(a_qv), _p(b_q), _p(b_v), D, r, float(s), _p(out), out.stride(0), _s()),
               f"mh_lora_merge D={D} r={r}")
    return out


def lora_merge_pack(w: torch.Tensor, a_qv: torch.Tensor, b_q: torch.Tensor, b_v: torch.Tensor, s: float,
                    out: Optional[PackedWeight] = None) -> PackedWeight:
    """gemv_pack(lora_merge(...)) bit for bit, written in one pass from w; `out` re-uses an earlier copy's storage."""
    D, r = _lora_merge_args(w, a_qv, b_q, b_v, "lora_merge_pack")
    if out is None:
        out = PackedWeight(torch.empty((_L().mh_gemv_pack_elems(3 * D, D),), dtype=BF16, device=w.device), 3 * D, D)
    elif not isinstance(out, PackedWeight) or (out.N, out.K) != (3 * D, D):
        raise _lib.MyriadHipError("lora_merge_pack: out is not a PackedWeight of this shape")
    _lib.check(_L().mh_lora_merge_pack(_p(w), w.stride(0), _p(a_qv), _p(b_q), _p(b_v), D, r, float(s), _p(out.data), _s()),
               f"mh_lora_merge_pack D={D} r={r}")
    return out


def lora_merge_pack_fp8(w: torch.Tensor, a_qv: torch.Tensor, b_q: torch.Tensor, b_v: torch.Tensor, s: float,
                        out: Optional[PackedFp8Weight] = None) -> PackedFp8Weight:
    """gemv_pack_fp8(lora_merge(...)) bit for bit (codes and row scales of the merged bf16 rows), in one pass from w."""
    D, r = _lora_merge_args(w, a_qv, b_q, b_v, "lora_merge_pack_fp8")
    if out is None:
        out = PackedFp8Weight(torch.empty((_L().mh_gemv_pack_fp8_elems(3 * D, D),), dtype=torch.uint8, device=w.device),
                              torch.empty((3 * D,), dtype=F32, device=w.device), 3 * D, D)
    elif not isinstance(out, PackedFp8Weight) or (out.N, out.K) != (3 * D, D):
        raise _lib.MyriadHipError("lora_merge_pack_fp8: out is not a PackedFp8Weight of this shape")
    _lib.check(_L().mh_lora_merge_pack_fp8(_p(w), w.stride(0), _p(a_qv), _p(b_q), _p(b_v), D, r, float(s), _p(out.data),
                                           _p(out.scales), _s()), f"mh_lora_merge_pack_fp8 D={D} r={r}")
    return out


def _gemv_product(base: str, name: Optional[str], a: torch.Tensor, pw, out, bias, residual, out_dtype, alpha, M: int, *pre):
    """The shared part of the packed products: the library entry mh_gemv_packed[_fp8|_fp4]<base> for this weight class, the
    output, the residual check, the weight arguments by class, the call.  `pre` goes between the operand and the weight (the
    fused forms' norm weight and eps); the fused forms (base _rmsnorm / _silu) answer MH_ERR_UNSUPPORTED with None."""
    entry = _packed_entry(base, pw)
    if out is None:
        out = torch.empty((M, pw.N), dtype=out_dtype, device=a.device)
    ldr = 0
    if residual is not None:
        _chk2d(residual, F32, (name or entry) + ".residual")          # the fused forms name their entry, as they always did
        ldr = residual.stride(0)
    wargs = (_p(pw.data), _p(pw.scales)) if isinstance(pw, (PackedFp8Weight, PackedFp4Weight)) else (_p(pw.data),)
    rc = getattr(_L(), entry)(_p(a), a.stride(0), *pre, *wargs, _p(out), out.stride(0), M, pw.N, pw.K, _p(bias), _p(residual), ldr,
                              1 if out.dtype == F32 else 0, float(alpha), _s())
    if rc == -3 and base in ("_rmsnorm", "_silu"):     # MH_ERR_UNSUPPORTED: the operand rows do not fit the fused kernel
        return None
    _lib.check(rc, f"{entry} M={M} N={pw.N} K={pw.K}")
    return out


def gemv_packed(a: torch.Tensor, pw, out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                residual: Optional[torch.Tensor] = None, out_dtype=BF16, alpha: float = 1.0) -> torch.Tensor:
    """out[M <= GEMV_MAX_ROWS, N] = alpha * a @ W^T (+bias) (+residual f32) with W given as its packed copy; same bits as gemm().
    A PackedFp8Weight runs the fp8 kernel: alpha * s_n * a @ q^T, q widened exactly to bf16; a PackedFp4Weight the fp4 kernel:
    alpha * a @ dq(W)^T, each code widened exactly to bf16 with its block scale."""
    _chk2d(a, BF16, "gemv_packed.a")
    M, K = a.shape
    if K != pw.K or M > GEMV_MAX_ROWS:
        raise _lib.MyriadHipError(f"gemv_packed: a is {tuple(a.shape)}, weight was packed as [{pw.N}, {pw.K}], "
                                  f"M must be <= {GEMV_MAX_ROWS}")
    return _gemv_product("", "gemv_packed", a, pw, out, bias, residual, out_dtype, alpha, M)


def gemv_packed_wide(a: torch.Tensor, pw, out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                     residual: Optional[torch.Tensor] = None, out_dtype=BF16, alpha: float = 1.0) -> torch.Tensor:
    """gemv_packed() for up to GEMV_WIDE_MAX_ROWS rows on the same packed copy (mh_gemv_packed*_wide): row m carries the bits
    gemv_packed() gives that row, whatever M; a workgroup shares each activation fragment over several column blocks."""
    _chk2d(a, BF16, "gemv_packed_wide.a")
    M, K = a.shape
    if K != pw.K or M > GEMV_WIDE_MAX_ROWS:
        raise _lib.MyriadHipError(f"gemv_packed_wide: a is {tuple(a.shape)}, weight was packed as [{pw.N}, {pw.K}], "
                                  f"M must be <= {GEMV_WIDE_MAX_ROWS}")
    return _gemv_product("_wide", "gemv_packed_wide", a, pw, out, bias, residual, out_dtype, alpha, M)


def gemv_packed_rmsnorm(h: torch.Tensor, norm_w: torch.Tensor, eps: float, pw, out=None, residual=None,
                        out_dtype=BF16, alpha: float = 1.0):
    """out[M <= GEMV_MAX_ROWS, N] = alpha * rmsnorm(h; norm_w, eps) @ W^T (+residual): mh_rmsnorm_fwd + mh_gemv_packed in one
    launch, same bits.
    Returns None when the operand rows exceed the fused kernel's LDS budget (run the two launches instead)."""
    _chk2d(h, F32, "gemv_packed_rmsnorm.h")
    M, K = h.shape
    if K != pw.K or M > GEMV_MAX_ROWS:
        raise _lib.MyriadHipError(f"gemv_packed_rmsnorm: h is {tuple(h.shape)}, weight was packed as [{pw.N}, {pw.K}]")
    return _gemv_product("_rmsnorm", None, h, pw, out, None, residual, out_dtype, alpha, M, _p(norm_w), float(eps))


def gemv_packed_silu(gu: torch.Tensor, pw, out=None, residual=None, out_dtype=BF16, alpha: float = 1.0):
    """out[M <= GEMV_MAX_ROWS, N] = alpha * (silu(g) * u) @ W^T (+residual) for gu [M, 2K] bf16 in the 128-blocked gate|up layout:
    mh_silu_mul_fwd_blk + mh_gemv_packed in one launch, same bits.  None when the rows exceed the LDS budget."""
    _chk2d(gu, BF16, "gemv_packed_silu.gu")
    M = gu.shape[0]
    if gu.shape[1] != 2 * pw.K or M > GEMV_MAX_ROWS:
        raise _lib.MyriadHipError(f"gemv_packed_silu: gu is {tuple(gu.shape)}, weight was packed as [{pw.N}, {pw.K}]")
    return _gemv_product("_silu", None, gu, pw, out, None, residual, out_dtype, alpha, M)


def attn_decode_rope(qkv2d: torch.Tensor, cache: torch.Tensor, pos: torch.Tensor, pos_dev: torch.Tensor, kv_len: torch.Tensor,
                     cos_tab: torch.Tensor, sin_tab: torch.Tensor, n_heads: int, head_dim: int, scale: float):
    """One decode token: rope_kv_append + attn_fwd(Sq = 1) as one launch (same bits).  qkv2d [B, >=3W] bf16 (q rotated in place),
    cache [B, T, 2W]; returns o [B, W] bf16."""
    _chk2d(qkv2d, BF16, "attn_decode_rope.qkv")
    B, W = qkv2d.shape[0], n_heads * head_dim
    if qkv2d.shape[1] < 3 * W or cache.shape[2] != 2 * W:
        raise _lib.MyriadHipError("attn_decode_rope: qkv must be [B, >=3W] and cache [B, T, 2W]")
    out = torch.empty((B, W), dtype=BF16, device=qkv2d.device)
    _lib.check(_L().mh_attn_decode_rope(_p(qkv2d), qkv2d.stride(0), _p(cache), cache.stride(0), cache.stride(1), _p(pos), _p(pos_dev),
                                        _p(kv_len), _p(cos_tab), _p(sin_tab), _p(out), out.stride(0), B, n_heads, head_dim,
                                        cache.shape[1], float(scale), _s()), "mh_attn_decode_rope")
    return out


def attn_decode_rope_rows(qkv2d: torch.Tensor, cache: torch.Tensor, pos: torch.Tensor, kv_len: torch.Tensor, live: torch.Tensor,
                          cos_tab: torch.Tensor, sin_tab: torch.Tensor, n_heads: int, head_dim: int, scale: float):
    """attn_decode_rope with per-row state (decode slots): row b rotates and appends at pos[b], sees kv_len[b] keys; a row with
    live[b] == 0 (int32 [B]) touches neither qkv2d nor the cache and gets a zero row of o.  A live row has attn_decode_rope's bits."""
    _chk2d(qkv2d, BF16, "attn_decode_rope_rows.qkv")
    B, W = qkv2d.shape[0], n_heads * head_dim
    if qkv2d.shape[1] < 3 * W or cache.shape[2] != 2 * W or cache.shape[0] != B:
        raise _lib.MyriadHipError("attn_decode_rope_rows: qkv must be [B, >=3W] and cache [B, T, 2W]")
    for name, t in (("pos", pos), ("kv_len", kv_len), ("live", live)):
        if t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous():
            raise _lib.MyriadHipError(f"attn_decode_rope_rows: {name} must be a contiguous int32 [B]")
    out = torch.empty((B, W), dtype=BF16, device=qkv2d.device)
    _lib.check(_L().mh_attn_decode_rope_rows(_p(qkv2d), qkv2d.stride(0), _p(cache), cache.stride(0), cache.stride(1), _p(pos),
                                             _p(kv_len), _p(live), _p(cos_tab), _p(sin_tab), _p(out), out.stride(0), B, n_heads,
                                             head_dim, cache.shape[1], float(scale), _s()), "mh_attn_decode_rope_rows")
    return out


DRAFT_MAX_K = 8        # most rows per sequence mh_attn_decode_rope_draft / mh_draft_accept take (include/myriad_hip.h)


def attn_decode_draft_supported(n_heads: int, head_dim: int, K: int, T_cap: int) -> bool:
    """Whether mh_attn_decode_rope_draft takes this shape (head dim, rows per sequence, the LDS for T_cap scores): the launcher's
    own answer to a call with no sequence, which launches nothing."""
    rc = _L().mh_attn_decode_rope_draft(None, 0, None, 0, 0, None, None, None, None, None, 0, 0, int(K), int(n_heads), int(head_dim),
                                        int(T_cap), 1.0, _s())
    if rc == -3:                                                         # MH_ERR_UNSUPPORTED
        return False
    _lib.check(rc, "mh_attn_decode_rope_draft (probe)")
    return True


def attn_decode_rope_draft(qkv2d: torch.Tensor, cache: torch.Tensor, pos: torch.Tensor, live: torch.Tensor, cos_tab: torch.Tensor,
                           sin_tab: torch.Tensor, n_heads: int, head_dim: int, scale: float, K: int,
                           out: Optional[torch.Tensor] = None):
    """K consecutive token steps of each of G sequences as one launch (the verify step of draft-and-verify decoding): row g*K + j
    of qkv2d [G*K, >=3W] is the token at position pos[g] + j, cache [G, T, 2W], pos / live int32 [G].  Every row has the bits of
    attn_decode_rope on it alone at its position after the rows before it were appended; returns o [G*K, W] bf16."""
    _chk2d(qkv2d, BF16, "attn_decode_rope_draft.qkv")
    R, W, K = qkv2d.shape[0], n_heads * head_dim, int(K)
    G = cache.shape[0]
    if K < 1 or R != G * K or qkv2d.shape[1] < 3 * W or cache.shape[2] != 2 * W:
        raise _lib.MyriadHipError("attn_decode_rope_draft: qkv must be [G*K, >=3W] and cache [G, T, 2W]")
    for name, t in (("pos", pos), ("live", live)):
        if t.dtype != torch.int32 or t.numel() != G or not t.is_contiguous():
            raise _lib.MyriadHipError(f"attn_decode_rope_draft: {name} must be a contiguous int32 [G]")
    if out is None:
        out = torch.empty((R, W), dtype=BF16, device=qkv2d.device)
    elif out.dtype != BF16 or out.shape != (R, W) or out.stride(1) != 1:
        raise _lib.MyriadHipError("attn_decode_rope_draft: out must be bf16 [G*K, W]")
    _lib.check(_L().mh_attn_decode_rope_draft(_p(qkv2d), qkv2d.stride(0), _p(cache), cache.stride(0), cache.stride(1), _p(pos),
                                              _p(live), _p(cos_tab), _p(sin_tab), _p(out), out.stride(0), G, K, n_heads, head_dim,
                                              cache.shape[1], float(scale), _s()), "mh_attn_decode_rope_draft")
    return out


def draft_accept(nxt, margin, pmax, ids, top_p: torch.Tensor, rec, pos, kvlen, step_dev, K: int):
    """The end of a verify step over G = nxt.numel() / K sequences: rec[g] = (K ids, K margins, K p_max, n_out) as f32, where n_out
    = 1 + the leading guesses ids[1..] the picks confirm (with p_max >= top_p, a device float; <= 0: not looked at);
    ids[g*K] = the last accepted pick, pos[g] += n_out, kvlen[g] = pos[g] + 1, step += 1 -- all on the device."""
    K = int(K)
    G = nxt.numel() // K
    if K < 1 or nxt.numel() != G * K or ids.numel() < G * K or rec.numel() < G * (3 * K + 1) or pos.numel() < G or kvlen.numel() < G:
        raise _lib.MyriadHipError("draft_accept: nxt / margin / pmax / ids hold G*K rows, rec G*(3K+1) floats, pos / kvlen G ints")
    _lib.check(_L().mh_draft_accept(_p(nxt), _p(margin), _p(pmax), _p(ids), _p(top_p), _p(rec), _p(pos), _p(kvlen), _p(step_dev), G, K,
                                    _s()), "mh_draft_accept")


def attn_decode_rope_draft_rows(qkv2d: torch.Tensor, cache: torch.Tensor, pos: torch.Tensor, live: torch.Tensor, nrow: torch.Tensor,
                                cos_tab: torch.Tensor, sin_tab: torch.Tensor, n_heads: int, head_dim: int, scale: float, K: int,
                                out: Optional[torch.Tensor] = None):
    """attn_decode_rope_draft for the decode slots: group g holds nrow[g] token rows (int32 [G] on the device, 1 .. K).  Rows
    below nrow[g] of a live group have attn_decode_rope_draft's bits; the others, and every row of an idle group, touch neither q
    nor the cache and get a zero out row.  Returns o [G*K, W] bf16."""
    _chk2d(qkv2d, BF16, "attn_decode_rope_draft_rows.qkv")
    R, W, K = qkv2d.shape[0], n_heads * head_dim, int(K)
    G = cache.shape[0]
    if K < 1 or R != G * K or qkv2d.shape[1] < 3 * W or cache.shape[2] != 2 * W:
        raise _lib.MyriadHipError("attn_decode_rope_draft_rows: qkv must be [G*K, >=3W] and cache [G, T, 2W]")
    for name, t in (("pos", pos), ("live", live), ("nrow", nrow)):
        if t.dtype != torch.int32 or t.numel() != G or not t.is_contiguous():
            raise _lib.MyriadHipError(f"attn_decode_rope_draft_rows: {name} must be a contiguous int32 [G]")
    if out is None:
        out = torch.empty((R, W), dtype=BF16, device=qkv2d.device)
    elif out.dtype != BF16 or out.shape != (R, W) or out.stride(1) != 1:
        raise _lib.MyriadHipError("attn_decode_rope_draft_rows: out must be bf16 [G*K, W]")
    _lib.check(_L().mh_attn_decode_rope_draft_rows(_p(qkv2d), qkv2d.stride(0), _p(cache), cache.stride(0), cache.stride(1), _p(pos),
                                                   _p(live), _p(nrow), _p(cos_tab), _p(sin_tab), _p(out), out.stride(0), G, K,
                                                   n_heads, head_dim, cache.shape[1], float(scale), _s()),
               "mh_attn_decode_rope_draft_rows")
    return out


def draft_accept_rows(nxt, margin, pmax, ids_k, next_ids, nguess, live, top_p: torch.Tensor, rec, pos, kvlen, step_dev, K: int):
    """draft_accept per decode slot: group g has nguess[g] real guesses (int32 [G] on the device, 0 .. K - 1) and a flag live[g].
    A live group's rec[g] = (K ids, K margins, K p_max, n_out), ids_k[g*K] = next_ids[g] = the last kept pick, pos[g] += n_out,
    kvlen[g] = pos[g] + 1; an idle group records ids -1, zeros and n_out = 0 and keeps its state.  step += 1."""
    K = int(K)
    G = nxt.numel() // max(K, 1)
    if K >= 1 and (nxt.numel() != G * K or margin.numel() != G * K or pmax.numel() != G * K or ids_k.numel() < G * K
                   or next_ids.numel() < G or rec.numel() < G * (3 * K + 1) or pos.numel() < G or kvlen.numel() < G):
        raise _lib.MyriadHipError("draft_accept_rows: nxt / margin / pmax / ids_k hold G*K rows, rec G*(3K+1) floats, next_ids / "
                                  "pos / kvlen G entries")
    for name, t in (("nguess", nguess), ("live", live)):
        if t.dtype != torch.int32 or t.numel() < G or not t.is_contiguous():
            raise _lib.MyriadHipError(f"draft_accept_rows: {name} must be a contiguous int32 [G]")
    if nxt.dtype != torch.long or ids_k.dtype != torch.long or next_ids.dtype != torch.long:
        raise _lib.MyriadHipError("draft_accept_rows: nxt, ids_k and next_ids are int64")
    for name, t, dt in (("margin", margin, F32), ("pmax", pmax, F32), ("rec", rec, F32), ("top_p", top_p, F32), ("pos", pos, torch.int32),
                        ("kvlen", kvlen, torch.int32), ("step", step_dev, torch.int32), ("nxt", nxt, torch.long), ("ids_k", ids_k, torch.long),
                        ("next_ids", next_ids, torch.long)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() < 1:
            raise _lib.MyriadHipError(f"draft_accept_rows: {name} must be a contiguous {dt} tensor")
    _lib.check(_L().mh_draft_accept_rows(_p(nxt), _p(margin), _p(pmax), _p(ids_k), _p(next_ids), _p(nguess), _p(live), _p(top_p),
                                         _p(rec), _p(pos), _p(kvlen), _p(step_dev), G, K, _s()), "mh_draft_accept_rows")


def _draft_groups(name: str, K: int, rows: int, per_group, per_row=()):
    """The checks the three draft_sample.hip wrappers share: G from `rows` = G * K, contiguous int32 [>= G] per-group state and
    contiguous per-row buffers of G * K entries with their dtypes.  K outside 1 .. DRAFT_MAX_K goes to the launcher, which refuses
    it with nothing launched."""
    K = int(K)
    G = rows // max(K, 1)
    if K >= 1 and rows != G * K:
        raise _lib.MyriadHipError(f"{name}: {rows} rows are not G groups of K = {K}")
    for what, t in per_group:
        if t.dtype != torch.int32 or t.numel() < G or not t.is_contiguous():
            raise _lib.MyriadHipError(f"{name}: {what} must be a contiguous int32 [G]")
    for what, t, dt in per_row:
        if t is not None and (t.dtype != dt or t.numel() < rows or not t.is_contiguous()):
            raise _lib.MyriadHipError(f"{name}: {what} must be a contiguous {dt} tensor of G*K entries")
    return G, K


def _draft_logits(name: str, logits: torch.Tensor):
    if logits.dtype != F32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise _lib.MyriadHipError(f"{name}: logits must be f32 [G*K, V] with unit column stride")
    return logits.shape


def _draft_seen(name: str, seen, G: int, V: int):
    if seen.dtype != torch.int32 or not seen.is_contiguous() or seen.numel() < G * ((V + 31) // 32):
        raise _lib.MyriadHipError(f"{name}: seen must be a contiguous int32 [G, ceil(V / 32)] bitmap")


def repetition_penalty_draft_rows(logits: torch.Tensor, seen: torch.Tensor, ids_k: torch.Tensor, nrow: torch.Tensor,
                                  live: torch.Tensor, penalty: torch.Tensor, K: int):
    """The repetition penalty on the rows of a verify step, in place on f32 logits [G*K, V]: row (g, j) with live[g] and j <
    nrow[g] is penalised on every id of the bitmap seen[g] (int32 [G, ceil(V/32)], only read) and of ids_k[g*K .. g*K + j], each
    once -- what repetition_penalty_rows_slots leaves on that row with the earlier fed ids in its bitmap.  Other rows are left
    alone."""
    name = "repetition_penalty_draft_rows"
    R, V = _draft_logits(name, logits)
    G, K = _draft_groups(name, K, R, (("nrow", nrow), ("live", live)), (("ids_k", ids_k, torch.long),))
    _draft_seen(name, seen, G, V)
    if penalty.dtype != F32 or penalty.numel() < 1:
        raise _lib.MyriadHipError(f"{name}: penalty is a device f32 scalar")
    _lib.check(_L().mh_repetition_penalty_draft_rows(_p(logits), logits.stride(0), _p(seen), _p(ids_k), _p(nrow), _p(live), G, K, V,
                                                     _p(penalty), _s()), "mh_repetition_penalty_draft_rows")
    return logits


def sample_rows_draft(logits: torch.Tensor, out, margin_out, pmax_out, kept_out, params: torch.Tensor, seed, gen: torch.Tensor,
                      nrow: torch.Tensor, live: torch.Tensor, K: int, draw: bool, u_out=None):
    """sample_rows_slots (`draw`) / argmax_pmax_rows_slots (not `draw`) for the rows of a verify step: row (g, j) of f32 logits
    [G*K, V] reads seed[g] (int64 [G]) and t = gen[g] + j, bans eos_id while t < min_length, and has the slot entry's bits on that
    row alone at gen = t.  A row with live[g] == 0 or j >= nrow[g] gets out = -1, margin = p_max = 0, kept = 0.  Without the
    draw kept_out, u_out and seed are not touched (they may be None)."""
    name = "sample_rows_draft"
    R, V = _draft_logits(name, logits)
    G, K = _draft_groups(name, K, R, (("gen", gen), ("nrow", nrow), ("live", live)),
                         (("out", out, torch.long), ("margin", margin_out, F32), ("pmax", pmax_out, F32),
                          ("kept", kept_out, torch.int32), ("u_out", u_out, F32)))
    if params.dtype != F32 or params.numel() < 6 or not params.is_contiguous():
        raise _lib.MyriadHipError(f"{name}: params is f32 (inv_temp, top_p, top_k, penalty, min_length, eos_id)")
    if draw and (kept_out is None or seed is None or seed.dtype != torch.long or seed.numel() < G or not seed.is_contiguous()):
        raise _lib.MyriadHipError(f"{name}: the draw needs kept_out and a contiguous int64 seed [G]")
    _lib.check(_L().mh_sample_rows_draft(_p(logits), logits.stride(0), _p(out), _p(margin_out), _p(pmax_out), _p(kept_out), _p(u_out),
                                         G, K, V, _p(params), _p(seed), _p(gen), _p(nrow), _p(live), int(bool(draw)), _s()),
               "mh_sample_rows_draft")
    return out, kept_out


def draft_accept_sampled_rows(nxt, margin, pmax, kept, ids_k, next_ids, nguess, live, top_p: torch.Tensor, seen, rec, pos, kvlen,
                              gen, step_dev, K: int, V: int = 0):
    """draft_accept_rows with the sampler's kept counts, the seen-id bitmap and the per-request token count: a row with kept[j] <
    0 ends its group's chain (kept None: the p_max >= top_p rule); the fed token and the confirmed guesses join seen[g] (int32 [G,
    ceil(V/32)], None: no bitmap); gen[g] += n_out.  rec[g] = (K ids, K margins, K p_max, K kept, n_out) as f32."""
    name = "draft_accept_sampled_rows"
    G, K = _draft_groups(name, K, nxt.numel(), (("nguess", nguess), ("live", live), ("pos", pos), ("kvlen", kvlen), ("gen", gen)),
                         (("nxt", nxt, torch.long), ("margin", margin, F32), ("pmax", pmax, F32), ("kept", kept, torch.int32),
                          ("ids_k", ids_k, torch.long)))
    if next_ids.dtype != torch.long or next_ids.numel() < G or not next_ids.is_contiguous():
        raise _lib.MyriadHipError(f"{name}: next_ids must be a contiguous int64 [G]")
    if rec.dtype != F32 or not rec.is_contiguous() or rec.numel() < G * (4 * max(K, 0) + 1):
        raise _lib.MyriadHipError(f"{name}: rec holds G*(4K+1) contiguous f32")
    for what, t, dt in (("top_p", top_p, F32), ("step", step_dev, torch.int32)):
        if t.dtype != dt or t.numel() < 1:
            raise _lib.MyriadHipError(f"{name}: {what} must be a device {dt} scalar")
    if seen is not None:
        if int(V) < 1:
            raise _lib.MyriadHipError(f"{name}: the bitmap needs V")
        _draft_seen(name, seen, G, int(V))
    _lib.check(_L().mh_draft_accept_sampled_rows(_p(nxt), _p(margin), _p(pmax), _p(kept), _p(ids_k), _p(next_ids), _p(nguess),
                                                 _p(live), _p(top_p), _p(seen), _p(rec), _p(pos), _p(kvlen), _p(gen), _p(step_dev), G,
                                                 K, int(V), _s()), "mh_draft_accept_sampled_rows")


def _attn_prefill_ragged(sw: int, qkv2d, pos, seg, seg_host, cache, cos_tab, sin_tab, n_heads, head_dim, scale, out,
                         shared: bool = False):
    """attn_prefill_ragged (sw = 3 ints per segment), attn_prefill_ragged_past (sw = 4) and attn_prefill_ragged_shared (sw = 4,
    `shared`): one set of checks."""
    name_ = "attn_prefill_ragged" + (("_shared" if shared else "_past") if sw == 4 else "")
    _chk2d(qkv2d, BF16, name_ + ".qkv")
    M, W = qkv2d.shape[0], n_heads * head_dim
    if qkv2d.shape[1] < 3 * W:
        raise _lib.MyriadHipError(f"{name_}: qkv must be [M, >=3W], got {tuple(qkv2d.shape)} for W = {W}")
    if cache.dtype != BF16 or not cache.is_cuda or cache.dim() != 3 or cache.shape[2] != 2 * W or cache.stride(2) != 1:
        raise _lib.MyriadHipError(f"{name_}: cache must be a cuda bf16 [n_slots, T, 2W] with unit inner stride, got "
                                  f"{cache.dtype} {tuple(cache.shape)}")
    if pos.dtype != torch.int32 or not pos.is_cuda or pos.shape != (M,) or not pos.is_contiguous():
        raise _lib.MyriadHipError(f"{name_}: pos must be a contiguous cuda int32 [M]")
    for name, t, cuda in (("seg", seg, True), ("seg_host", seg_host, False)):
        if t.dtype != torch.int32 or t.is_cuda != cuda or t.dim() != 2 or t.shape[1] != sw or not t.is_contiguous():
            raise _lib.MyriadHipError(f"{name_}: {name} must be a contiguous {'cuda' if cuda else 'cpu'} int32 [R, {sw}]")
    if seg.shape != seg_host.shape:
        raise _lib.MyriadHipError(f"{name_}: seg and seg_host must hold the same table")
    for name, t in (("cos", cos_tab), ("sin", sin_tab)):
        if t.dtype != F32 or not t.is_cuda or t.dim() != 2 or t.shape[1] != head_dim // 2 or not t.is_contiguous():
            raise _lib.MyriadHipError(f"{name_}: {name} must be a contiguous cuda f32 [max_pos, D / 2]")
    if cos_tab.shape != sin_tab.shape:
        raise _lib.MyriadHipError(f"{name_}: cos and sin tables differ in shape")
    if out is None:
        out = torch.zeros((M, W), dtype=BF16, device=qkv2d.device)
    else:
        _chk2d(out, BF16, name_ + ".out")
        if out.shape != (M, W):
            raise _lib.MyriadHipError(f"{name_}: out shape {tuple(out.shape)} != {(M, W)}")
    R = seg_host.shape[0]
    fn = getattr(_L(), "mh_" + name_)
    _lib.check(fn(_p(qkv2d), qkv2d.stride(0), _p(pos), _p(seg), seg_host.data_ptr(), R, _p(cache), cache.stride(0), cache.stride(1),
                  cache.shape[0], cache.shape[1], _p(cos_tab), _p(sin_tab), cos_tab.shape[0], _p(out), out.stride(0), M, n_heads,
                  head_dim, float(scale), _s()), f"mh_{name_} M={M} R={R} H={n_heads} D={head_dim}")
    return out


def attn_prefill_ragged(qkv2d: torch.Tensor, pos: torch.Tensor, seg: torch.Tensor, seg_host: torch.Tensor, cache: torch.Tensor,
                        cos_tab: torch.Tensor, sin_tab: torch.Tensor, n_heads: int, head_dim: int, scale: float,
                        out: Optional[torch.Tensor] = None):
    """Packed prefill attention of several decode slots in one launch.  qkv2d [M, >=3W] bf16 = [q | k | v], pre-rotary and only
    read; pos int32 [M] the rotary position of each row; seg int32 [R, 3] on the device = (row0, len, slot) per segment and
    seg_host the same table on the CPU (the entry sizes its grid and validates by it); cache [n_slots, T, 2W].  Per segment:
    rope_ + copy3d_bf16 into cache[slot, :len] + attn_fwd(causal=True) on its rows as a B = 1 batch, same bits.  Returns
    o [M, W] bf16; rows outside every segment are not written (zeros when `out` is allocated here)."""
    return _attn_prefill_ragged(3, qkv2d, pos, seg, seg_host, cache, cos_tab, sin_tab, n_heads, head_dim, scale, out)


def attn_prefill_ragged_past(qkv2d: torch.Tensor, pos: torch.Tensor, seg: torch.Tensor, seg_host: torch.Tensor,
                             cache: torch.Tensor, cos_tab: torch.Tensor, sin_tab: torch.Tensor, n_heads: int, head_dim: int,
                             scale: float, out: Optional[torch.Tensor] = None):
    """attn_prefill_ragged on top of a cached prefix: seg / seg_host are int32 [R, 4] = (row0, len, slot, past) per segment, the
    segment's rows are the len NEW rows of a request whose keys 0 .. past - 1 are cache[slot]'s rows already.  Per segment:
    rope_ + copy3d_bf16 into cache[slot, past:past + len] + attn_fwd(causal=True) over the past + len keys, same bits; no cache
    row >= past is read, none outside [past, past + len) written.  With past = 0 everywhere it is attn_prefill_ragged's bits."""
    return _attn_prefill_ragged(4, qkv2d, pos, seg, seg_host, cache, cos_tab, sin_tab, n_heads, head_dim, scale, out)


def attn_prefill_ragged_shared(qkv2d: torch.Tensor, pos: torch.Tensor, seg: torch.Tensor, seg_host: torch.Tensor,
                               cache: torch.Tensor, cos_tab: torch.Tensor, sin_tab: torch.Tensor, n_heads: int, head_dim: int,
                               scale: float, out: Optional[torch.Tensor] = None):
    """attn_prefill_ragged_past for segments that continue the SAME cached prefix: the [R, 4] tables of (row0, len, slot, past),
    but several segments may name one slot (equal or different past, 0 included) and `cache` is only read -- rows < past of a
    named slot; no byte of it is written.  A segment's o rows have the bits attn_prefill_ragged_past gives it alone on a private
    copy of its slot."""
    return _attn_prefill_ragged(4, qkv2d, pos, seg, seg_host, cache, cos_tab, sin_tab, n_heads, head_dim, scale, out, shared=True)


# keys per workgroup of mh_attn_decode_rope_split: 128 measured fastest at 256 / 1,024 / 2,048 cached keys, batch 1, 32 heads
# (tools/chat_bench.py --chunks: 11.5 / 15.2 / 21.0 us per layer; 256 keys 16.0 / 17.8 / 22.2; 512 keys 19.9 / 27.0 / 30.6)
SPLIT_KV_CHUNK = 128


def attn_decode_split_ws(B: int, n_heads: int, T_cap: int, device, chunk: int = SPLIT_KV_CHUNK) -> torch.Tensor:
    """The fp32 partials buffer mh_attn_decode_rope_split needs for a [B, T_cap] cache (one (m, l, o) record per chunk)."""
    n = _L().mh_attn_decode_split_ws_floats(B, n_heads, T_cap, chunk)
    if n < 0:
        raise _lib.MyriadHipError(f"attn_decode_split_ws: bad shape B={B} H={n_heads} T_cap={T_cap} chunk={chunk}")
    return torch.empty((n,), dtype=F32, device=device)


def attn_decode_rope_split(qkv2d: torch.Tensor, cache: torch.Tensor, pos: torch.Tensor, pos_dev: torch.Tensor, kv_len: torch.Tensor,
                           cos_tab: torch.Tensor, sin_tab: torch.Tensor, n_heads: int, head_dim: int, scale: float,
                           partials: torch.Tensor, chunk: int = SPLIT_KV_CHUNK, out: Optional[torch.Tensor] = None):
    """attn_decode_rope with the keys split into chunks over many workgroups plus an in-order merge (two launches).  qkv2d is
    read only (q is rotated in registers); the appended cache row has attn_decode_rope's bits.  partials: attn_decode_split_ws()."""
    _chk2d(qkv2d, BF16, "attn_decode_rope_split.qkv")
    B, W = qkv2d.shape[0], n_heads * head_dim
    if qkv2d.shape[1] < 3 * W or cache.shape[2] != 2 * W:
        raise _lib.MyriadHipError("attn_decode_rope_split: qkv must be [B, >=3W] and cache [B, T, 2W]")
    if partials.dtype != F32 or not partials.is_contiguous():
        raise _lib.MyriadHipError("attn_decode_rope_split: partials must be a contiguous f32 buffer")
    if out is None:
        out = torch.empty((B, W), dtype=BF16, device=qkv2d.device)
    _lib.check(_L().mh_attn_decode_rope_split(_p(qkv2d), qkv2d.stride(0), _p(cache), cache.stride(0), cache.stride(1), _p(pos),
                                              _p(pos_dev), _p(kv_len), _p(cos_tab), _p(sin_tab), _p(out), out.stride(0), _p(partials),
                                              partials.numel(), B, n_heads, head_dim, cache.shape[1], int(chunk), float(scale), _s()),
               "mh_attn_decode_rope_split")
    return out


def attn_decode_rope_split_rows(qkv2d: torch.Tensor, cache: torch.Tensor, pos: torch.Tensor, kv_len: torch.Tensor, live: torch.Tensor,
                                cos_tab: torch.Tensor, sin_tab: torch.Tensor, n_heads: int, head_dim: int, scale: float,
                                partials: torch.Tensor, chunk: int = SPLIT_KV_CHUNK, out: Optional[torch.Tensor] = None):
    """attn_decode_rope_split with per-row state (decode slots): row b rotates and appends at pos[b], sees kv_len[b] keys; a row
    with live[b] == 0 (int32 [B]) touches neither qkv2d, the cache nor the partials and gets a zero row of o.  A live row has the
    bits of attn_decode_rope_split at B = 1 on that row.  qkv2d is read only (attn_decode_rope_rows rotates q in place, this
    does not).  partials: attn_decode_split_ws()."""
    _chk2d(qkv2d, BF16, "attn_decode_rope_split_rows.qkv")
    B, W = qkv2d.shape[0], n_heads * head_dim
    if qkv2d.shape[1] < 3 * W or cache.shape[2] != 2 * W or cache.shape[0] != B:
        raise _lib.MyriadHipError("attn_decode_rope_split_rows: qkv must be [B, >=3W] and cache [B, T, 2W]")
    for name, t in (("pos", pos), ("kv_len", kv_len), ("live", live)):
        if t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous():
            raise _lib.MyriadHipError(f"attn_decode_rope_split_rows: {name} must be a contiguous int32 [B]")
    if partials.dtype != F32 or not partials.is_contiguous():
        raise _lib.MyriadHipError("attn_decode_rope_split_rows: partials must be a contiguous f32 buffer")
    if out is None:
        out = torch.empty((B, W), dtype=BF16, device=qkv2d.device)
    _lib.check(_L().mh_attn_decode_rope_split_rows(_p(qkv2d), qkv2d.stride(0), _p(cache), cache.stride(0), cache.stride(1), _p(pos),
                                                   _p(kv_len), _p(live), _p(cos_tab), _p(sin_tab), _p(out), out.stride(0),
                                                   _p(partials), partials.numel(), B, n_heads, head_dim, cache.shape[1], int(chunk),
                                                   float(scale), _s()), "mh_attn_decode_rope_split_rows")
    return out


def attn_decode_split_draft_supported(n_heads: int, head_dim: int, K: int, T_cap: int, chunk: int = SPLIT_KV_CHUNK) -> bool:
    """Whether mh_attn_decode_rope_split_draft takes this shape (head dim, rows per sequence, cache length, chunk): the launcher's
    own answer to a call with no sequence, which launches nothing."""
    rc = _L().mh_attn_decode_rope_split_draft(None, 0, None, 0, 0, None, None, None, None, None, 0, None, 0, 0, int(K), int(n_heads),
                                              int(head_dim), int(T_cap), int(chunk), 1.0, _s())
    return rc == 0


def attn_decode_split_draft_ws(G: int, K: int, n_heads: int, T_cap: int, device, chunk: int = SPLIT_KV_CHUNK) -> torch.Tensor:
    """The fp32 partials buffer mh_attn_decode_rope_split_draft needs for G sequences of K rows on a [G, T_cap] cache."""
    n = _L().mh_attn_decode_split_draft_ws_floats(G, K, n_heads, T_cap, chunk)
    if n < 0:
        raise _lib.MyriadHipError(f"attn_decode_split_draft_ws: bad shape G={G} K={K} H={n_heads} T_cap={T_cap} chunk={chunk}")
    return torch.empty((n,), dtype=F32, device=device)


def _attn_decode_rope_split_draft(name, qkv2d, cache, pos, live, nrow, cos_tab, sin_tab, n_heads, head_dim, scale, K, partials, chunk,
                                  out):
    _chk2d(qkv2d, BF16, f"{name}.qkv")
    R, W, K = qkv2d.shape[0], n_heads * head_dim, int(K)
    G = cache.shape[0]
    if K < 1 or R != G * K or qkv2d.shape[1] < 3 * W or cache.shape[2] != 2 * W:
        raise _lib.MyriadHipError(f"{name}: qkv must be [G*K, >=3W] and cache [G, T, 2W]")
    for what, t in (("pos", pos), ("live", live)) + ((("nrow", nrow),) if nrow is not None else ()):
        if t.dtype != torch.int32 or t.numel() != G or not t.is_contiguous():
            raise _lib.MyriadHipError(f"{name}: {what} must be a contiguous int32 [G]")
    if partials.dtype != F32 or not partials.is_contiguous():
        raise _lib.MyriadHipError(f"{name}: partials must be a contiguous f32 buffer")
    if out is None:
        out = torch.empty((R, W), dtype=BF16, device=qkv2d.device)
    elif out.dtype != BF16 or out.shape != (R, W) or out.stride(1) != 1:
        raise _lib.MyriadHipError(f"{name}: out must be bf16 [G*K, W]")
    head = (_p(qkv2d), qkv2d.stride(0), _p(cache), cache.stride(0), cache.stride(1), _p(pos), _p(live))
    tail = (_p(cos_tab), _p(sin_tab), _p(out), out.stride(0), _p(partials), partials.numel(), G, K, n_heads, head_dim, cache.shape[1],
            int(chunk), float(scale), _s())
    if nrow is None:
        _lib.check(_L().mh_attn_decode_rope_split_draft(*head, *tail), "mh_attn_decode_rope_split_draft")
    else:
        _lib.check(_L().mh_attn_decode_rope_split_draft_rows(*head, _p(nrow), *tail), "mh_attn_decode_rope_split_draft_rows")
    return out


def attn_decode_rope_split_draft(qkv2d: torch.Tensor, cache: torch.Tensor, pos: torch.Tensor, live: torch.Tensor, cos_tab: torch.Tensor,
                                 sin_tab: torch.Tensor, n_heads: int, head_dim: int, scale: float, K: int, partials: torch.Tensor,
                                 chunk: int = SPLIT_KV_CHUNK, out: Optional[torch.Tensor] = None):
    """K consecutive split-KV token steps of each of G sequences as one launch pair (the verify step on the split-KV view): row
    g*K + j of qkv2d [G*K, >=3W] is the token at position pos[g] + j, cache [G, T, 2W], pos / live int32 [G].  Every out row and
    appended cache row has the bits of attn_decode_rope_split_rows at B = 1 on that row at its position after the rows before it
    were appended; every cached key is loaded once for the K queries.  qkv2d is read only.  partials:
    attn_decode_split_draft_ws().  Returns o [G*K, W] bf16."""
    return _attn_decode_rope_split_draft("attn_decode_rope_split_draft", qkv2d, cache, pos, live, None, cos_tab, sin_tab, n_heads,
                                         head_dim, scale, K, partials, chunk, out)


def attn_decode_rope_split_draft_rows(qkv2d: torch.Tensor, cache: torch.Tensor, pos: torch.Tensor, live: torch.Tensor,
                                      nrow: torch.Tensor, cos_tab: torch.Tensor, sin_tab: torch.Tensor, n_heads: int, head_dim: int,
                                      scale: float, K: int, partials: torch.Tensor, chunk: int = SPLIT_KV_CHUNK,
                                      out: Optional[torch.Tensor] = None):
    """attn_decode_rope_split_draft for the decode slots: group g holds nrow[g] token rows (int32 [G] on the device, 1 .. K).
    Rows below nrow[g] of a live group have attn_decode_rope_split_draft's bits; the others, and every row of an idle group, write
    neither the cache nor a partial record and get a zero out row."""
    if nrow is None:
        raise _lib.MyriadHipError("attn_decode_rope_split_draft_rows: nrow must be a contiguous int32 [G]")
    return _attn_decode_rope_split_draft("attn_decode_rope_split_draft_rows", qkv2d, cache, pos, live, nrow, cos_tab, sin_tab, n_heads,
                                         head_dim, scale, K, partials, chunk, out)


def gemm_auto_f32(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """f32 out = a @ b^T, choosing split-K when the output is small and the reduction long (wgrad shapes)."""
    M, K = a.shape
    N = b.shape[0]
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    kt = K // 64
    if tiles >= 128 or kt < 16:
        return gemm(a, b, out=out)
    splits = max(1, min(kt // 4, 512 // tiles))
    ws = torch.empty((_L().mh_gemm_splitk_ws_floats(M, N, splits),), dtype=F32, device=a.device)
    rc = _L().mh_gemm_bf16_nt_splitk(_p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N, K, splits,
                                     _p(ws), _s())
    _lib.check(rc, f"mh_gemm_bf16_nt_splitk M={M} N={N} K={K} splits={splits}")
    return out


# --------------------------------------------------------------------------- attention
def _attn_fwd_outputs(name, q, k, v, H, D, out=None, need_lse=True):
    """The forward pair's q / k / v check and its (o, lse) allocation."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        if t.dtype != BF16 or t.stride(2) != 1:
            raise _lib.MyriadHipError(f"{name}.{n}: need bf16 with unit inner stride")
    B, Sq = q.shape[0], q.shape[1]
    if out is None:
        out = torch.empty((B, Sq, H * D), dtype=BF16, device=q.device)
    return out, (torch.empty((B, H, Sq), dtype=F32, device=q.device) if need_lse else None)


def _attn_bwd_outputs(q, k, H, D, dq, dk, dv):
    """The backward pair's (dq, dk, dv, delta): the gradients the caller did not pass, and the delta scratch."""
    B, Sq, Sk, dev = q.shape[0], q.shape[1], k.shape[1], q.device
    if dq is None:
        dq = torch.empty((B, Sq, H * D), dtype=BF16, device=dev)
    if dk is None:
        dk = torch.empty((B, Sk, H * D), dtype=BF16, device=dev)
    if dv is None:
        dv = torch.empty((B, Sk, H * D), dtype=BF16, device=dev)
    return dq, dk, dv, torch.empty((B, H, Sq), dtype=F32, device=dev)


def _strides(*ts):
    """(batch stride, token stride) of each tensor, flattened: the order the attention entries take them in."""
    return [t.stride(i) for t in ts for i in (0, 1)]


def attn_fwd(q, k, v, H: int, D: int, scale: float, causal: bool = False, bias=None, kv_len=None, out=None,
             need_lse: bool = True):
    """q [B,Sq,Wq], k/v [B,Sk,W*] bf16 views (head h at cols h*D..), returns (o [B,Sq,H*D] bf16, lse [B,H,Sq] f32)."""
    B, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    out, lse = _attn_fwd_outputs("attn_fwd", q, k, v, H, D, out, need_lse)
    rc = _L().mh_attn_fwd(_p(q), _p(k), _p(v), _p(out), _p(lse), _p(bias), _p(kv_len), B, H, Sq, Sk, D,
                          *_strides(q, k, v, out), float(scale), int(causal), _s())
    _lib.check(rc, f"mh_attn_fwd B={B} H={H} Sq={Sq} Sk={Sk} D={D}")
    return out, lse


def attn_fwd_dropout(q, k, v, H: int, D: int, scale: float, p: float, seed: int):
    """attn_fwd with attention-probability dropout (mask index ((b*H + h)*Sq + i)*Sk + j); p = 0 is attn_fwd itself."""
    if p == 0.0:
        return attn_fwd(q, k, v, H, D, scale)
    B, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    out, lse = _attn_fwd_outputs("attn_fwd_dropout", q, k, v, H, D)
    rc = _L().mh_attn_fwd_dropout(_p(q), _p(k), _p(v), _p(out), _p(lse), B, H, Sq, Sk, D, *_strides(q, k, v, out),
                                  float(scale), float(p), int(seed), _s())
    _lib.check(rc, f"mh_attn_fwd_dropout B={B} H={H} Sq={Sq} Sk={Sk} D={D}")
    return out, lse


def attn_bwd_dropout(q, k, v, o, dout, lse, H: int, D: int, scale: float, p: float, seed: int, dq=None, dk=None, dv=None):
    """attn_bwd of attn_fwd_dropout (o = its dropped output); p = 0 is attn_bwd itself."""
    if p == 0.0:
        return attn_bwd(q, k, v, o, dout, lse, H, D, scale, dq=dq, dk=dk, dv=dv)
    B, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    dq, dk, dv, delta = _attn_bwd_outputs(q, k, H, D, dq, dk, dv)
    rc = _L().mh_attn_bwd_dropout(_p(q), _p(k), _p(v), _p(o), _p(dout), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv),
                                  B, H, Sq, Sk, D, *_strides(q, k, v, o, dout, dq, dk, dv), float(scale), float(p), int(seed),
                                  _s())
    _lib.check(rc, f"mh_attn_bwd_dropout B={B} H={H} Sq={Sq} Sk={Sk} D={D}")
    return dq, dk, dv


def attn_bwd(q, k, v, o, dout, lse, H: int, D: int, scale: float, causal: bool = False, bias=None, kv_len=None,
             dq=None, dk=None, dv=None):
    B, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    dq, dk, dv, delta = _attn_bwd_outputs(q, k, H, D, dq, dk, dv)
    rc = _L().mh_attn_bwd(_p(q), _p(k), _p(v), _p(o), _p(dout), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), _p(bias),
                          _p(kv_len), B, H, Sq, Sk, D, *_strides(q, k, v, o, dout, dq, dk, dv), float(scale), int(causal),
                          _s())
    _lib.check(rc, f"mh_attn_bwd B={B} H={H} Sq={Sq} Sk={Sk} D={D}")
    return dq, dk, dv


def attn_rope_supported(S: int, D: int) -> bool:
    """Whether the whole-sequence fused rotary attention (mh_attn_rope_*) covers this shape."""
    return bool(_L().mh_attn_rope_supported(int(S), int(D)))


def _chk_qkv3(qkv3, H, D, name):
    if qkv3.dtype != BF16 or qkv3.dim() != 3 or qkv3.stride(2) != 1 or qkv3.stride(0) != qkv3.shape[1] * qkv3.stride(1):
        raise _lib.MyriadHipError(f"{name}: need bf16 [B, S, >=3*H*D] with unit inner stride and dense batches")
    if qkv3.shape[2] < 3 * H * D:
        raise _lib.MyriadHipError(f"{name}: last dim {qkv3.shape[2]} < 3*H*D")


def attn_rope_fwd(qkv3: torch.Tensor, H: int, D: int, scale: float, pos, cos, sin, kv_len=None, need_lse: bool = True):
    """LLaMA causal self-attention with rotary applied on load.  qkv3 [B, S, >=3W] bf16 = [q | k | v], PRE-rotary.
    Returns (o [B, S, W] bf16, lse [B, H, S] f32)."""
    _chk_qkv3(qkv3, H, D, "attn_rope_fwd")
    B, S = qkv3.shape[0], qkv3.shape[1]
    o = torch.empty((B, S, H * D), dtype=BF16, device=qkv3.device)
    lse = torch.empty((B, H, S), dtype=F32, device=qkv3.device) if need_lse else None
    rc = _L().mh_attn_rope_fwd(_p(qkv3), qkv3.stride(1), _p(o), o.stride(1), _p(lse), _p(pos), _p(cos), _p(sin), _p(kv_len),
                               B, H, S, D, float(scale), _s())
    _lib.check(rc, f"mh_attn_rope_fwd B={B} H={H} S={S} D={D}")
    return o, lse


def attn_rope_bwd(qkv3, o, dout, lse, H: int, D: int, scale: float, pos, cos, sin, kv_len=None, dqkv=None):
    """Backward of attn_rope_fwd: dqkv [B, S, ld] = [dq | dk | dv] (dq, dk un-rotated).  dout [B*S or B,S, W] bf16."""
    _chk_qkv3(qkv3, H, D, "attn_rope_bwd")
    B, S = qkv3.shape[0], qkv3.shape[1]
    if dqkv is None:
        dqkv = torch.empty_like(qkv3)
    d2 = dout.reshape(B * S, -1)
    _chk2d(d2, BF16, "attn_rope_bwd.dout")
    rc = _L().mh_attn_rope_bwd(_p(qkv3), qkv3.stride(1), _p(o), o.stride(1), _p(d2), d2.stride(0), _p(lse), _p(dqkv),
                               _p(pos), _p(cos), _p(sin), _p(kv_len), B, H, S, D, float(scale), _s())
    _lib.check(rc, f"mh_attn_rope_bwd B={B} H={H} S={S} D={D}")
    return dqkv


def gemm_attn_rope_bwd(a, bw, qkv3, o, lse, H: int, D: int, scale: float, pos, cos, sin, kv_len=None, dqkv=None):
    """dO = a @ bw^T (the o_proj dgrad) and the fused rotary attention backward that consumes it; when the GEMM policy
    splits K the attention kernel sums the partial slabs itself.  Same bits as gemm() + attn_rope_bwd()."""
    _chk_qkv3(qkv3, H, D, "gemm_attn_rope_bwd")
    _chk2d(a, BF16, "gemm_attn_rope_bwd.a")
    _chk2d(bw, BF16, "gemm_attn_rope_bwd.bw")
    B, S = qkv3.shape[0], qkv3.shape[1]
    M, K = a.shape
    if M != B * S or bw.shape != (H * D, K):
        raise _lib.MyriadHipError(f"gemm_attn_rope_bwd: a {tuple(a.shape)} bw {tuple(bw.shape)} vs B*S={B * S} W={H * D}")
    if dqkv is None:
        dqkv = torch.empty_like(qkv3)
    do_buf = torch.empty((M, H * D), dtype=BF16, device=a.device)
    rc = _L().mh_gemm_attn_rope_bwd(_p(a), a.stride(0), _p(bw), bw.stride(0), _p(do_buf), K, _p(qkv3), qkv3.stride(1), _p(o),
                                    o.stride(1), _p(lse), _p(dqkv), _p(pos), _p(cos), _p(sin), _p(kv_len), B, H, S, D,
                                    float(scale), _s())
    _lib.check(rc, f"mh_gemm_attn_rope_bwd M={M} K={K} H={H} S={S}")
    return dqkv


# --------------------------------------------------------------------------- norms
def rmsnorm_fwd(x: torch.Tensor, w: torch.Tensor, eps: float, out=None):
    """out may be a [M, D] view of a wider bf16 buffer (row stride >= D)."""
    M, D = x.shape
    if out is None:
        out = torch.empty((M, D), dtype=BF16, device=x.device)
    _lib.check(_L().mh_rmsnorm_fwd(_p(x), _p(w), _p(out), out.stride(0), M, D, float(eps), _s()), "mh_rmsnorm_fwd")
    return out


def dropout_bf16(x2d: torch.Tensor, p: float, seed: int):
    """x2d: [rows, cols] bf16 (row stride free).  Returns a contiguous masked/rescaled copy."""
    rows, cols = x2d.shape
    y = torch.empty((rows, cols), dtype=BF16, device=x2d.device)
    _lib.check(_L().mh_dropout_bf16(_p(x2d), x2d.stride(0), _p(y), cols, rows, cols, float(p),
                                    int(seed) & 0xFFFFFFFFFFFFFFFF, _s()), "mh_dropout_bf16")
    return y


def dropout_add_(dy2d: torch.Tensor, acc2d: torch.Tensor, p: float, seed: int):
    rows, cols = dy2d.shape
    _lib.check(_L().mh_dropout_add_f32(_p(dy2d), dy2d.stride(0), _p(acc2d), acc2d.stride(0), rows, cols, float(p),
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, _s()), "mh_dropout_add_f32")
    return acc2d


def rmsnorm_bwd(dy, x, w, eps: float, dres=None, want_f32=True, want_bf16=False):
    M, D = x.shape
    dx = torch.empty((M, D), dtype=F32, device=x.device) if want_f32 else None
    dxb = torch.empty((M, D), dtype=BF16, device=x.device) if want_bf16 else None
    _lib.check(_L().mh_rmsnorm_bwd(_p(dy), _p(x), _p(w), _p(dres), _p(dx), _p(dxb), M, D, float(eps), _s()),
               "mh_rmsnorm_bwd")
    return dx, dxb


def gemm_rmsnorm_bwd(a, b, x, w, eps: float, dres=None, want_f32=True, want_bf16=True):
    """dY = a @ b^T (f32), then rmsnorm_bwd(dY, x, w) + dres -> (dx f32, dx bf16): a dgrad Linear and the norm backward that
    reads it, with the split-K partials summed inside the norm kernel.  Same bits as gemm(out f32) + rmsnorm_bwd."""
    _chk2d(a, BF16, "gemm_rmsnorm_bwd.a")
    _chk2d(b, BF16, "gemm_rmsnorm_bwd.b")
    M, K = a.shape
    N = b.shape[0]
    if x.shape != (M, N) or b.shape[1] != K:
        raise _lib.MyriadHipError(f"gemm_rmsnorm_bwd: a {tuple(a.shape)} b {tuple(b.shape)} x {tuple(x.shape)}")
    dy = torch.empty((M, N), dtype=F32, device=a.device)
    dx = torch.empty((M, N), dtype=F32, device=a.device) if want_f32 else None
    dxb = torch.empty((M, N), dtype=BF16, device=a.device) if want_bf16 else None
    rc = _L().mh_gemm_rmsnorm_bwd(_p(a), a.stride(0), _p(b), b.stride(0), _p(dy), _p(x), _p(w), _p(dres), _p(dx), _p(dxb),
                                  M, N, K, float(eps), _s())
    _lib.check(rc, f"mh_gemm_rmsnorm_bwd M={M} N={N} K={K}")
    return dx, dxb


def gemm_layernorm_bwd(a, b, x, w, eps: float, dres=None, want_f32=True, want_bf16=True, dgamma=None, dbeta=None,
                       accumulate: bool = False):
    """dY = a @ b^T (f32), then layernorm_bwd(dY, x, w) + dres -> (dx f32, dx bf16); with dgamma / dbeta (f32 [N]) also the
    LayerNorm's parameter gradients ((+)= when accumulate).  The split-K partials are summed inside the norm kernel.  Same bits
    as gemm(out f32) + layernorm_bwd (+ layernorm_param_grads)."""
    _chk2d(a, BF16, "gemm_layernorm_bwd.a")
    _chk2d(b, BF16, "gemm_layernorm_bwd.b")
    M, K = a.shape
    N = b.shape[0]
    if x.shape != (M, N) or b.shape[1] != K or x.dtype != F32 or not x.is_contiguous():
        raise _lib.MyriadHipError(f"gemm_layernorm_bwd: a {tuple(a.shape)} b {tuple(b.shape)} x {tuple(x.shape)}")
    if w.dtype != F32 or w.numel() != N or not w.is_contiguous() or w.device != a.device:
        raise ValueError("gemm_layernorm_bwd: w must be contiguous f32 [N] on a's device")
    if (dgamma is None) != (dbeta is None):
        raise ValueError("gemm_layernorm_bwd: dgamma and dbeta go together")
    if dgamma is not None and (dgamma.dtype != F32 or dbeta.dtype != F32 or dgamma.numel() != N or dbeta.numel() != N
                               or not dgamma.is_contiguous() or not dbeta.is_contiguous()):
        raise ValueError("gemm_layernorm_bwd: dgamma / dbeta must be contiguous f32 [N]")
    if dres is not None and (dres.shape != (M, N) or dres.dtype != F32 or not dres.is_contiguous()):
        raise ValueError("gemm_layernorm_bwd: dres must be contiguous f32 [M, N]")
    L = _L()
    dy = torch.empty((M, N), dtype=F32, device=a.device)
    dx = torch.empty((M, N), dtype=F32, device=a.device) if want_f32 else None
    dxb = torch.empty((M, N), dtype=BF16, device=a.device) if want_bf16 else None
    n = L.mh_layernorm_param_grads_ws_floats(M, N) if dgamma is not None else 0
    ws = torch.empty((max(n, 1),), dtype=F32, device=a.device) if dgamma is not None else None
    rc = L.mh_gemm_layernorm_bwd(_p(a), a.stride(0), _p(b), b.stride(0), _p(dy), _p(x), _p(w), _p(dres), _p(dx), _p(dxb),
                                 _p(dgamma), _p(dbeta), int(accumulate), _p(ws), n, M, N, K, float(eps), _s())
    _lib.check(rc, f"mh_gemm_layernorm_bwd M={M} N={N} K={K}")
    return dx, dxb


def layernorm_fwd(x, w, b, eps: float, want_bf16=True, want_f32=False):
    M, D = x.shape
    yb = torch.empty((M, D), dtype=BF16, device=x.device) if want_bf16 else None
    yf = torch.empty((M, D), dtype=F32, device=x.device) if want_f32 else None
    _lib.check(_L().mh_layernorm_fwd(_p(x), _p(w), _p(b), _p(yb), _p(yf), M, D, float(eps), _s()), "mh_layernorm_fwd")
    return yb, yf


def layernorm_bwd(dy, x, w, eps: float, dres=None, want_f32=True, want_bf16=False):
    M, D = x.shape
    dx = torch.empty((M, D), dtype=F32, device=x.device) if want_f32 else None
    dxb = torch.empty((M, D), dtype=BF16, device=x.device) if want_bf16 else None
    _lib.check(_L().mh_layernorm_bwd(_p(dy), _p(x), _p(w), _p(dres), _p(dx), _p(dxb), M, D, float(eps), _s()),
               "mh_layernorm_bwd")
    return dx, dxb


def layernorm_param_grads(dy, x, eps: float, dgamma: torch.Tensor, dbeta: torch.Tensor, accumulate: bool = False,
                          p_out: float = 0.0, seed_out: int = 0):
    """dgamma (+)= sum_m dy * xhat(x), dbeta (+)= sum_m dy: the LayerNorm's parameter gradients (x = its f32 input).
    p_out > 0: the LayerNorm's output went through dropout (mask seed_out), dy is the gradient after it."""
    M, D = x.shape
    _chk2d(dy, F32, "dy")
    _chk2d(x, F32, "x")
    if dy.shape != x.shape or dy.stride(0) != D or x.stride(0) != D:
        raise ValueError("layernorm_param_grads: dy and x must be contiguous [M, D]")
    if dgamma.dtype != F32 or dbeta.dtype != F32 or dgamma.numel() != D or dbeta.numel() != D:
        raise ValueError("layernorm_param_grads: dgamma / dbeta must be f32 [D]")
    n = _L().mh_layernorm_param_grads_ws_floats(M, D)
    ws = torch.empty((max(n, 1),), dtype=F32, device=x.device)
    _lib.check(_L().mh_layernorm_param_grads(_p(dy), _p(x), _p(dgamma), _p(dbeta), M, D, float(eps), int(accumulate),
                                             float(p_out), int(seed_out), _p(ws), n, _s()), "mh_layernorm_param_grads")
    return dgamma, dbeta


def layernorm_fwd_dropout(z, res, w, b, eps: float, p_in: float = 0.0, seed_in: int = 0, p_out: float = 0.0,
                          seed_out: int = 0, want_bf16=True, want_f32=True):
    """Hidden dropout fused into a LayerNorm: x = dropout(z) + res (res given; x returned, the backward's input) or x = z;
    y = dropout(LN(x)).  Returns (x or None, y bf16, y f32)."""
    M, D = z.shape
    x = torch.empty((M, D), dtype=F32, device=z.device) if res is not None else None
    yb = torch.empty((M, D), dtype=BF16, device=z.device) if want_bf16 else None
    yf = torch.empty((M, D), dtype=F32, device=z.device) if want_f32 else None
    _lib.check(_L().mh_layernorm_fwd_dropout(_p(z), _p(res), _p(w), _p(b), _p(x), _p(yb), _p(yf), M, D, float(eps),
                                             float(p_in), int(seed_in), float(p_out), int(seed_out), _s()),
               "mh_layernorm_fwd_dropout")
    return x, yb, yf


def layernorm_bwd_dropout(dy, x, w, eps: float, p_in: float = 0.0, seed_in: int = 0, p_out: float = 0.0, seed_out: int = 0,
                          want_bf16=True):
    """Backward of layernorm_fwd_dropout: (dL/dx f32 -- the residual's gradient --, dL/dz = dL/dx * mask_in as bf16)."""
    M, D = x.shape
    dx = torch.empty((M, D), dtype=F32, device=x.device)
    dzb = torch.empty((M, D), dtype=BF16, device=x.device) if want_bf16 else None
    _lib.check(_L().mh_layernorm_bwd_dropout(_p(dy), _p(x), _p(w), _p(dx), _p(dzb), M, D, float(eps), float(p_in),
                                             int(seed_in), float(p_out), int(seed_out), _s()), "mh_layernorm_bwd_dropout")
    return dx, dzb


# --------------------------------------------------------------------------- stochastic depth (drop_path.hip)
DROP_PATH_MAX_B = 64


class DropPathMap:
    """The kept samples of one branch: slot[b] = compact sample index of sample b, or -1 (a host int32 array; the launchers read
    it on the host and pass it in the kernel arguments).  Built from a per-sample keep sequence (`from_keep`) or from an explicit
    slot list, which is checked: every entry -1 or in [0, K), the kept entries numbering 0 .. K-1 exactly once each."""

    def __init__(self, slot):
        if isinstance(slot, torch.Tensor):
            if slot.is_cuda or slot.dim() != 1 or slot.dtype not in (torch.int32, torch.int64):
                raise ValueError("DropPathMap: slot must be a 1-D host integer tensor")
            slot = slot.tolist()
        slot = list(slot)
        if not all(isinstance(v, numbers.Integral) and not isinstance(v, bool) for v in slot):
            raise ValueError("DropPathMap: slot entries must be integers")
        B = len(slot)
        if not 1 <= B <= DROP_PATH_MAX_B:
            raise ValueError(f"DropPathMap: {B} samples (1 .. {DROP_PATH_MAX_B} supported)")
        kept = [int(v) for v in slot if v >= 0]
        K = len(kept)
        if any(v < -1 or v >= B for v in slot):
            raise ValueError(f"DropPathMap: slot {slot}: entries must be -1 or in [0, {B})")
        if sorted(kept) != list(range(K)):
            raise ValueError(f"DropPathMap: slot {slot}: the kept samples must number 0 .. {K - 1}, each once")
        self.B, self.K = B, K
        self.slot = torch.tensor([int(v) for v in slot], dtype=torch.int32)
        self.samples = [b for _, b in sorted((v, b) for b, v in enumerate(slot) if v >= 0)]    # compact index -> sample

    @classmethod
    def from_keep(cls, keep) -> "DropPathMap":
        keep = [bool(k) for k in (keep.tolist() if isinstance(keep, torch.Tensor) else keep)]
        n, slot = 0, []
        for k in keep:
            slot.append(n if k else -1)
            n += int(k)
        return cls(slot)

    @property
    def full(self) -> bool:
        return self.K == self.B

    def ptr(self) -> int:
        return self.slot.data_ptr()


def _dp_map(m, B: int, name: str) -> DropPathMap:
    if not isinstance(m, DropPathMap):
        m = DropPathMap(m)
    if m.B != B:
        raise ValueError(f"{name}: the map covers {m.B} samples, the batch has {B}")
    return m


def _dp_dense(t, dtype, rows: int, D: int, name: str):
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or t.dim() != 2 or tuple(t.shape) != (rows, D)
            or not t.is_contiguous()):
        raise ValueError(f"{name}: need a contiguous device {dtype} [{rows}, {D}], got "
                         f"{(t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t)}")


def _dp_vec(t, D: int, name: str):
    if not isinstance(t, torch.Tensor) or t.dtype != F32 or not t.is_cuda or t.numel() != D or not t.is_contiguous():
        raise ValueError(f"{name}: need a contiguous device f32 [{D}]")


def _dp_dims(B: int, N: int, D: int, name: str, max_d: int = 8192):
    if N < 1 or D < 4 or D % 4 or D > max_d:
        raise ValueError(f"{name}: N = {N}, D = {D} (N >= 1, D a multiple of 4, D <= {max_d})")


def drop_path_residual_layernorm(h: torch.Tensor, y: Optional[torch.Tensor], keep_in, scale: float, N: int,
                                 w: Optional[torch.Tensor] = None, b: Optional[torch.Tensor] = None, eps: float = 1e-6,
                                 keep_out=None, want_h: bool = True):
    """Stochastic depth, forward (mh_drop_path_residual_layernorm).  h [B*N, D] f32: the residual stream; y [K_in*N, D] f32: the
    branch's output on the kept samples of `keep_in` (a DropPathMap or a slot list), or None = no branch (then keep_in is None).
    Returns (h_out, xn): h_out = h + scale * y on kept samples, h's bits on the others (None when want_h is False, which needs
    y None: h itself is the stream); xn = LayerNorm(h_out; w, b) in bf16 for the samples of `keep_out` ([K_out*N, D], compact;
    keep_out None = all of them), or None when w is None.  Every argument is checked before the launch (ValueError)."""
    if not isinstance(h, torch.Tensor) or h.dim() != 2 or N < 1 or h.shape[0] % N:
        raise ValueError("drop_path_residual_layernorm: h must be [B*N, D]")
    M, D = h.shape
    B = M // N
    _dp_dims(B, N, D, "drop_path_residual_layernorm")
    _dp_dense(h, F32, M, D, "drop_path_residual_layernorm.h")
    if not 1 <= B <= DROP_PATH_MAX_B:
        raise ValueError(f"drop_path_residual_layernorm: {B} samples (1 .. {DROP_PATH_MAX_B} supported)")
    m_in = m_out = None
    if y is not None:
        m_in = _dp_map(keep_in, B, "drop_path_residual_layernorm.keep_in")
        if m_in.K < 1:
            raise ValueError("drop_path_residual_layernorm: a branch that keeps nothing has no y (pass y=None)")
        _dp_dense(y, F32, m_in.K * N, D, "drop_path_residual_layernorm.y")
        if not want_h:
            raise ValueError("drop_path_residual_layernorm: a branch output needs h_out")
    elif keep_in is not None:
        raise ValueError("drop_path_residual_layernorm: keep_in without y")
    if (w is None) != (b is None):
        raise ValueError("drop_path_residual_layernorm: w and b go together")
    if w is not None:
        _dp_vec(w, D, "drop_path_residual_layernorm.w")
        _dp_vec(b, D, "drop_path_residual_layernorm.b")
        if keep_out is not None:
            m_out = _dp_map(keep_out, B, "drop_path_residual_layernorm.keep_out")
            if m_out.K < 1:
                raise ValueError("drop_path_residual_layernorm: keep_out keeps nothing (pass w=None)")
    elif keep_out is not None:
        raise ValueError("drop_path_residual_layernorm: keep_out without a norm")
    if w is None and not (want_h and y is not None):
        raise ValueError("drop_path_residual_layernorm: nothing to compute")
    K_out = 0 if w is None else (B if m_out is None else m_out.K)
    want_h = want_h and y is not None
    h_out = torch.empty((M, D), dtype=F32, device=h.device) if want_h else None
    xn = torch.empty((K_out * N, D), dtype=BF16, device=h.device) if w is not None else None
    rc = _L().mh_drop_path_residual_layernorm(_p(h), _p(y), m_in.ptr() if m_in else None, m_in.K if m_in else 0, float(scale),
                                              _p(w), _p(b), m_out.ptr() if m_out else None, K_out, _p(h_out), _p(xn), B, N, D,
                                              float(eps), _s())
    _lib.check(rc, "mh_drop_path_residual_layernorm")
    return h_out, xn


def drop_path_layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, eps: float, dres: torch.Tensor, keep_in, N: int,
                            keep_out=None, out_scale: float = 1.0, want_bf16: bool = True):
    """Stochastic depth, backward (mh_drop_path_layernorm_bwd).  dy [K_in*N, D] f32: the branch's dgrad on its kept samples
    (`keep_in`); x [B*N, D] f32: the LayerNorm's input; dres [B*N, D] f32: the residual gradient.  Returns (dx f32 [B*N, D],
    dx_bf16): dx = dres + LayerNorm backward on kept samples, dres's bits on the others; dx_bf16 = bf16(out_scale * dx) of the
    samples of `keep_out` ([K_out*N, D]; None = all).  Checked before the launch (ValueError)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or N < 1 or x.shape[0] % N:
        raise ValueError("drop_path_layernorm_bwd: x must be [B*N, D]")
    M, D = x.shape
    B = M // N
    _dp_dims(B, N, D, "drop_path_layernorm_bwd")
    m_in = _dp_map(keep_in, B, "drop_path_layernorm_bwd.keep_in")
    if m_in.K < 1:
        raise ValueError("drop_path_layernorm_bwd: a branch that keeps nothing has no backward")
    _dp_dense(x, F32, M, D, "drop_path_layernorm_bwd.x")
    _dp_dense(dres, F32, M, D, "drop_path_layernorm_bwd.dres")
    _dp_dense(dy, F32, m_in.K * N, D, "drop_path_layernorm_bwd.dy")
    _dp_vec(w, D, "drop_path_layernorm_bwd.w")
    m_out = None
    if keep_out is not None:
        if not want_bf16:
            raise ValueError("drop_path_layernorm_bwd: keep_out without the bf16 output")
        m_out = _dp_map(keep_out, B, "drop_path_layernorm_bwd.keep_out")
        if m_out.K < 1:
            raise ValueError("drop_path_layernorm_bwd: keep_out keeps nothing (pass want_bf16=False)")
    K_out = 0 if not want_bf16 else (B if m_out is None else m_out.K)
    dx = torch.empty((M, D), dtype=F32, device=x.device)
    dxb = torch.empty((K_out * N, D), dtype=BF16, device=x.device) if want_bf16 else None
    rc = _L().mh_drop_path_layernorm_bwd(_p(dy), _p(x), _p(w), _p(dres), m_in.ptr(), m_in.K, m_out.ptr() if m_out else None,
                                         K_out, float(out_scale), _p(dx), _p(dxb), B, N, D, float(eps), _s())
    _lib.check(rc, "mh_drop_path_layernorm_bwd")
    return dx, dxb


def drop_path_gather_scale(src: torch.Tensor, keep_out, scale: float, N: int):
    """bf16(scale * src) of the samples of `keep_out` (None = all), compact [K*N, D]; src [B*N, D] f32."""
    if not isinstance(src, torch.Tensor) or src.dim() != 2 or N < 1 or src.shape[0] % N:
        raise ValueError("drop_path_gather_scale: src must be [B*N, D]")
    M, D = src.shape
    B = M // N
    _dp_dims(B, N, D, "drop_path_gather_scale")
    _dp_dense(src, F32, M, D, "drop_path_gather_scale.src")
    m_out = _dp_map(keep_out, B, "drop_path_gather_scale.keep_out") if keep_out is not None else None
    if not 1 <= B <= DROP_PATH_MAX_B:
        raise ValueError(f"drop_path_gather_scale: {B} samples (1 .. {DROP_PATH_MAX_B} supported)")
    K = B if m_out is None else m_out.K
    if K < 1:
        raise ValueError("drop_path_gather_scale: keep_out keeps nothing")
    dst = torch.empty((K * N, D), dtype=BF16, device=src.device)
    rc = _L().mh_drop_path_gather_scale(_p(src), m_out.ptr() if m_out else None, K, float(scale), _p(dst), B, N, D, _s())
    _lib.check(rc, "mh_drop_path_gather_scale")
    return dst


def drop_path_layernorm_param_grads(dy: torch.Tensor, x: torch.Tensor, eps: float, keep_in, N: int, dgamma: torch.Tensor,
                                    dbeta: torch.Tensor, accumulate: bool = False):
    """dgamma (+)= sum dy * xhat(x), dbeta (+)= sum dy over the rows of the kept samples only: dy [K*N, D] f32 compact, x [B*N, D]
    f32 the LayerNorm's input.  Fixed summation order (16 compact rows a block, blocks in order)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or N < 1 or x.shape[0] % N:
        raise ValueError("drop_path_layernorm_param_grads: x must be [B*N, D]")
    M, D = x.shape
    B = M // N
    _dp_dims(B, N, D, "drop_path_layernorm_param_grads", max_d=4096)
    m_in = _dp_map(keep_in, B, "drop_path_layernorm_param_grads.keep_in")
    if m_in.K < 1:
        raise ValueError("drop_path_layernorm_param_grads: nothing kept (leave the gradients alone)")
    _dp_dense(x, F32, M, D, "drop_path_layernorm_param_grads.x")
    _dp_dense(dy, F32, m_in.K * N, D, "drop_path_layernorm_param_grads.dy")
    _dp_vec(dgamma, D, "drop_path_layernorm_param_grads.dgamma")
    _dp_vec(dbeta, D, "drop_path_layernorm_param_grads.dbeta")
    L = _L()
    n = L.mh_drop_path_param_grads_ws_floats(m_in.K, N, D)
    ws = torch.empty((max(n, 1),), dtype=F32, device=x.device)
    rc = L.mh_drop_path_layernorm_param_grads(_p(dy), _p(x), m_in.ptr(), m_in.K, _p(dgamma), _p(dbeta), B, N, D, float(eps),
                                              int(accumulate), _p(ws), n, _s())
    _lib.check(rc, "mh_drop_path_layernorm_param_grads")
    return dgamma, dbeta


def dropout_keep_mask(n: int, p: float, seed: int, device):
    """The keep mask the dropout kernels use: element i = 1/(1-p) if kept, else 0 (flat index i of the masked tensor)."""
    out = torch.empty((n,), dtype=F32, device=device)
    _lib.check(_L().mh_dropout_keep_mask(_p(out), int(n), float(p), int(seed), _s()), "mh_dropout_keep_mask")
    return out


def gemm_tn_wgrad(dy: torch.Tensor, x: torch.Tensor, out: torch.Tensor, bias: Optional[torch.Tensor] = None,
                  accumulate: bool = False, splits: int = 0):
    """out[N,K] (+)= dy^T . x for row-major bf16 dy [M,N] and x [M,K] (no transposed copies), fp32 into `out` (row-strided);
    `bias` [N] f32 (+)= the column sums of dy in the same launch.  splits = 0: the library's M-split choice."""
    _chk2d(dy, BF16, "dy")
    _chk2d(x, BF16, "x")
    M, N = dy.shape
    K = x.shape[1]
    if x.shape[0] != M or out.dtype != F32 or out.dim() != 2 or tuple(out.shape) != (N, K) or out.stride(1) != 1:
        raise ValueError(f"gemm_tn_wgrad: dy {tuple(dy.shape)} x {tuple(x.shape)} out {tuple(out.shape)} {out.dtype}")
    if bias is not None and (bias.dtype != F32 or bias.numel() != N or not bias.is_contiguous()):
        raise ValueError("gemm_tn_wgrad: bias must be contiguous f32 [N]")
    L = _L()
    s = int(splits) if splits else L.mh_gemm_tn_wgrad_auto_splits(M, N, K)
    n = L.mh_gemm_tn_wgrad_ws_floats(M, N, K, s)
    ws = torch.empty((n,), dtype=F32, device=dy.device) if n > 0 else None
    _lib.check(L.mh_gemm_tn_wgrad(_p(dy), dy.stride(0), _p(x), x.stride(0), _p(out), out.stride(0), _p(bias), M, N, K,
                                  int(accumulate), s, _p(ws), n, _s()), f"mh_gemm_tn_wgrad M={M} N={N} K={K}")
    return out


# --------------------------------------------------------------------------- elementwise
def rope_(x2d: torch.Tensor, col0: int, n_heads: int, head_dim: int, pos: torch.Tensor, cos, sin, sign: float = 1.0):
    n_tok = x2d.shape[0]
    _lib.check(_L().mh_rope_inplace(_p(x2d), x2d.stride(0), col0, n_tok, n_heads, head_dim, _p(pos), _p(cos), _p(sin),
                                    float(sign), _s()), "mh_rope_inplace")
    return x2d


def silu_mul_fwd(gu: torch.Tensor):
    M, I2 = gu.shape
    h = torch.empty((M, I2 // 2), dtype=BF16, device=gu.device)
    _lib.check(_L().mh_silu_mul_fwd(_p(gu), _p(h), M, I2 // 2, _s()), "mh_silu_mul_fwd")
    return h


def silu_mul_bwd(dh: torch.Tensor, gu: torch.Tensor):
    M, I2 = gu.shape
    dgu = torch.empty_like(gu)
    _lib.check(_L().mh_silu_mul_bwd(_p(dh), _p(gu), _p(dgu), M, I2 // 2, _s()), "mh_silu_mul_bwd")
    return dgu


SWIGLU_BLK = 128      # gate / up interleave of the fused MLP GEMMs (csrc/gemm.hip mh_gemm_swiglu_*)


def interleave_gate_up(wg: torch.Tensor, wu: torch.Tensor, blk: int = SWIGLU_BLK) -> torch.Tensor:
    """[I, D] gate and up weights -> [2I, D] with rows [g 0..blk-1 | u 0..blk-1 | g blk.. | ...] (I % blk == 0)."""
    I, D = wg.shape
    if I % blk:
        raise _lib.MyriadHipError(f"interleave_gate_up: I={I} is not a multiple of {blk}")
    return torch.stack([wg.reshape(I // blk, blk, D), wu.reshape(I // blk, blk, D)], 1).reshape(2 * I, D).contiguous()


def silu_mul_fwd_blk(gu: torch.Tensor, blk: int = SWIGLU_BLK):
    M, I2 = gu.shape
    h = torch.empty((M, I2 // 2), dtype=BF16, device=gu.device)
    _lib.check(_L().mh_silu_mul_fwd_blk(_p(gu), _p(h), M, I2 // 2, blk, _s()), "mh_silu_mul_fwd_blk")
    return h


def silu_mul_bwd_blk(dh: torch.Tensor, gu: torch.Tensor, blk: int = SWIGLU_BLK):
    M, I2 = gu.shape
    dgu = torch.empty_like(gu)
    _lib.check(_L().mh_silu_mul_bwd_blk(_p(dh), _p(gu), _p(dgu), M, I2 // 2, blk, _s()), "mh_silu_mul_bwd_blk")
    return dgu


def gemm_swiglu_fwd(x: torch.Tensor, wgu: torch.Tensor):
    """(gu [M, 2I] bf16 in the interleaved layout, act [M, I] = silu(g) * u): the gate|up projection with the gated product
    in its epilogue (separate launches, same bits, when the policy does not run the fused kernel)."""
    _chk2d(x, BF16, "gemm_swiglu_fwd.x")
    _chk2d(wgu, BF16, "gemm_swiglu_fwd.wgu")
    M, K = x.shape
    I = wgu.shape[0] // 2
    gu = torch.empty((M, 2 * I), dtype=BF16, device=x.device)
    act = torch.empty((M, I), dtype=BF16, device=x.device)
    rc = _L().mh_gemm_swiglu_fwd(_p(x), x.stride(0), _p(wgu), wgu.stride(0), _p(gu), 2 * I, _p(act), I, M, I, K, _s())
    _lib.check(rc, f"mh_gemm_swiglu_fwd M={M} I={I} K={K}")
    return gu, act


def gemm_swiglu_bwd(dh: torch.Tensor, wdT: torch.Tensor, gu: torch.Tensor):
    """dgu [M, 2I] = silu_mul_bwd(dh @ wdT^T, gu): the down projection's dgrad with the gate backward in its epilogue."""
    _chk2d(dh, BF16, "gemm_swiglu_bwd.dh")
    _chk2d(wdT, BF16, "gemm_swiglu_bwd.wdT")
    _chk2d(gu, BF16, "gemm_swiglu_bwd.gu")
    M, K = dh.shape
    I = wdT.shape[0]
    dgu = torch.empty_like(gu)
    dact = torch.empty((M, I), dtype=BF16, device=dh.device)
    rc = _L().mh_gemm_swiglu_bwd(_p(dh), dh.stride(0), _p(wdT), wdT.stride(0), _p(gu), gu.stride(0), _p(dgu), dgu.stride(0),
                                 _p(dact), M, I, K, _s())
    _lib.check(rc, f"mh_gemm_swiglu_bwd M={M} I={I} K={K}")
    return dgu


def gemm_gelu_fwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None):
    """(pre [M, N] bf16 = x @ w^T + bias, act = gelu(pre)): the MLP's first product with the GELU in its epilogue (separate
    launches, same bits, when the policy does not run an unsplit tile kernel)."""
    _chk2d(x, BF16, "gemm_gelu_fwd.x")
    _chk2d(w, BF16, "gemm_gelu_fwd.w")
    M, K = x.shape
    N = w.shape[0]
    pre = torch.empty((M, N), dtype=BF16, device=x.device)
    act = torch.empty((M, N), dtype=BF16, device=x.device)
    rc = _L().mh_gemm_gelu_fwd(_p(x), x.stride(0), _p(w), w.stride(0), _p(bias), _p(pre), N, _p(act), N, M, N, K, _s())
    _lib.check(rc, f"mh_gemm_gelu_fwd M={M} N={N} K={K}")
    return pre, act


def gemm_gelu_bwd(dy: torch.Tensor, wT: torch.Tensor, pre: torch.Tensor):
    """dpre [M, N] bf16 = bf16(dy @ wT^T) * gelu'(pre): the MLP's second dgrad with the GELU backward in its epilogue."""
    _chk2d(dy, BF16, "gemm_gelu_bwd.dy")
    _chk2d(wT, BF16, "gemm_gelu_bwd.wT")
    _chk2d(pre, BF16, "gemm_gelu_bwd.pre")
    M, K = dy.shape
    N = wT.shape[0]
    dpre = torch.empty((M, N), dtype=BF16, device=dy.device)
    dact = torch.empty((M, N), dtype=BF16, device=dy.device)
    rc = _L().mh_gemm_gelu_bwd(_p(dy), dy.stride(0), _p(wT), wT.stride(0), _p(pre), pre.stride(0), _p(dpre), N, _p(dact), M, N, K, _s())
    _lib.check(rc, f"mh_gemm_gelu_bwd M={M} N={N} K={K}")
    return dpre


def gelu_fwd(x):
    y = torch.empty_like(x)
    _lib.check(_L().mh_gelu_fwd(_p(x), _p(y), x.numel(), _s()), "mh_gelu_fwd")
    return y


def gelu_bwd(dy, x):
    dx = torch.empty_like(x)
    _lib.check(_L().mh_gelu_bwd(_p(dy), _p(x), _p(dx), x.numel(), _s()), "mh_gelu_bwd")
    return dx


def to_bf16(x: torch.Tensor, out=None):
    if out is None:
        out = torch.empty(x.shape, dtype=BF16, device=x.device)
    _lib.check(_L().mh_cast_f32_to_bf16(_p(x), _p(out), x.numel(), _s()), "mh_cast_f32_to_bf16")
    return out


def to_f32(x: torch.Tensor, out=None):
    if out is None:
        out = torch.empty(x.shape, dtype=F32, device=x.device)
    _lib.check(_L().mh_cast_bf16_to_f32(_p(x), _p(out), x.numel(), _s()), "mh_cast_bf16_to_f32")
    return out


def transpose_to_bf16(x2d: torch.Tensor, pad_to: int = 64, out=None):
    """[R,C] (f32 or bf16) -> [C, round_up(R,pad_to)] bf16, zero padded."""
    R, C = x2d.shape
    ldo = round_up(R, pad_to)
    if out is None:
        out = torch.empty((C, ldo), dtype=BF16, device=x2d.device)
    _lib.check(_L().mh_transpose_to_bf16(_p(x2d), int(x2d.dtype == F32), x2d.stride(0), _p(out), out.stride(0), R, C,
                                         _s()), "mh_transpose_to_bf16")
    return out


class RefreshTable:
    """The fp32 master -> bf16 working copy (+ transposed copy) refresh of a list of matrices as ONE launch
    (mh_refresh_bf16_pair).  entries = [(src f32 [R, C] contiguous, dst bf16 [>= R, >= C] or None, dst_t bf16 [>= C, >= R] or None)];
    only the [R, C] part of a wider destination is written.  The descriptor table is built and uploaded once, here; run()
    rewrites the copies from whatever the masters hold now, on the current stream.  The tensors must outlive the table."""

    def __init__(self, entries, device):
        L = _L()
        nb = int(L.mh_refresh_bf16_pair_desc_bytes())
        self.n = len(entries)
        self.tiles = 0
        self._keep = list(entries)
        self.weights = 0
        if not self.n:
            self.table = None
            return
        host = torch.zeros((self.n * nb,), dtype=torch.uint8)
        for i, (src, dst, dst_t) in enumerate(entries):
            if src.dtype != F32 or src.dim() != 2 or not src.is_contiguous():
                raise _lib.MyriadHipError(f"RefreshTable entry {i}: the source must be a contiguous f32 matrix")
            R, C = src.shape
            for t, rows, cols, name in ((dst, R, C, "dst"), (dst_t, C, R, "dst_t")):
                if t is not None and (t.dtype != BF16 or t.dim() != 2 or t.stride(1) != 1 or t.shape[0] < rows
                                      or t.shape[1] < cols or t.device != src.device):
                    raise _lib.MyriadHipError(f"RefreshTable entry {i}: {name} must be bf16 [>= {rows}, >= {cols}] with unit "
                                              "inner stride, on the source's device")
            nxt = int(L.mh_refresh_bf16_pair_pack(host.data_ptr(), i, self.tiles, _p(src), _p(dst),
                                                  0 if dst is None else dst.stride(0), _p(dst_t),
                                                  0 if dst_t is None else dst_t.stride(0), R, C))
            if nxt < 0:
                _lib.check(nxt, f"mh_refresh_bf16_pair_pack (entry {i})")
            self.tiles = nxt
            self.weights += R * C
        self.table = host.to(device)

    def run(self) -> None:
        if self.n:
            _lib.check(_L().mh_refresh_bf16_pair(_p(self.table), self.n, self.tiles, _s()), "mh_refresh_bf16_pair")


def refresh_bf16_pair(src: torch.Tensor, dst: Optional[torch.Tensor] = None, dst_t: Optional[torch.Tensor] = None) -> None:
    """One matrix through mh_refresh_bf16_pair (tests, one-off uses: the table is built and uploaded per call)."""
    RefreshTable([(src, dst, dst_t)], src.device).run()


def copy2d(src: torch.Tensor, dst: torch.Tensor, accumulate: bool = False):
    rows, cols = src.shape
    _lib.check(_L().mh_copy2d_f32(_p(src), src.stride(0), _p(dst), dst.stride(0), rows, cols, int(accumulate), _s()),
               "mh_copy2d_f32")
    return dst


def copy3d(src: torch.Tensor, dst: torch.Tensor, accumulate: bool = False):
    nb, rows, cols = src.shape
    _lib.check(_L().mh_copy3d_f32(_p(src), src.stride(0), src.stride(1), _p(dst), dst.stride(0), dst.stride(1), nb,
                                  rows, cols, int(accumulate), _s()), "mh_copy3d_f32")
    return dst


def embed_gather(table: torch.Tensor, ids: torch.Tensor, out: torch.Tensor, dst_rows: Optional[torch.Tensor] = None):
    """out[dst_rows[i]] = f32(table[ids[i]]); out is a 2-D f32 view."""
    n = ids.numel()
    D = table.shape[1]
    _lib.check(_L().mh_embed_gather(_p(table), _p(ids), _p(dst_rows), _p(out), n, D, out.stride(0), _s()),
               "mh_embed_gather")
    return out


def gather_rows_bf16(src: torch.Tensor, rows: torch.Tensor):
    n, D = rows.numel(), src.shape[1]
    out = torch.empty((n, D), dtype=BF16, device=src.device)
    _lib.check(_L().mh_gather_rows_f32_to_bf16(_p(src), src.stride(0), _p(rows), _p(out), n, D, _s()),
               "mh_gather_rows_f32_to_bf16")
    return out


def gather_rows(src: torch.Tensor, rows: torch.Tensor):
    """src [*, D] (bf16 or f32, row stride free) -> [n, D] dense, same dtype: rows `rows` (int32, device)."""
    n, D = rows.numel(), src.shape[1]
    out = torch.empty((n, D), dtype=src.dtype, device=src.device)
    _lib.check(_L().mh_gather_rows(_p(src), src.stride(0), _p(rows), _p(out), n, D, src.element_size(), _s()), "mh_gather_rows")
    return out


def expand_rows(src: torch.Tensor, inv: torch.Tensor, M: int):
    """[n, D] dense -> [M, D] with row m = src[inv[m]] or zeros where inv[m] < 0 (inv int32 [M], device)."""
    D = src.shape[1]
    out = torch.empty((M, D), dtype=src.dtype, device=src.device)
    _lib.check(_L().mh_expand_rows(_p(src), _p(inv), _p(out), D, M, D, src.element_size(), _s()), "mh_expand_rows")
    return out


def gather_rows_f32(src: torch.Tensor, rows: torch.Tensor):
    n, D = rows.numel(), src.shape[1]
    out = torch.empty((n, D), dtype=F32, device=src.device)
    _lib.check(_L().mh_gather_rows_f32(_p(src), src.stride(0), _p(rows), _p(out), n, D, _s()), "mh_gather_rows_f32")
    return out


def copy3d_bf16(src: torch.Tensor, dst: torch.Tensor):
    nb, rows, cols = src.shape
    _lib.check(_L().mh_copy3d_bf16(_p(src), src.stride(0), src.stride(1), _p(dst), dst.stride(0), dst.stride(1), nb,
                                   rows, cols, _s()), "mh_copy3d_bf16")
    return dst


def patchify(img: torch.Tensor, P: int):
    B, C, H, W = img.shape
    Kpad = round_up(C * P * P, 64)
    out = torch.empty((B * (H // P) * (W // P), Kpad), dtype=BF16, device=img.device)
    _lib.check(_L().mh_patchify_nchw(_p(img), _p(out), B, C, H, W, P, Kpad, _s()), "mh_patchify_nchw")
    return out


def scatter_rows(src: torch.Tensor, rows: torch.Tensor, dst: torch.Tensor, accumulate: bool = False):
    n, D = src.shape
    _lib.check(_L().mh_scatter_rows_f32(_p(src), _p(rows), _p(dst), dst.stride(0), n, D, int(accumulate), _s()),
               "mh_scatter_rows_f32")
    return dst


def colsum(x2d: torch.Tensor):
    R, C = x2d.shape
    out = torch.empty((C,), dtype=F32, device=x2d.device)
    _lib.check(_L().mh_colsum_f32(_p(x2d), x2d.stride(0), _p(out), R, C, _s()), "mh_colsum_f32")
    return out


def scale_(x: torch.Tensor, a: float):
    _lib.check(_L().mh_scale_f32(_p(x), float(a), x.numel(), _s()), "mh_scale_f32")
    return x


# --------------------------------------------------------------------------- low-rank adaptor
def lowrank_fwd(x, A, Bm):
    M, D = x.shape
    R = A.shape[0]
    y = torch.empty_like(x)
    t = torch.empty((M, R), dtype=F32, device=x.device)
    _lib.check(_L().mh_lowrank_fwd(_p(x), _p(A), _p(Bm), _p(y), _p(t), M, D, R, _s()), "mh_lowrank_fwd")
    return y, t


def lowrank_bwd(dy, x, t, A, Bm, dA, dB, need_dx=False):
    M, D = x.shape
    R = A.shape[0]
    ws = torch.empty((_L().mh_lowrank_bwd_ws_floats(M, D, R),), dtype=F32, device=x.device)
    dx = torch.empty_like(x) if need_dx else None
    _lib.check(_L().mh_lowrank_bwd(_p(dy), _p(x), _p(t), _p(A), _p(Bm), _p(dA), _p(dB), _p(dx), _p(ws), M, D, R, _s()),
               "mh_lowrank_bwd")
    return dx


# --------------------------------------------------------------------------- loss / decode
def clamp_ce(logits: torch.Tensor, labels: torch.Tensor, grad_scale: float, want_grad: bool = True, ldd: int = 0):
    R, V = logits.shape
    row_loss = torch.empty((R,), dtype=F32, device=logits.device)
    dlog = None
    if want_grad:
        ldd = ldd or round_up(V, 64)
        dlog = torch.empty((R, ldd), dtype=BF16, device=logits.device)
    _lib.check(_L().mh_clamp_ce(_p(logits), logits.stride(0), _p(labels), _p(row_loss), _p(dlog), ldd, R, V,
                                float(grad_scale), _s()), "mh_clamp_ce")
    return row_loss, dlog


def sum_f32(x: torch.Tensor, scale: float = 1.0):
    out = torch.empty((1,), dtype=F32, device=x.device)
    _lib.check(_L().mh_sum_f32(_p(x), _p(out), x.numel(), float(scale), _s()), "mh_sum_f32")
    return out


def kv_append(src2d: torch.Tensor, cache: torch.Tensor, pos_dev: torch.Tensor):
    """cache[b, pos_dev[0], :] = src2d[b, :] with the position read on the device (graph-replayable)."""
    B, cols = src2d.shape
    _lib.check(_L().mh_kv_append_bf16(_p(src2d), src2d.stride(0), _p(cache), cache.stride(0), cache.stride(1),
                                      _p(pos_dev), B, cols, _s()), "mh_kv_append_bf16")


def rope_kv_append(qkv2d: torch.Tensor, n_heads: int, head_dim: int, pos: torch.Tensor, cos_tab: torch.Tensor,
                   sin_tab: torch.Tensor, cache: torch.Tensor, pos_dev: torch.Tensor):
    """Decode token: rotary on q (in place) and k, k|v written to cache[b, pos_dev[0]] -- one launch."""
    _chk2d(qkv2d, BF16, "rope_kv_append.qkv")
    B = qkv2d.shape[0]
    if qkv2d.shape[1] < 3 * n_heads * head_dim or cache.shape[2] != 2 * n_heads * head_dim:
        raise _lib.MyriadHipError("rope_kv_append: qkv must be [B, >=3W] and cache [B, T, 2W]")
    _lib.check(_L().mh_rope_kv_append(_p(qkv2d), qkv2d.stride(0), n_heads, head_dim, _p(pos), _p(cos_tab), _p(sin_tab),
                                      _p(cache), cache.stride(0), cache.stride(1), _p(pos_dev), B, _s()),
               "mh_rope_kv_append")


def add_i32_(x: torch.Tensor, delta: int):
    _lib.check(_L().mh_add_i32(_p(x), x.numel(), int(delta), _s()), "mh_add_i32")
    return x


def argmax_rows(logits: torch.Tensor, ban_id: int = -1, want_margin: bool = False, out=None, margin_out=None):
    R, V = logits.shape
    if out is None:
        out = torch.empty((R,), dtype=torch.long, device=logits.device)
    margin = margin_out
    if margin is None and want_margin:
        margin = torch.empty((R,), dtype=F32, device=logits.device)
    _lib.check(_L().mh_argmax_rows(_p(logits), logits.stride(0), _p(out), _p(margin), R, V, ban_id, _s()),
               "mh_argmax_rows")
    return (out, margin) if want_margin else out


def argmax_pmax_rows(logits: torch.Tensor, out, margin_out, pmax_out, ban_id: int = -1, inv_temp: float = 1.0):
    """Row arg-max + top-1/top-2 margin + p_max = softmax(logits * inv_temp)[argmax] into the given buffers."""
    R, V = logits.shape
    _lib.check(_L().mh_argmax_pmax_rows(_p(logits), logits.stride(0), _p(out), _p(margin_out), _p(pmax_out), R, V, ban_id,
                                        float(inv_temp), _s()), "mh_argmax_pmax_rows")
    return out, margin_out, pmax_out


def decode_record(nxt, margin, pmax, rec, next_ids, step_dev):
    """rec[3, R] = this step's (ids, margins, p_max) as f32; next_ids = ids; step += 1 -- all on the device (graph-replayable)."""
    R = nxt.numel()
    _lib.check(_L().mh_decode_record(_p(nxt), _p(margin), _p(pmax), _p(rec), _p(next_ids), _p(step_dev), R, _s()),
               "mh_decode_record")


def decode_advance(nxt, margin, pmax, rec, next_ids, step_dev, pos, kvlen):
    """decode_record() and pos += 1, kvlen += 1 in one launch (the end of a KV-cache token step)."""
    R = nxt.numel()
    _lib.check(_L().mh_decode_advance(_p(nxt), _p(margin), _p(pmax), _p(rec), _p(next_ids), _p(step_dev), _p(pos), _p(kvlen), R,
                                      _s()), "mh_decode_advance")


def decode_advance_rows(nxt, margin, pmax, rec, next_ids, step_dev, pos, kvlen, live):
    """decode_advance() for the rows with live[r] != 0 (int32 [R]); an idle row records (-1, 0, 0) and keeps next_ids / pos / kvlen."""
    R = nxt.numel()
    _lib.check(_L().mh_decode_advance_rows(_p(nxt), _p(margin), _p(pmax), _p(rec), _p(next_ids), _p(step_dev), _p(pos), _p(kvlen),
                                           _p(live), R, _s()), "mh_decode_advance_rows")


GEMV_MAX_ROWS = 16     # most rows mh_gemv_packed and its fused forms take (include/myriad_hip.h)
GEMV_WIDE_MAX_ROWS = 64    # most rows mh_gemv_packed*_wide take: the slot engine's row limit
SAMPLE_CAP = 1024      # most top-k candidates mh_sample_rows sorts on the device (include/myriad_hip.h)


def sample_rows(logits: torch.Tensor, out, margin_out, pmax_out, kept_out, params: torch.Tensor, seed: torch.Tensor,
                ban_id: int = -1, step=None, t_add: int = 0, u_out=None):
    """HF top-k / top-p draw of one id per row on the device: params = f32 (inv_temp, top_p, top_k, penalty), seed = one int64,
    Philox counter t = step[0] + t_add (t_add alone without `step`).  kept_out[r] = kept-set size, -1 = draw the row elsewhere."""
    R, V = logits.shape
    _lib.check(_L().mh_sample_rows(_p(logits), logits.stride(0), _p(out), _p(margin_out), _p(pmax_out), _p(kept_out), _p(u_out), R, V,
                                   int(ban_id), _p(params), _p(seed), _p(step), int(t_add), _s()), "mh_sample_rows")
    return out, kept_out


def repetition_penalty_rows(logits: torch.Tensor, seen: torch.Tensor, prev_ids, penalty: torch.Tensor):
    """In place: add prev_ids[r] to row r's seen-id bitmap (int32 [R, ceil(V/32)]), then x * p / x / p on every seen id."""
    R, V = logits.shape
    _lib.check(_L().mh_repetition_penalty_rows(_p(logits), logits.stride(0), _p(seen), _p(prev_ids), R, V, _p(penalty), _s()),
               "mh_repetition_penalty_rows")
    return logits


def decode_advance_kept(nxt, margin, pmax, kept, rec, next_ids, step_dev, pos, kvlen):
    """decode_advance() with the sampler's kept counts as a fourth record row (rec[4, R])."""
    R = nxt.numel()
    _lib.check(_L().mh_decode_advance_kept(_p(nxt), _p(margin), _p(pmax), _p(kept), _p(rec), _p(next_ids), _p(step_dev), _p(pos),
                                           _p(kvlen), R, _s()), "mh_decode_advance_kept")


def sample_rows_slots(logits: torch.Tensor, out, margin_out, pmax_out, kept_out, params: torch.Tensor, seed: torch.Tensor,
                      gen: torch.Tensor, live=None, u_out=None):
    """sample_rows() with per-row state (the slot engine's): params = f32 (inv_temp, top_p, top_k, penalty, min_length, eos_id),
    seed = int64 [R], gen = int32 [R] (Philox step of row r's draw; eos_id is banned while gen[r] < min_length), live = int32 [R]
    or None (every row live).  An idle row gets out = -1, margin = p_max = 0, kept = 0."""
    R, V = logits.shape
    _lib.check(_L().mh_sample_rows_slots(_p(logits), logits.stride(0), _p(out), _p(margin_out), _p(pmax_out), _p(kept_out), _p(u_out),
                                         R, V, _p(params), _p(seed), _p(gen), _p(live), _s()), "mh_sample_rows_slots")
    return out, kept_out


def argmax_pmax_rows_slots(logits: torch.Tensor, out, margin_out, pmax_out, params: torch.Tensor, gen: torch.Tensor, live=None):
    """argmax_pmax_rows() with sample_rows_slots' per-row EOS ban and idle rows; inv_temp is params[0]."""
    R, V = logits.shape
    _lib.check(_L().mh_argmax_pmax_rows_slots(_p(logits), logits.stride(0), _p(out), _p(margin_out), _p(pmax_out), R, V, _p(params),
                                              _p(gen), _p(live), _s()), "mh_argmax_pmax_rows_slots")
    return out, margin_out, pmax_out


def repetition_penalty_rows_slots(logits: torch.Tensor, seen: torch.Tensor, prev_ids, penalty: torch.Tensor, live: torch.Tensor):
    """repetition_penalty_rows() for the rows with live[r] != 0; an idle row keeps its logits and its bitmap."""
    R, V = logits.shape
    _lib.check(_L().mh_repetition_penalty_rows_slots(_p(logits), logits.stride(0), _p(seen), _p(prev_ids), R, V, _p(penalty), _p(live),
                                                     _s()), "mh_repetition_penalty_rows_slots")
    return logits


def decode_advance_kept_rows(nxt, margin, pmax, kept, rec, next_ids, step_dev, pos, kvlen, gen, live):
    """decode_advance_kept() for the rows with live[r] != 0, which also advance gen[r]; an idle row records (-1, 0, 0, 0) and keeps
    its state.  kept may be None (fourth record row 0)."""
    R = (nxt if live is None else live).numel()
    _lib.check(_L().mh_decode_advance_kept_rows(_p(nxt), _p(margin), _p(pmax), _p(kept), _p(rec), _p(next_ids), _p(step_dev), _p(pos),
                                                _p(kvlen), _p(gen), _p(live), R, _s()), "mh_decode_advance_kept_rows")


SCORE_WATCH_MAX = 8    # watch slots of mh_token_scores_rows (include/myriad_hip.h)
SCORE_ROWS = 2 + SCORE_WATCH_MAX    # rows of its output: lse, the pick's log-prob, one per watch slot


def score_watch_ids(watch_ids, V: int) -> list:
    """The decode loops' check of `watch_ids`: at most SCORE_WATCH_MAX integers in [0, V) (ValueError otherwise), as a list."""
    watch = list(watch_ids)
    if len(watch) > SCORE_WATCH_MAX:
        raise ValueError(f"watch_ids: at most {SCORE_WATCH_MAX} ids, got {len(watch)}")
    for w in watch:
        if isinstance(w, bool) or not isinstance(w, numbers.Integral) or not 0 <= int(w) < V:
            raise ValueError(f"watch_ids: integers in [0, {V}), got {w!r}")
    return [int(w) for w in watch]


def score_watch_table(watch_ids, V: int) -> torch.Tensor:
    """score_watch_ids as the int32 [SCORE_WATCH_MAX] host table the kernel reads once uploaded: unused slots hold -1."""
    watch = score_watch_ids(watch_ids, V)
    return torch.tensor(watch + [-1] * (SCORE_WATCH_MAX - len(watch)), dtype=torch.int32)


def token_scores_rows(logits: torch.Tensor, ids: torch.Tensor, watch: torch.Tensor, out: torch.Tensor, live=None):
    """Log-softmax (temperature 1) of each row of f32 logits [R, V] at its pick ids[r] and at the SCORE_WATCH_MAX int32 ids of the
    device table `watch` (-1 = unused: 0.0) into out [SCORE_ROWS, >= R] f32 (any row stride): lse, the pick's log-prob, one row per
    watch slot.  A row with live[r] == 0 or ids[r] < 0 gets zeros and its logits are not read."""
    R, V = logits.shape
    if watch.numel() != SCORE_WATCH_MAX or watch.dtype != torch.int32 or out.shape[0] != SCORE_ROWS or out.stride(1) != 1:
        raise _lib.MyriadHipError(f"token_scores_rows: watch is int32 [{SCORE_WATCH_MAX}] and out f32 [{SCORE_ROWS}, >= R]")
    _lib.check(_L().mh_token_scores_rows(_p(logits), logits.stride(0), _p(ids), _p(watch), _p(out), out.stride(0), R, V, _p(live),
                                         _s()), "mh_token_scores_rows")
    return out


BEAM_MAX = 8           # most beams mh_beam_topk / mh_beam_reorder_kv take (include/myriad_hip.h)


def _chk_flat(t, dtype, need: int, name: str):
    """A buffer a kernel indexes linearly: a contiguous cuda tensor of `dtype` with at least `need` elements."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or t.numel() < need:
        got = f"{t.dtype} {tuple(t.shape)} cuda={t.is_cuda} contiguous={t.is_contiguous()}" if isinstance(t, torch.Tensor) else repr(t)
        raise _lib.MyriadHipError(f"{name}: need a contiguous cuda {dtype} tensor of at least {need} elements, got {got}")


def beam_topk(logits: torch.Tensor, scores: torch.Tensor, part_s, part_i, out_s, out_i, B: int, nb: int, ban_id: int = -1,
              pos=None, kvlen=None):
    """The beam step's selection: per item b the top 2*nb of (scores[row] + log_softmax(logits[row])) over the item's rows
    (logits [B*rpi, V], rpi = nb, or 1 for the step after a B-row prefill), best first, ties to the lower flat index
    row_in_item * V + token, into out_s (f32) / out_i (int32) [B, 2*nb].  part_s / part_i: scratch of B*rpi*2*nb entries.
    With pos / kvlen (both or neither, int32, one length), every row of those buffers advances by one (the end of a token
    step).  A buffer of the wrong type or too short for what the kernels index is refused here, before any launch."""
    _chk2d(logits, F32, "beam_topk: logits")
    R, V = logits.shape
    if B <= 0 or R % B != 0:
        raise _lib.MyriadHipError(f"beam_topk: {R} logits rows do not divide into B={B} items")
    rpi = R // B
    for name, t, dtype, need in (("scores", scores, F32, R), ("part_s", part_s, F32, R * 2 * nb), ("part_i", part_i, torch.int32, R * 2 * nb),
                                 ("out_s", out_s, F32, B * 2 * nb), ("out_i", out_i, torch.int32, B * 2 * nb)):
        _chk_flat(t, dtype, need, f"beam_topk: {name}")
    if (pos is None) != (kvlen is None):
        raise _lib.MyriadHipError("beam_topk: pos and kvlen advance together: give both or neither")
    n_adv = 0
    if pos is not None:
        n_adv = pos.numel()
        _chk_flat(pos, torch.int32, n_adv, "beam_topk: pos")
        _chk_flat(kvlen, torch.int32, n_adv, "beam_topk: kvlen")
        if kvlen.numel() != n_adv:
            raise _lib.MyriadHipError(f"beam_topk: pos has {n_adv} rows and kvlen {kvlen.numel()}")
    _lib.check(_L().mh_beam_topk(_p(logits), logits.stride(0), _p(scores), _p(part_s), _p(part_i), _p(out_s), _p(out_i), B, rpi, nb,
                                 V, int(ban_id), _p(pos), _p(kvlen), n_adv, _s()), "mh_beam_topk")
    return out_s, out_i


def beam_reorder_kv(cache_table: torch.Tensor, L: int, B: int, nb: int, T_cap: int, C: int, src, lo, hi):
    """In place, every layer: cache[r, p] = cache[src[r], p] for p in [lo[0], hi[0]); cache_table = int64 device tensor of the L
    [B*nb, T_cap, C] bf16 cache base pointers; src / lo / hi int32 device tensors (read by the kernel: capturable).  A table
    shorter than L, a src shorter than B*nb or a tensor of another type is refused here, before any launch."""
    _chk_flat(cache_table, torch.long, L, "beam_reorder_kv: cache_table")
    _chk_flat(src, torch.int32, B * nb, "beam_reorder_kv: src")
    _chk_flat(lo, torch.int32, 1, "beam_reorder_kv: lo")
    _chk_flat(hi, torch.int32, 1, "beam_reorder_kv: hi")
    _lib.check(_L().mh_beam_reorder_kv(_p(cache_table), L, B, nb, int(T_cap), C, _p(src), _p(lo), _p(hi), _s()),
               "mh_beam_reorder_kv")


def beam_topk_items(logits: torch.Tensor, scores: torch.Tensor, part_s, part_i, out_s, out_i, G: int, nb: int, live, gen, prm, pos,
                    kvlen):
    """beam_topk for the decode slots' G beam groups (logits [G*nb, V], one request per item): live / gen int32 [G] and prm =
    int32 (min_length, eos_id) are read by the kernels.  A live item bans eos_id iff gen[g] < min_length, records what beam_topk
    records for it alone, and advances its nb rows of pos / kvlen and its gen by one; an idle item records (0.0, -1) and keeps
    everything else.  A buffer of the wrong type or too short is refused here, before any launch."""
    _chk2d(logits, F32, "beam_topk_items: logits")
    R, V = logits.shape
    if G <= 0 or nb <= 0 or R != G * nb:
        raise _lib.MyriadHipError(f"beam_topk_items: {R} logits rows are not G={G} items of nb={nb} rows")
    i32 = torch.int32
    for name, t, dtype, need in (("scores", scores, F32, R), ("part_s", part_s, F32, R * 2 * nb), ("part_i", part_i, i32, R * 2 * nb),
                                 ("out_s", out_s, F32, G * 2 * nb), ("out_i", out_i, i32, G * 2 * nb), ("live", live, i32, G),
                                 ("gen", gen, i32, G), ("prm", prm, i32, 2), ("pos", pos, i32, R), ("kvlen", kvlen, i32, R)):
        _chk_flat(t, dtype, need, f"beam_topk_items: {name}")
    _lib.check(_L().mh_beam_topk_items(_p(logits), logits.stride(0), _p(scores), _p(part_s), _p(part_i), _p(out_s), _p(out_i), G, nb, V,
                                       _p(live), _p(gen), _p(prm), _p(pos), _p(kvlen), _s()), "mh_beam_topk_items")
    return out_s, out_i


def beam_reorder_kv_items(cache_table: torch.Tensor, L: int, G: int, nb: int, T_cap: int, C: int, src, lo, hi, live):
    """beam_reorder_kv with a window [lo[g], hi[g]) (clamped to [0, T_cap)) and a live flag per item, int32 [G] device tensors read
    by the kernel; an idle item and every position outside a window are not touched."""
    _chk_flat(cache_table, torch.long, L, "beam_reorder_kv_items: cache_table")
    _chk_flat(src, torch.int32, G * nb, "beam_reorder_kv_items: src")
    for name, t in (("lo", lo), ("hi", hi), ("live", live)):
        _chk_flat(t, torch.int32, G, f"beam_reorder_kv_items: {name}")
    _lib.check(_L().mh_beam_reorder_kv_items(_p(cache_table), L, G, nb, int(T_cap), C, _p(src), _p(lo), _p(hi), _p(live), _s()),
               "mh_beam_reorder_kv_items")


def beam_sample_topk(logits: torch.Tensor, scores: torch.Tensor, part_k, part_a, part_i, part_f, out_s, out_i, out_f, B: int, nb: int,
                     ban_id: int = -1, draw: bool = True, params=None, seed=None, seen=None, step=None, t_add: int = 0, out_k=None,
                     pos=None, kvlen=None):
    """beam_topk's selection with HF's processor chain on the log-probs and, with `draw`, beam-search multinomial sampling (the
    rule is include/myriad_hip.h's): logits [B*nb, V] (nb rows per item), params = f32 (inv_temp, top_p, top_k, penalty) and seed =
    one int64 on the device, seen = int32 [B*nb, ceil(V/32)] bitmaps or None (no penalty), Philox step t = step[0] + t_add (t_add
    alone without `step`).  Per item the top 2*nb by (key desc, flat asc): out_s = acc, out_i = flat, out_k = key (optional),
    out_f [B] = 1 where the host has to redo the item.  part_k / part_a / part_i: scratch of B*nb*2*nb entries, part_f of B*nb.
    With pos / kvlen (both or neither) those rows advance by one, and step[0] with them.  A buffer of the wrong type or too short
    for what the kernels index is refused here, before any launch."""
    _chk2d(logits, F32, "beam_sample_topk: logits")
    R, V = logits.shape
    if B <= 0 or nb <= 0 or R != B * nb:
        raise _lib.MyriadHipError(f"beam_sample_topk: {R} logits rows are not B={B} items of nb={nb} rows")
    i32, K = torch.int32, 2 * nb
    for name, t, dtype, need in (("scores", scores, F32, R), ("part_k", part_k, F32, R * K), ("part_a", part_a, F32, R * K),
                                 ("part_i", part_i, i32, R * K), ("part_f", part_f, i32, R), ("out_s", out_s, F32, B * K),
                                 ("out_i", out_i, i32, B * K), ("out_f", out_f, i32, B)):
        _chk_flat(t, dtype, need, f"beam_sample_topk: {name}")
    if out_k is not None:
        _chk_flat(out_k, F32, B * K, "beam_sample_topk: out_k")
    if draw or seen is not None:
        _chk_flat(params, F32, 4, "beam_sample_topk: params")
    if draw:
        _chk_flat(seed, torch.long, 1, "beam_sample_topk: seed")
    if seen is not None:
        _chk_flat(seen, i32, R * ((V + 31) // 32), "beam_sample_topk: seen")
    if step is not None:
        _chk_flat(step, i32, 1, "beam_sample_topk: step")
    if (pos is None) != (kvlen is None):
        raise _lib.MyriadHipError("beam_sample_topk: pos and kvlen advance together: give both or neither")
    n_adv = 0
    if pos is not None:
        n_adv = pos.numel()
        _chk_flat(pos, i32, n_adv, "beam_sample_topk: pos")
        _chk_flat(kvlen, i32, n_adv, "beam_sample_topk: kvlen")
        if kvlen.numel() != n_adv:
            raise _lib.MyriadHipError(f"beam_sample_topk: pos has {n_adv} rows and kvlen {kvlen.numel()}")
    _lib.check(_L().mh_beam_sample_topk(_p(logits), logits.stride(0), _p(scores), _p(seen), _p(part_k), _p(part_a), _p(part_i),
                                        _p(part_f), _p(out_s), _p(out_i), _p(out_f), _p(out_k), B, nb, V, int(ban_id), int(bool(draw)),
                                        _p(params), _p(seed), _p(step), int(t_add), _p(pos), _p(kvlen), n_adv, _s()),
               "mh_beam_sample_topk")
    return out_s, out_i, out_f


def beam_seen_update(seen: torch.Tensor, src: torch.Tensor, ids: torch.Tensor, B: int, nb: int, V: int):
    """In place: seen[r] = seen[src[r]] | bit(ids[r]) over the int32 [B*nb, ceil(V/32)] seen-id bitmaps; src int32 (parents within
    r's item, as beam_reorder_kv takes them), ids int64, both read by the kernel (capturable)."""
    if B <= 0 or nb <= 0 or V <= 0:
        raise _lib.MyriadHipError(f"beam_seen_update: B={B}, nb={nb}, V={V} must be positive")
    _chk_flat(seen, torch.int32, B * nb * ((V + 31) // 32), "beam_seen_update: seen")
    _chk_flat(src, torch.int32, B * nb, "beam_seen_update: src")
    _chk_flat(ids, torch.long, B * nb, "beam_seen_update: ids")
    _lib.check(_L().mh_beam_seen_update(_p(seen), _p(src), _p(ids), B, nb, V, _s()), "mh_beam_seen_update")
    return seen


def beam_sample_topk_items(logits: torch.Tensor, scores: torch.Tensor, part_k, part_a, part_i, part_f, out_s, out_i, out_f, G: int,
                           nb: int, live, gen, bprm, draw: bool = True, params=None, seed=None, seen=None, t_add: int = 0, out_k=None,
                           pos=None, kvlen=None):
    """beam_sample_topk for the decode slots' G beam groups (logits [G*nb, V], one request per item): live / gen int32 [G], bprm =
    int32 (min_length, eos_id) and seed = int64 [G] (one Philox key per item) are read by the kernels.  A live item bans eos_id
    iff gen[g] < min_length, draws Philox step gen[g] + t_add of seed[g] with the counter's item field 0 -- what beam_sample_topk
    records for it alone at B = 1 with that seed and step -- and, with pos / kvlen (both or neither, [G*nb]), advances its nb rows
    of them and its gen by one; without them nothing advances (a refill's first pick).  An idle item records (0.0, -1) with flag
    0 and keeps everything else.  A buffer of the wrong type or too short is refused here, before any launch."""
    _chk2d(logits, F32, "beam_sample_topk_items: logits")
    R, V = logits.shape
    if G <= 0 or nb <= 0 or R != G * nb:
        raise _lib.MyriadHipError(f"beam_sample_topk_items: {R} logits rows are not G={G} items of nb={nb} rows")
    i32, K = torch.int32, 2 * nb
    for name, t, dtype, need in (("scores", scores, F32, R), ("part_k", part_k, F32, R * K), ("part_a", part_a, F32, R * K),
                                 ("part_i", part_i, i32, R * K), ("part_f", part_f, i32, R), ("out_s", out_s, F32, G * K),
                                 ("out_i", out_i, i32, G * K), ("out_f", out_f, i32, G), ("live", live, i32, G), ("gen", gen, i32, G),
                                 ("bprm", bprm, i32, 2)):
        _chk_flat(t, dtype, need, f"beam_sample_topk_items: {name}")
    if out_k is not None:
        _chk_flat(out_k, F32, G * K, "beam_sample_topk_items: out_k")
    if draw or seen is not None:
        _chk_flat(params, F32, 4, "beam_sample_topk_items: params")
    if draw:
        _chk_flat(seed, torch.long, G, "beam_sample_topk_items: seed")
    if seen is not None:
        _chk_flat(seen, i32, R * ((V + 31) // 32), "beam_sample_topk_items: seen")
    if (pos is None) != (kvlen is None):
        raise _lib.MyriadHipError("beam_sample_topk_items: pos and kvlen advance together: give both or neither")
    if pos is not None:
        _chk_flat(pos, i32, R, "beam_sample_topk_items: pos")
        _chk_flat(kvlen, i32, R, "beam_sample_topk_items: kvlen")
    _lib.check(_L().mh_beam_sample_topk_items(_p(logits), logits.stride(0), _p(scores), _p(seen), _p(part_k), _p(part_a), _p(part_i),
                                              _p(part_f), _p(out_s), _p(out_i), _p(out_f), _p(out_k), G, nb, V, int(bool(draw)),
                                              _p(params), _p(seed), _p(live), _p(gen), _p(bprm), int(t_add), _p(pos), _p(kvlen),
                                              _s()), "mh_beam_sample_topk_items")
    return out_s, out_i, out_f


def beam_seen_update_items(seen: torch.Tensor, src: torch.Tensor, ids: torch.Tensor, G: int, nb: int, V: int, live: torch.Tensor):
    """beam_seen_update with a live flag per item (int32 [G], read by the kernel): an idle item's bitmap rows are neither read nor
    written."""
    if G <= 0 or nb <= 0 or V <= 0:
        raise _lib.MyriadHipError(f"beam_seen_update_items: G={G}, nb={nb}, V={V} must be positive")
    _chk_flat(seen, torch.int32, G * nb * ((V + 31) // 32), "beam_seen_update_items: seen")
    _chk_flat(src, torch.int32, G * nb, "beam_seen_update_items: src")
    _chk_flat(ids, torch.long, G * nb, "beam_seen_update_items: ids")
    _chk_flat(live, torch.int32, G, "beam_seen_update_items: live")
    _lib.check(_L().mh_beam_seen_update_items(_p(seen), _p(src), _p(ids), G, nb, V, _p(live), _s()), "mh_beam_seen_update_items")
    return seen


# --------------------------------------------------------------------------- conv stack pieces
def im2col(x_nhwc: torch.Tensor, kh: int, kw: int, pad: int, bias_col: bool = True):
    """[B*OH*OW, Kpad] bf16 patches, (ky, kx, c) order; with bias_col a column of ones follows the K patch columns (the bias
    then rides the GEMM as one more weight column).  Without it K = kh*kw*C must be a multiple of 64: the kernel marks column K
    of a padded row with 1.0, so a padded row always carries the ones column and is refused here."""
    B, H, W, C = x_nhwc.shape
    OH, OW = H + 2 * pad - kh + 1, W + 2 * pad - kw + 1
    Kpad = round_up(kh * kw * C + (1 if bias_col else 0), 64)
    if not bias_col and Kpad != kh * kw * C:
        raise _lib.MyriadHipError(f"im2col: bias_col=False needs kh*kw*C % 64 == 0, got {kh * kw * C}")
    col = torch.empty((B * OH * OW, Kpad), dtype=BF16, device=x_nhwc.device)
    _lib.check(_L().mh_im2col_nhwc(_p(x_nhwc), _p(col), B, H, W, C, kh, kw, pad, Kpad, _s()), "mh_im2col_nhwc")
    return col


def col2im(dcol: torch.Tensor, B, H, W, C, kh, kw, pad):
    dx = torch.empty((B, H, W, C), dtype=F32, device=dcol.device)
    _lib.check(_L().mh_col2im_nhwc(_p(dcol), _p(dx), B, H, W, C, kh, kw, pad, dcol.stride(0), _s()), "mh_col2im_nhwc")
    return dx


def relu_pool_fwd(y2d: torch.Tensor, B, H, W, C):
    p = torch.empty((B, H // 2, W // 2, C), dtype=BF16, device=y2d.device)
    _lib.check(_L().mh_relu_maxpool2_fwd(_p(y2d), int(y2d.dtype == F32), y2d.stride(0), _p(p), B, H, W, C, _s()),
               "mh_relu_maxpool2_fwd")
    return p


def relu_pool_bwd(dp: torch.Tensor, y2d: torch.Tensor, B, H, W, C, pad_cols_to: int = 1):
    """dy [B*H*W, C] bf16 (a view of a zero-padded [*, round_up(C,pad_cols_to)] buffer so it can be a GEMM A operand)."""
    cpad = round_up(C, pad_cols_to)
    full = (torch.zeros if cpad != C else torch.empty)((B * H * W, cpad), dtype=BF16, device=y2d.device)
    _lib.check(_L().mh_relu_maxpool2_bwd(_p(dp), _p(y2d), int(y2d.dtype == F32), y2d.stride(0), _p(full),
                                         full.stride(0), B, H, W, C, _s()), "mh_relu_maxpool2_bwd")
    return full[:, :C], full


def conv_pack(Wm: torch.Tensor, bias: Optional[torch.Tensor], out=None):
    Cout, K = Wm.shape
    Kpad = round_up(K + 1, 64)
    if out is None:
        out = torch.empty((Cout, Kpad), dtype=BF16, device=Wm.device)
    _lib.check(_L().mh_conv_pack_weight(_p(Wm), _p(bias), _p(out), Cout, K, Kpad, _s()), "mh_conv_pack_weight")
    return out


def conv_unpack_grad(dWp: torch.Tensor, dW: torch.Tensor, db: Optional[torch.Tensor]):
    Cout, Kpad = dWp.shape
    K = dW.shape[1]
    _lib.check(_L().mh_conv_unpack_grad(_p(dWp), _p(dW), _p(db), Cout, K, Kpad, _s()), "mh_conv_unpack_grad")


# --------------------------------------------------------------------------- optimiser
def adamw_step(p, g, m, v, lr, wd, step, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, shadow=None):
    _lib.check(_L().mh_adamw_step(_p(p), _p(g), _p(m), _p(v), _p(shadow), p.numel(), float(lr), float(beta1),
                                  float(beta2), float(eps), float(wd), int(step), float(grad_scale), _s()),
               "mh_adamw_step")


def adamw_gated(p, g, m, v, lr, wd, used: torch.Tensor, steps: torch.Tensor, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """AdamW on one contiguous range iff the device scalar `used` > 0, with step = device scalar `steps` + 1."""
    _lib.check(_L().mh_adamw_gated(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
                                   float(wd), float(grad_scale), _p(used), _p(steps), _s()), "mh_adamw_gated")


def adamw_bump(used: torch.Tensor, steps: torch.Tensor):
    _lib.check(_L().mh_adamw_bump(_p(used), _p(steps), steps.numel(), _s()), "mh_adamw_bump")


# ---- gradient-norm clipping / non-finite guard: the control block `ctl` (4 doubles: s, norm, apply, skipped) lives on the device
def grad_sumsq_slots(n: int) -> int:
    """fp64 workspace slots grad_sumsq writes for a range of n elements (one per workgroup)."""
    return int(_L().mh_grad_sumsq_slots(int(n)))


def grad_sumsq(g: torch.Tensor, used: torch.Tensor, partials: torch.Tensor) -> int:
    """fp64 sum of squares of the contiguous f32 range g, per workgroup, into the head of `partials` (f64); zeros when the
    device scalar `used` <= 0.  -> the number of slots written."""
    _lib.check(_L().mh_grad_sumsq(_p(g), g.numel(), _p(used), _p(partials), partials.numel(), _s()), "mh_grad_sumsq")
    return grad_sumsq_slots(g.numel())


def clip_rank_sum(partials: torch.Tensor, n_partials: int, rank_sums: torch.Tensor, rank: int):
    _lib.check(_L().mh_clip_rank_sum(_p(partials), int(n_partials), _p(rank_sums), rank_sums.numel(), int(rank), _s()),
               "mh_clip_rank_sum")


def clip_finalize(partials: torch.Tensor, n_partials: int, rank_sums: Optional[torch.Tensor], max_norm: Optional[float],
                  grad_scale: float, guard: bool, ctl: torch.Tensor):
    """Write ctl from the partials (and the per-rank sums).  max_norm None: no clipping, s = (float)grad_scale."""
    if n_partials > partials.numel() or ctl.numel() < 4 or ctl.dtype != torch.float64 or partials.dtype != torch.float64:
        raise _lib.MyriadHipError("clip_finalize: f64 partials / ctl[4] expected")
    _lib.check(_L().mh_clip_finalize(_p(partials), int(n_partials), _p(rank_sums), 0 if rank_sums is None else rank_sums.numel(),
                                     float("inf") if max_norm is None else float(max_norm), float(grad_scale), int(bool(guard)),
                                     _p(ctl), _s()), "mh_clip_finalize")


def adamw_gated_ctl(p, g, m, v, lr, wd, used: torch.Tensor, steps: torch.Tensor, ctl: torch.Tensor, beta1=0.9, beta2=0.999, eps=1e-8):
    """adamw_gated under the control block: nothing when ctl[2] == 0, else the gradient times (float)ctl[0]."""
    _lib.check(_L().mh_adamw_gated_ctl(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
                                       float(wd), _p(used), _p(steps), _p(ctl), _s()), "mh_adamw_gated_ctl")


def adamw_bump_ctl(used: torch.Tensor, steps: torch.Tensor, ctl: torch.Tensor):
    _lib.check(_L().mh_adamw_bump_ctl(_p(used), _p(steps), steps.numel(), _p(ctl), _s()), "mh_adamw_bump_ctl")


# --------------------------------------------------------------------------- vision-expert map heads (K16)
def l2norm_rows(x: torch.Tensor, want_bf16: bool = True, want_f32: bool = False, eps: float = 1e-12):
    """y = x / max(||x||, eps) row-wise; x [M, D] f32 (row stride free)."""
    _chk2d(x, F32, "l2norm_rows.x")
    M, D = x.shape
    yb = torch.empty((M, D), dtype=BF16, device=x.device) if want_bf16 else None
    yf = torch.empty((M, D), dtype=F32, device=x.device) if want_f32 else None
    _lib.check(_L().mh_l2norm_rows(_p(x), x.stride(0), _p(yb), _p(yf), D, M, D, float(eps), _s()), "mh_l2norm_rows")
    return yb, yf


def pair_logits(p: torch.Tensor, text: torch.Tensor, rows_per_batch: int, scale: float = 100.0):
    """p [rows, C] f32, text [B, 2, C] f32 -> [rows, 2] = scale * cos(p, text[row // rows_per_batch])."""
    _chk2d(p, F32, "pair_logits.p")
    rows, C = p.shape
    out = torch.empty((rows, 2), dtype=F32, device=p.device)
    _lib.check(_L().mh_pair_logits(_p(p), p.stride(0), _p(text.contiguous()), _p(out), rows, rows_per_batch, C, float(scale),
                                   _s()), "mh_pair_logits")
    return out


def zs_accumulate(logits: torch.Tensor, mask_acc: torch.Tensor, map_acc: torch.Tensor, w: float):
    B, h, S = mask_acc.shape[0], mask_acc.shape[-1], map_acc.shape[-1]
    _lib.check(_L().mh_zs_accumulate(_p(logits), _p(mask_acc), _p(map_acc), B, h, S, float(w), _s()), "mh_zs_accumulate")


def rowmax_skip(scores: torch.Tensor, acc: torch.Tensor, period: int, w: float):
    """acc[row] += w * max over columns c with c % period != 0 (period 0: all columns)."""
    rows, cols = scores.shape
    _lib.check(_L().mh_rowmax_skip(_p(scores), scores.stride(0), _p(acc), rows, cols, period, float(w), _s()), "mh_rowmax_skip")


def bilinear_ac(x: torch.Tensor, H: int, W: int, one_minus: bool = False):
    """x [B, h, w] f32 -> [B, H, W], align_corners=True; optionally 1 - result."""
    B, h, w = x.shape
    out = torch.empty((B, H, W), dtype=F32, device=x.device)
    _lib.check(_L().mh_bilinear_ac(_p(x.contiguous()), _p(out), B, h, w, H, W, int(one_minus), _s()), "mh_bilinear_ac")
    return out


def bank_sim_chunks(rows: int) -> int:
    """Chunks bank_sim_max splits a class of `rows` bank rows into (a function of the row count alone)."""
    ch = _L().mh_bank_sim_chunk_rows()
    return (int(rows) + ch - 1) // ch


def bank_sim_max(q: torch.Tensor, bank: torch.Tensor, ranges, L: int, q_row0: int = 0, q_sample_rows: Optional[int] = None,
                 out: Optional[torch.Tensor] = None, dev_ranges=None):
    """One tap of the banked one-shot head for a whole batch.  q [*, D] bf16: the query row of sample b, patch l is row
    b * q_sample_rows + q_row0 + l (q_row0 = 1, q_sample_rows = 1 + L skips the class tokens); bank [R, D] bf16; ranges: the B
    host pairs (offset, rows) of each sample's class in the bank.  Returns (part [B, max_chunks, L] f32, (bank_off, bank_rows)
    int32 device arrays): part[b, c] is the max over chunk c of sample b's rows, written for c < bank_sim_chunks(rows_b) only.
    `dev_ranges`: the device arrays of an earlier call with the same ranges (the other taps of a batch)."""
    for t, name in ((q, "bank_sim_max.q"), (bank, "bank_sim_max.bank")):
        _chk2d(t, BF16, name)
        if not t.is_contiguous():
            raise _lib.MyriadHipError(f"{name}: need a contiguous tensor, got strides {t.stride()}")
    ranges = [(int(o), int(r)) for o, r in ranges]
    B, D, R = len(ranges), q.shape[1], bank.shape[0]
    if q_sample_rows is None:
        q_sample_rows = q_row0 + L
    if bank.shape[1] != D:
        raise _lib.MyriadHipError(f"bank_sim_max: q has D = {D}, bank has D = {bank.shape[1]}")
    if B < 1 or L < 1 or q_row0 < 0 or q_sample_rows < q_row0 + L or (B - 1) * q_sample_rows + q_row0 + L > q.shape[0]:
        raise _lib.MyriadHipError(f"bank_sim_max: {B} samples of rows [{q_row0}, {q_row0 + L}) at stride {q_sample_rows} "
                                  f"do not fit q's {q.shape[0]} rows")
    for b, (o, r) in enumerate(ranges):
        if r < 1 or o < 0 or o + r > R:
            raise _lib.MyriadHipError(f"bank_sim_max: sample {b} has the bank range [{o}, {o + r}) of a bank of {R} rows "
                                      "(at least one row, inside the bank)")
    max_chunks = max(bank_sim_chunks(r) for _, r in ranges)
    if dev_ranges is None:
        both = h2d(torch.tensor([[o for o, _ in ranges], [r for _, r in ranges]], dtype=torch.int32), q.device)
        dev_ranges = (both[0], both[1])
    if out is None:
        out = torch.empty((B, max_chunks, L), dtype=F32, device=q.device)
    elif out.dtype != F32 or tuple(out.shape) != (B, max_chunks, L) or not out.is_contiguous():
        raise _lib.MyriadHipError(f"bank_sim_max.out: need contiguous f32 {(B, max_chunks, L)}, got {out.dtype} {tuple(out.shape)}")
    _lib.check(_L().mh_bank_sim_max(_p(q), q_row0, q_sample_rows, _p(bank), _p(dev_ranges[0]), _p(dev_ranges[1]), _p(out), B, L,
                                    D, max_chunks, _s()), "mh_bank_sim_max")
    return out, dev_ranges


def bank_sim_finish(part: torch.Tensor, bank_rows: torch.Tensor, S: int, w: Optional[float] = None):
    """part [T, B, max_chunks, h*h] f32 (bank_sim_max's output of T taps), bank_rows [B] int32 (device) ->
    (sim [B, h, h] = sum_t w * max over chunks (w: 1 / T), simmask [B, h, h] = 1 - sim, amap [B, S, S] = 1 - bilinear_ac(sim))."""
    if part.dtype != F32 or not part.is_cuda or part.dim() != 4 or not part.is_contiguous():
        raise _lib.MyriadHipError(f"bank_sim_finish.part: need contiguous cuda f32 [T, B, chunks, L], got {part.dtype} "
                                  f"{tuple(part.shape)}")
    T, B, max_chunks, L = part.shape
    h = int(round(L ** 0.5))
    if h * h != L:
        raise _lib.MyriadHipError(f"bank_sim_finish: L = {L} patches are not a square grid")
    if bank_rows.dtype != torch.int32 or not bank_rows.is_cuda or bank_rows.numel() != B or not bank_rows.is_contiguous():
        raise _lib.MyriadHipError(f"bank_sim_finish.bank_rows: need {B} contiguous cuda int32, got {bank_rows.dtype} "
                                  f"{tuple(bank_rows.shape)}")
    sim = torch.empty((B, h, h), dtype=F32, device=part.device)
    simmask = torch.empty((B, h, h), dtype=F32, device=part.device)
    amap = torch.empty((B, S, S), dtype=F32, device=part.device)
    _lib.check(_L().mh_bank_sim_finish(_p(part), _p(bank_rows), _p(sim), _p(simmask), _p(amap), T, B, max_chunks, h, S,
                                       float(1.0 / T if w is None else w), _s()), "mh_bank_sim_finish")
    return sim, simmask, amap


class CoresetResult(NamedTuple):
    """coreset_select's outputs, all device tensors: sel int32 [n] (row indices relative to row0, in selection order),
    radius2 f32 [n] (radius2[0] = +inf), cover2 f32 [1], mind f32 [rows] (-1 on the selected rows)."""
    sel: torch.Tensor
    radius2: torch.Tensor
    cover2: torch.Tensor
    mind: torch.Tensor


def coreset_select(taps: Sequence[torch.Tensor], n: int, *, row0: int = 0, rows: Optional[int] = None,
                   start: int = 0) -> CoresetResult:
    """Greedy k-centre (farthest-point) selection of n of the rows [row0, row0 + rows) of `taps`, T contiguous bf16 [R, D]
    matrices that are summed over in the squared distance (csrc/coreset.hip; the rule is DESIGN section 6).  2 n launches, no
    host synchronisation."""
    return _coreset_select_into(None, taps, n, row0, rows, start)


def _coreset_select_into(out: Optional[CoresetResult], taps, n: int, row0: int = 0, rows: Optional[int] = None, start: int = 0):
    """coreset_select writing the four tensors of `out` (the tests frame them in poison); None allocates them."""
    taps = list(taps)
    if not 1 <= len(taps) <= 8:
        raise _lib.MyriadHipError(f"coreset_select: need 1..8 taps, got {len(taps)}")
    for t, x in enumerate(taps):
        _chk2d(x, BF16, f"coreset_select.taps[{t}]")
        if not x.is_contiguous():
            raise _lib.MyriadHipError(f"coreset_select.taps[{t}]: need a contiguous tensor, got strides {x.stride()}")
        if x.shape != taps[0].shape or x.device != taps[0].device:
            raise _lib.MyriadHipError(f"coreset_select.taps[{t}]: {tuple(x.shape)} on {x.device}, taps[0] is "
                                      f"{tuple(taps[0].shape)} on {taps[0].device}")
    R, D = taps[0].shape
    row0, start, n = int(row0), int(start), int(n)
    rows = R - row0 if rows is None else int(rows)
    if D < 8 or D % 8:
        raise _lib.MyriadHipError(f"coreset_select: D = {D} is not a multiple of 8 (16-byte loads)")
    if row0 < 0 or rows < 1 or row0 + rows > R:
        raise _lib.MyriadHipError(f"coreset_select: the class [{row0}, {row0 + rows}) is not a non-empty range of the {R} rows")
    if not 1 <= n <= rows or not 0 <= start < rows:
        raise _lib.MyriadHipError(f"coreset_select: n = {n} outside 1..{rows} or start = {start} outside 0..{rows - 1}")
    dev = taps[0].device
    if out is None:
        out = CoresetResult(torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=F32, device=dev),
                            torch.empty((1,), dtype=F32, device=dev), torch.empty((rows,), dtype=F32, device=dev))
    for t, dt, shape, name in ((out.sel, torch.int32, (n,), "sel"), (out.radius2, F32, (n,), "radius2"),
                               (out.cover2, F32, (1,), "cover2"), (out.mind, F32, (rows,), "mind")):
        if t.dtype != dt or not t.is_cuda or tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.MyriadHipError(f"coreset_select.out.{name}: need contiguous cuda {dt} {shape}, got {t.dtype} {tuple(t.shape)}")
    ws_bytes = _L().mh_coreset_ws_bytes(rows)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    ptrs = (ctypes.c_void_p * len(taps))(*(x.data_ptr() for x in taps))
    _lib.check(_L().mh_coreset_select(ptrs, len(taps), D, D, row0, rows, n, start, _p(out.sel), _p(out.radius2), _p(out.mind),
                                      _p(out.cover2), _p(ws), ws_bytes, _s()), f"mh_coreset_select T={len(taps)} D={D} rows={rows}")
    return out


SEG_HIST_BINS = 1 << 20      # keys of seg_hist_update: the top 20 bits of the order-preserving transform of the fp32 bits
SEG_MAX_PIXELS = 65536       # mask_components keeps one image's union-find in LDS


def _chk_masks(masks: torch.Tensor, name: str):
    if masks.dtype not in (torch.uint8, torch.bool) or not masks.is_cuda or masks.dim() != 3 or not masks.is_contiguous():
        raise _lib.MyriadHipError(f"{name}: need contiguous cuda uint8 / bool [B, H, W], got {masks.dtype} {tuple(masks.shape)} "
                                  f"cuda={masks.is_cuda}")
    B, H, W = masks.shape
    if B < 1 or H < 1 or W < 1:
        raise _lib.MyriadHipError(f"{name}: empty shape {tuple(masks.shape)}")
    if H * W > SEG_MAX_PIXELS or _L().mh_mask_components_lds_bytes(H, W) < 0:
        raise _lib.MyriadHipError(f"{name}: an image of {H} x {W} does not fit one workgroup's LDS (H * W <= {SEG_MAX_PIXELS}, "
                                  "both sides >= 4 or few enough 2 x 2 blocks)")
    return B, H, W


def mask_components(masks: torch.Tensor, out=None):
    """8-connected components of binary masks [B, H, W] (uint8 / bool, nonzero = anomalous) -> (labels [B, H, W] int32: -1 on
    background, else the smallest linear index y * W + x of the pixel's component; area [B, H, W] int32: the component's pixel
    count at that pixel, 0 elsewhere; n_regions [B] int32).  `out`: the three tensors to write.  H * W <= 65536."""
    B, H, W = _chk_masks(masks, "mask_components.masks")
    if out is None:
        out = (torch.empty((B, H, W), dtype=torch.int32, device=masks.device),
               torch.empty((B, H, W), dtype=torch.int32, device=masks.device),
               torch.empty((B,), dtype=torch.int32, device=masks.device))
    labels, area, n_regions = out
    for t, shape, name in ((labels, (B, H, W), "labels"), (area, (B, H, W), "area"), (n_regions, (B,), "n_regions")):
        if t.dtype != torch.int32 or not t.is_cuda or tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.MyriadHipError(f"mask_components.{name}: need contiguous cuda int32 {shape}, got {t.dtype} {tuple(t.shape)}")
    _lib.check(_L().mh_mask_components(_p(masks), _p(labels), _p(area), _p(n_regions), B, H, W, _s()), "mh_mask_components")
    return labels, area, n_regions


def seg_hist_update(hist: torch.Tensor, counters: torch.Tensor, maps: torch.Tensor, masks: torch.Tensor, labels: torch.Tensor,
                    area: torch.Tensor, aggregate: bool = True) -> None:
    """hist [3, 2^20] int64 and counters [4] int64 += the batch: maps [B, H, W] f32 / bf16 scores, masks [B, H, W] uint8 / bool,
    labels / area: mask_components(masks).  Rows: normal pixels per key, anomalous pixels per key, floor(2^40 / region area) per
    anomalous pixel; counters: pixels, anomalous pixels, regions, non-finite scores (those reach no histogram row).  Integer
    atomics: bitwise reproducible.  `aggregate`: equal keys of a wave add once (False: one atomic per lane; same result)."""
    B, H, W = _chk_masks(masks, "seg_hist_update.masks")
    if hist.dtype != torch.int64 or not hist.is_cuda or tuple(hist.shape) != (3, SEG_HIST_BINS) or not hist.is_contiguous():
        raise _lib.MyriadHipError(f"seg_hist_update.hist: need contiguous cuda int64 {(3, SEG_HIST_BINS)}, got {hist.dtype} "
                                  f"{tuple(hist.shape)}")
    if counters.dtype != torch.int64 or not counters.is_cuda or tuple(counters.shape) != (4,) or not counters.is_contiguous():
        raise _lib.MyriadHipError(f"seg_hist_update.counters: need contiguous cuda int64 (4,), got {counters.dtype} "
                                  f"{tuple(counters.shape)}")
    if maps.dtype not in (F32, BF16) or not maps.is_cuda or tuple(maps.shape) != (B, H, W) or not maps.is_contiguous():
        raise _lib.MyriadHipError(f"seg_hist_update.maps: need contiguous cuda f32 / bf16 {(B, H, W)}, got {maps.dtype} "
                                  f"{tuple(maps.shape)}")
    for t, name in ((labels, "labels"), (area, "area")):
        if t.dtype != torch.int32 or not t.is_cuda or tuple(t.shape) != (B, H, W) or not t.is_contiguous():
            raise _lib.MyriadHipError(f"seg_hist_update.{name}: need contiguous cuda int32 {(B, H, W)}, got {t.dtype} "
                                      f"{tuple(t.shape)}")
    _lib.check(_L().mh_seg_hist_update(_p(hist), _p(counters), _p(maps), int(maps.dtype == BF16), _p(masks), _p(labels), _p(area),
                                       B, H, W, int(bool(aggregate)), _s()), "mh_seg_hist_update")


def gemm_residual_rmsnorm(a: torch.Tensor, b: torch.Tensor, residual: torch.Tensor, norm_w: torch.Tensor, eps: float,
                          y_out: Optional[torch.Tensor] = None):
    """(h, y): h = a @ b^T + residual (f32), y = rmsnorm(h) * norm_w (bf16; y_out may be a [M, N] view of a wider buffer).
    One launch less than gemm + rmsnorm_fwd when the GEMM is split along K; bit-identical results either way."""
    _chk2d(a, BF16, "gemm_residual_rmsnorm.a")
    _chk2d(b, BF16, "gemm_residual_rmsnorm.b")
    _chk2d(residual, F32, "gemm_residual_rmsnorm.residual")
    M, K = a.shape
    N = b.shape[0]
    h = torch.empty((M, N), dtype=F32, device=a.device)
    y = y_out if y_out is not None else torch.empty((M, N), dtype=BF16, device=a.device)
    _chk2d(y, BF16, "gemm_residual_rmsnorm.y")
    rc = _L().mh_gemm_residual_rmsnorm(_p(a), a.stride(0), _p(b), b.stride(0), _p(h), N, _p(residual), residual.stride(0),
                                       _p(norm_w), float(eps), _p(y), y.stride(0), M, N, K, _s())
    _lib.check(rc, f"mh_gemm_residual_rmsnorm M={M} N={N} K={K}")
    return h, y


def gemm_residual_layernorm(a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor], residual: torch.Tensor,
                            norm_w: torch.Tensor, norm_b: torch.Tensor, eps: float):
    """(h, y): h = a @ b^T + bias + residual (f32), y = layernorm(h) * norm_w + norm_b (bf16).  Pre-LN ViT blocks."""
    _chk2d(a, BF16, "gemm_residual_layernorm.a")
    _chk2d(b, BF16, "gemm_residual_layernorm.b")
    _chk2d(residual, F32, "gemm_residual_layernorm.residual")
    M, K = a.shape
    N = b.shape[0]
    h = torch.empty((M, N), dtype=F32, device=a.device)
    y = torch.empty((M, N), dtype=BF16, device=a.device)
    rc = _L().mh_gemm_residual_layernorm(_p(a), a.stride(0), _p(b), b.stride(0), _p(h), N, _p(bias), _p(residual),
                                         residual.stride(0), _p(norm_w), _p(norm_b), float(eps), _p(y), M, N, K, _s())
    _lib.check(rc, f"mh_gemm_residual_layernorm M={M} N={N} K={K}")
    return h, y
