"""Reference of the MXFP4 weight-only decode step (LlamaHIP.decode_fp4, csrc/gemv.hip mh_gemv_pack_fp4).

The format (include/myriad_hip.h), for W [N, K] bf16, finite, blocks of 32 consecutive k within a row:
    E = biased bf16 exponent field of the block's largest |w| (0 for a zero or subnormal maximum),
    b = max(2, E - 2) the scale byte, X = 2^(b-127),
    code = sign | index into E2M1 of w / X rounded to nearest, ties to the even code, saturated at +-6; sign bit copied from w,
    dq = code * X.
The quantiser below works on the bf16 bit patterns in integer arithmetic only (no float rounding mode or denormal setting bears
on it) and picks each code by a nearest-value search, not by the kernel's midpoint count.

The decode loop is tests/fp8_ref.py's (prefill on the bf16 weights, every later step on the dequantised copies)."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from tests import fp8_ref as F8

E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
BLOCK = 32
_FRAC = 15                                           # ratios are held as integers in units of 2^-15
_E2M1_FIX = np.array([int(v * 2 ** _FRAC) for v in E2M1], dtype=np.int64)


def bf16_bits(w: torch.Tensor) -> np.ndarray:
    """int64 array of the 16-bit patterns of w (bf16, or float values that are exactly bf16)."""
    wb = w.to(torch.bfloat16)
    assert torch.equal(wb.float(), w.float()), "values must be bf16-representable"
    return wb.contiguous().view(torch.int16).numpy().astype(np.int64) & 0xFFFF


def _nearest_code(r: np.ndarray) -> np.ndarray:
    """Index into E2M1 of the value nearest to r * 2^-15 (integer r >= 0), an exact tie going to the even code; values past 6
    land on 6."""
    dist = np.abs(r[..., None] - _E2M1_FIX)                        # exact integers
    cost = 2 * dist + (np.arange(8) & 1)
    return cost.argmin(axis=-1)


_R_MAX = 255 << 10                                                # the largest ratio: sig = 255 at d = 2
_NEAREST = _nearest_code(np.arange(_R_MAX + 1, dtype=np.int64)).astype(np.uint8)      # the search, once per possible ratio


def quantize_blocks(w: torch.Tensor, chunk: int = 1024):
    """(codes uint8 [N, K] in 0..15, scale bytes uint8 [N, K / 32]) of the rule above; K % 32 == 0.  Rows go through in chunks."""
    N, K = w.shape
    assert K % BLOCK == 0
    codes = np.empty((N, K), dtype=np.uint8)
    sb = np.empty((N, K // BLOCK), dtype=np.uint8)
    for n0 in range(0, N, chunk):
        bits = bf16_bits(w[n0:n0 + chunk]).astype(np.int32)
        n = bits.shape[0]
        mag = bits & 0x7FFF
        e = mag >> 7
        sig = np.where(e > 0, 128 | (mag & 127), mag & 127)       # |w| = sig * 2^(max(e, 1) - 134)
        ee = np.maximum(e, 1)
        E = (mag.reshape(n, K // BLOCK, BLOCK).max(axis=2)) >> 7   # exponent field of the largest magnitude
        b = np.maximum(2, E - 2)
        # |w| / X = sig * 2^(ee - 134 - (b - 127)) = sig * 2^(d - 7), d = ee - b <= 2.  In units of 2^-15: sig << (d + 8); below
        # d = -8 the ratio is under 2^-7 and the nearest code is 0 whatever the rest, so d is clamped there.
        d = ee - np.repeat(b, BLOCK, axis=1)
        assert int(d.max(initial=-999)) <= 2
        r = sig << (np.maximum(d, -8) + 8)
        codes[n0:n0 + n] = ((bits >> 12) & 8) | _NEAREST[r]
        sb[n0:n0 + n] = b
    return torch.from_numpy(codes), torch.from_numpy(sb)


def decode_codes(codes: torch.Tensor) -> torch.Tensor:
    """float64 values of e2m1 codes (sign | index)."""
    c = codes.long()
    v = torch.tensor(E2M1, dtype=torch.float64)[c & 7]
    return torch.where((c & 8) != 0, -v, v)


def scale_values(b: torch.Tensor) -> torch.Tensor:
    """float64 2^(b-127)."""
    return torch.exp2(b.double() - 127.0)


def dequantize(codes: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """float64 code * 2^(b-127), exact."""
    return decode_codes(codes) * scale_values(b).repeat_interleave(BLOCK, dim=1)


def fp4_round_trip(w: torch.Tensor) -> torch.Tensor:
    """The float32 weights the fp4 token step multiplies by: dequantize(quantize_blocks(bf16(w))).  A K that is no multiple of
    32 is padded with zeros first, as the model pads its intermediate size (zero columns leave a block's maximum alone)."""
    wb = w.to(torch.bfloat16)
    K = wb.shape[1]
    Kp = (K + BLOCK - 1) // BLOCK * BLOCK
    if Kp != K:
        wb = torch.cat([wb, torch.zeros(wb.shape[0], Kp - K, dtype=wb.dtype)], 1)
    dq = dequantize(*quantize_blocks(wb))[:, :K]
    out = dq.float()
    assert torch.equal(out.double(), dq)
    return out


# ---- stream order of the packed copy (mh_gemv_pack_fp4)
def packed_dims(N: int, K: int):
    """(nblk, nw, per, per4): 16-row blocks, waves per workgroup, 128-deep steps per wave, scale dwords per lane and wave."""
    nw = F8.packed_nw(N)
    per = (K // 128 + nw - 1) // nw
    return (N + 15) // 16, nw, per, (per + 3) // 4


def unpack_fp4(data: torch.Tensor, scales: torch.Tensor, N: int, K: int):
    """(codes uint8 [ceil(N/16)*16, nw*per*128], scale bytes uint8 [same rows, nw*per*4], pad scale bytes) from the packed
    streams.  Codes: the 16 B lane (lr, lg) of wave w reads at step t hold row 16 block + lr, k = 128 (w per + t) + 32 lg .. +31,
    two per byte with the lower k in the low nibble, at ((block nw + w) per + t) KiB + (16 lg + lr) * 16.  Scale bytes: that
    lane's at ((block nw + w) per4 + t / 4) * 256 + (16 lg + lr) * 4 + t % 4; `pad` are the bytes of steps per .. 4 per4 - 1."""
    nblk, nw, per, per4 = packed_dims(N, K)
    assert data.numel() == nblk * nw * per * 1024 and scales.numel() == nblk * nw * per4 * 256
    v = data.view(nblk, nw, per, 4, 16, 16)                          # block, wave, step, lg, lr, byte
    by = v.permute(0, 4, 1, 2, 3, 5).reshape(nblk * 16, nw * per * 64)
    codes = torch.stack([by & 15, by >> 4], dim=-1).reshape(nblk * 16, nw * per * 128)
    s = scales.view(nblk, nw, per4, 4, 16, 4)                        # block, wave, step / 4, lg, lr, step % 4
    s = s.permute(0, 4, 1, 2, 5, 3).reshape(nblk * 16, nw, per4 * 4, 4)   # row, wave, step, lg
    return codes, s[:, :, :per].reshape(nblk * 16, nw * per * 4), s[:, :, per:].reshape(-1)


# ---- decode loop
def fp4_state_dict(sd: Dict[str, torch.Tensor], qkv: bool = True, prefix: str = "llama_model.model.") -> Dict[str, torch.Tensor]:
    """sd with the decoder-layer matrices the fp4 step streams replaced by their fp4 round trip (q/k/v only when `qkv`: with the
    bordered LoRA the qkv product stays bf16)."""
    out = dict(sd)
    names = F8.MATS_FP8 + (F8.MATS_QKV if qkv else ())
    i = 0
    while f"{prefix}layers.{i}.input_layernorm.weight" in sd:
        for n in names:
            k = f"{prefix}layers.{i}.{n}.weight"
            out[k] = fp4_round_trip(sd[k])
        i += 1
    return out


greedy_decode = F8.greedy_decode
two_ulp_horizon = F8.two_ulp_horizon
bf16_ulp = F8.bf16_ulp
