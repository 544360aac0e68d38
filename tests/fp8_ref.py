"""Reference of the FP8 (e4m3fn) weight-only decode step (LlamaHIP.decode_fp8, csrc/gemv.hip mh_gemv_pack_fp8).

Quantisation, per output row n of a bf16 matrix W [N, K]:
    amax_n = max_k |W[n, k]|,   s_n = amax_n / 448 (fp32, correctly rounded; 1 for an all-zero row),
    q[n, k] = e4m3fn(clamp(W[n, k] / s_n, -448, 448))   (fp32 division, round to nearest even).
torch's float -> float8_e4m3fn cast rounds to nearest even but gives NaN past the largest finite value, and amax / s can round
just above 448: the clamp comes first.  Dequantisation is q.float() * s_n (fp32; in float64 the product is exact).

The decode loop below is the oracle's greedy loop (oracle.myriad_ref.llama_model + lm_head arg-max) with the prefill on the bf16
weights and every later step on the dequantised copies of the matrices the packed token step streams as fp8."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from oracle import myriad_ref as R

E4M3_MAX = 448.0
# the 254 finite e4m3fn codes (0x7F and 0xFF are NaN)
FINITE_CODES = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)


def to_e4m3fn(x: torch.Tensor) -> torch.Tensor:
    """e4m3fn codes (uint8) of fp32 values: nearest even, saturated to +-448."""
    return x.float().clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def quantize_rows(w: torch.Tensor):
    """(q uint8 [N, K], s float32 [N]) of the rule above, for w [N, K] (bf16 or its exact float values)."""
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    s = amax / E4M3_MAX
    s = torch.where(amax > 0, s, torch.ones_like(s))
    return to_e4m3fn(wf / s[:, None]), s


def decode_codes(q: torch.Tensor) -> torch.Tensor:
    """float32 values of e4m3fn codes (uint8)."""
    return q.view(torch.float8_e4m3fn).float()


def dequantize(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    return decode_codes(q) * s[:, None]


def fp8_round_trip(w: torch.Tensor) -> torch.Tensor:
    """The weights the fp8 token step multiplies by: dequantize(quantize_rows(bf16(w)))."""
    q, s = quantize_rows(w.to(torch.bfloat16))
    return dequantize(q, s)


# ---- stream order of the packed copy (mh_gemv_pack / mh_gemv_pack_fp8)
def packed_nw(N: int) -> int:
    """Waves per workgroup of the packed kernels: 8 when N / 16 workgroups under-fill the chip, else 4."""
    return 8 if (N + 15) // 16 < 512 else 4


def unpack_fp8(data: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """[ceil(N/16)*16, nw*per*64] uint8 codes from the packed bytes: the 16 B lane (lr, lg) of wave w reads at step t hold
    row 16 * block + lr, k = 64 (w * per + t) + 16 lg .. +15, at ((block * nw + w) * per + t) * 1 KiB + (16 lg + lr) * 16."""
    nw = packed_nw(N)
    per = (K // 64 + nw - 1) // nw
    nblk = (N + 15) // 16
    v = data.view(nblk, nw, per, 4, 16, 16)                  # block, wave, step, lg, lr, byte
    return v.permute(0, 4, 1, 2, 3, 5).reshape(nblk * 16, nw * per * 64)


# ---- decode loop
MATS_FP8 = ("self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
MATS_QKV = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")


def fp8_state_dict(sd: Dict[str, torch.Tensor], qkv: bool = True, prefix: str = "llama_model.model.") -> Dict[str, torch.Tensor]:
    """sd with the decoder-layer matrices the fp8 step streams replaced by their fp8 round trip (q/k/v only when `qkv`: with LoRA
    attached the bordered qkv product stays bf16)."""
    out = dict(sd)
    names = MATS_FP8 + (MATS_QKV if qkv else ())
    i = 0
    while f"{prefix}layers.{i}.input_layernorm.weight" in sd:
        for n in names:
            k = f"{prefix}layers.{i}.{n}.weight"
            out[k] = fp8_round_trip(sd[k])
        i += 1
    return out


def greedy_decode(sd: Dict[str, torch.Tensor], sd_step: Dict[str, torch.Tensor], emb: torch.Tensor, heads: int,
                  max_new_tokens: int, lora: Optional[dict] = None, eos_id: int = 2, min_length: int = 1, eps: float = 1e-6,
                  prefix: str = "llama_model."):
    """Greedy ids [B, T] with the prefill on `sd` and every single-token step on `sd_step`, plus per step the logits [B, T, V],
    the top-1 / top-2 margin and the largest finite |logit|.  EOS is banned while fewer than `min_length` ids were generated and
    the loop ends once every row has emitted it (LlamaHIP.greedy_generate without stop sequences; rows are not padded)."""
    B, S0, _ = emb.shape
    ew = sd[prefix + "model.embed_tokens.weight"]
    lm = sd[prefix + "lm_head.weight"]
    past, x, total = None, emb, S0
    done = torch.zeros(B, dtype=torch.bool)
    ids, logits_all, margins, scales = [], [], [], []
    for step in range(max_new_tokens):
        pos = None if past is None else torch.full((B, 1), total - 1, dtype=torch.long)
        hidden, past = R.llama_model(sd if past is None else sd_step, x, torch.ones(B, total), heads, eps, position_ids=pos,
                                     past=past, prefix=prefix + "model.", lora=lora)
        logits = torch.nn.functional.linear(hidden[:, -1], lm)
        if step < min_length:
            logits[:, eos_id] = -float("inf")
        top2 = logits.topk(2, dim=-1).values
        margins.append(top2[:, 0] - top2[:, 1])
        scales.append(torch.where(torch.isfinite(logits), logits, torch.zeros_like(logits)).abs().amax(-1))
        logits_all.append(logits)
        nxt = logits.argmax(-1)
        ids.append(nxt)
        done |= nxt == eos_id
        if bool(done.all()):
            break
        x = ew[nxt][:, None]
        total += 1
    return torch.stack(ids, 1), torch.stack(logits_all, 1), torch.stack(margins, 1), torch.stack(scales, 1)


def two_ulp_horizon(margins: torch.Tensor, scales: torch.Tensor) -> int:
    """Steps before the first one whose reference top-2 margin is below two bf16 ulps of its logit scale (2 * 2^-7 * max|logit|),
    over all rows: up to there a correct bf16-activation decode must pick the same ids."""
    near = (margins < 2.0 * 2.0 ** -7 * scales).any(0)
    return int(near.nonzero()[0]) if bool(near.any()) else margins.shape[1]


def e4m3_value(code: int) -> float:
    """Hand decoding of one e4m3fn code (sign, 4 exponent bits with bias 7, 3 mantissa bits; exponent 0 is subnormal)."""
    sign = -1.0 if code & 0x80 else 1.0
    e, m = (code >> 3) & 0xF, code & 7
    if e == 0:
        return sign * m * 2.0 ** -9
    return sign * (1.0 + m / 8.0) * 2.0 ** (e - 7)


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """One bf16 ulp at |x| (8 significant bits), for x != 0; the smallest normal's ulp at 0."""
    ax = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(ax)) - 7)

