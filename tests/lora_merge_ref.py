"""Reference of the q/v LoRA merge of the decode token step (LlamaHIP.decode_merge_lora, csrc/lora_merge.hip).

Merged rule, for the frozen qkv weight W [3D, D] (rows q | k | v, bf16 values), the fp32 masters A_q | A_v [2r, D], B_q, B_v [D, r]
and s = alpha / r (fp32):
    q rows n < D:        M[n, k] = bf16(W[n, k] + s * acc),  acc = 0 + B_q[n, 0] * A_q[0, k] + ... + B_q[n, r-1] * A_q[r-1, k]
    k rows D <= n < 2D:  M[n, k] = W[n, k]
    v rows n >= 2D:      the q rule with B_v[n - 2D] and A_v
every product and sum a separate fp32 operation rounded to nearest even, left to right, then one round-to-nearest-even to bf16.
merge_rows below is that rule in torch fp32 (elementwise ops, no fused multiply-add), so it gives the kernel's bits.

The decode reference of the merged step is tests/fp8_ref.greedy_decode with the exact LoRA in the prefill (the oracle's
llama_layer applies LoRA wherever the state dict holds lora_A / lora_B keys) and, for every later step, a state dict whose q/v
weights are the merged ones and that holds no LoRA keys (merged_step_state_dict)."""
from __future__ import annotations

from typing import Dict

import torch

from tests import fp8_ref as F

ORACLE_LAYERS = "llama_model.model.layers."


def merge_rows(w: torch.Tensor, a_qv: torch.Tensor, b_q: torch.Tensor, b_v: torch.Tensor, s: float) -> torch.Tensor:
    """The merged [3D, D] bf16 matrix by the rule above (CPU, torch fp32)."""
    N, D = w.shape
    r = a_qv.shape[0] // 2
    sf = torch.tensor(float(s), dtype=torch.float32)
    out = w.to(torch.bfloat16).clone()
    for part, b, a in ((0, b_q, a_qv[:r]), (2, b_v, a_qv[r:])):
        b, a = b.float(), a.float()
        acc = torch.zeros((D, D), dtype=torch.float32)
        for j in range(r):
            acc = acc + b[:, j:j + 1] * a[j:j + 1, :]
        rows = slice(part * D, (part + 1) * D)
        out[rows] = (w[rows].float() + sf * acc).to(torch.bfloat16)
    return out


def merge_float64(w: torch.Tensor, a_qv: torch.Tensor, b_q: torch.Tensor, b_v: torch.Tensor, s: float) -> torch.Tensor:
    """W + s * B A in float64 (the exact value the bf16 result approximates), [3D, D]."""
    N, D = w.shape
    r = a_qv.shape[0] // 2
    out = w.double().clone()
    out[:D] += float(s) * (b_q.double() @ a_qv[:r].double())
    out[2 * D:] += float(s) * (b_v.double() @ a_qv[r:].double())
    return out


def fp32_sum_bound(a_qv: torch.Tensor, b_q: torch.Tensor, b_v: torch.Tensor, s: float, D: int) -> torch.Tensor:
    """[3D, D] float64 bound on the fp32 rounding of the rank-r sum before the bf16 rounding: (r + 2) * 2^-24 * s * sum_j |B| |A|
    (zero on the k rows).  It exceeds half a bf16 ulp only where W and s * B A nearly cancel."""
    r = a_qv.shape[0] // 2
    out = torch.zeros((3 * D, D), dtype=torch.float64)
    out[:D] = b_q.double().abs() @ a_qv[:r].double().abs()
    out[2 * D:] = b_v.double().abs() @ a_qv[r:].double().abs()
    return out * (float(s) * (r + 2) * 2.0 ** -24)


def ulp_distance(m: torch.Tensor, exact: torch.Tensor) -> torch.Tensor:
    """|m - exact| in bf16 ulps of exact (float64)."""
    return (m.double() - exact).abs() / F.bf16_ulp(exact)


def qkv_of(sd: Dict[str, torch.Tensor], i: int) -> torch.Tensor:
    """Layer i's [3D, D] q | k | v weight from an oracle state dict."""
    p = f"{ORACLE_LAYERS}{i}.self_attn."
    return torch.cat([sd[p + n + ".weight"] for n in ("q_proj", "k_proj", "v_proj")], 0)


def lora_of(sd: Dict[str, torch.Tensor], i: int):
    """(A_q | A_v [2r, D], B_q, B_v) of layer i from an oracle state dict with LoRA keys."""
    p = f"{ORACLE_LAYERS}{i}.self_attn."
    a = torch.cat([sd[p + "q_proj.lora_A.default.weight"], sd[p + "v_proj.lora_A.default.weight"]], 0)
    return a, sd[p + "q_proj.lora_B.default.weight"], sd[p + "v_proj.lora_B.default.weight"]


def merged_step_state_dict(sd: Dict[str, torch.Tensor], n_layers: int, s: float) -> Dict[str, torch.Tensor]:
    """sd with every layer's q/v weights replaced by the merged ones (as float values of bf16) and its LoRA keys dropped: the
    weights of the merged token step."""
    out = {k: v for k, v in sd.items() if ".lora_" not in k}
    for i in range(n_layers):
        D = sd[f"{ORACLE_LAYERS}{i}.self_attn.q_proj.weight"].shape[0]
        m = merge_rows(qkv_of(sd, i).to(torch.bfloat16), *lora_of(sd, i), s).float()
        p = f"{ORACLE_LAYERS}{i}.self_attn."
        out[p + "q_proj.weight"], out[p + "v_proj.weight"] = m[:D], m[2 * D:]
    return out
