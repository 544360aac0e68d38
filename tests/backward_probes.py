"""Backward probes: inputs and cotangents that are nonzero in ONE token row, so that the gradients they reach consist of that
row's contribution alone, and the float64 (LLaMA: float32, see LlamaRef) references they are compared with.  Needs no device.

Backward is linear in the cotangent.  A weight gradient is a sum over token rows, so under a dense cotangent one row carries
about 1/sqrt(M) of its norm and the project's gate (rel < 6e-2 and cos > 0.998 per tensor) cannot see a backward that loses it.
With the cotangent (or a free input) nonzero in a single row, a *localised part* -- a gradient tensor, or a slice of one, that
only that row feeds -- is lost whole when the row is lost: relative error 1.0 against the same 6e-2.  Which parts are localised
is argued beside each list below and proved on the reference by tests/test_backward_probes_cpu.py (rank one, non-zero).

Every reference runs the oracle's forward once per input and back-propagates each cotangent through the kept graph.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Tuple

import torch

from oracle import myriad_ref as R
from tests import golden_utils as gu

BF16, F64 = torch.bfloat16, torch.float64
REL, COS = 6e-2, 0.998                  # the project's gradient gate (tests/test_vit_train_gpu.py::_check_grads)
LLAMA_DEMB, LLAMA_LORA, LLAMA_LOSS = 5e-2, 6e-2, 3e-3      # tests/test_model_gpu.py::test_llama_lora_qv_vs_oracle
ZERO_ROW = 2.0 ** -20                   # of max |demb|: forgives a zero formed through a rounded cancellation, nothing more


# ------------------------------------------------------------------------------------------------ measures
def rel_cos(got: torch.Tensor, want: torch.Tensor, scale=None) -> Tuple[float, float]:
    """(relative L2 error, cosine) of one tensor; `scale` replaces the reference's own norm where its exact value is zero."""
    got, want = got.detach().double().cpu().reshape(-1), want.detach().double().cpu().reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    n = want.norm() if scale is None else scale
    return float((got - want).norm() / (n + 1e-30)), float((got @ want) / (got.norm() * want.norm() + 1e-30))


def row_rel_cos(got: torch.Tensor, want: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """rel_cos of every row of a [rows, D] pair."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape and got.dim() == 2, (got.shape, want.shape)
    rel = (got - want).norm(dim=1) / (want.norm(dim=1) + 1e-30)
    cos = (got * want).sum(1) / (got.norm(dim=1) * want.norm(dim=1) + 1e-30)
    return rel, cos


def max_relerr(got: torch.Tensor, want: torch.Tensor) -> float:
    """tests/test_model_gpu.py::relerr: max-abs error over the reference's max-abs."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max() / (want.abs().max() + 1e-30))


def rank_one_residual(G: torch.Tensor, seed: int = 0) -> float:
    """|| G - (G v)(u^T G) / (u^T G v) || / || G || with random u, v: zero exactly when G has rank one."""
    g = torch.Generator().manual_seed(seed)
    G = G.detach().double().reshape(G.shape[0], -1)
    u = torch.randn(G.shape[0], generator=g, dtype=F64)
    v = torch.randn(G.shape[1], generator=g, dtype=F64)
    Gv, uG = G @ v, u @ G
    return float((G - torch.outer(Gv, uG) / (u @ Gv)).norm() / G.norm())


def min_row_norm_over_median(rows: torch.Tensor) -> float:
    n = rows.detach().double().norm(dim=1)
    return float(n.min() / n.median())


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------------------------------------ ViT
VIT_D, VIT_HD, VIT_P, VIT_TOK, VIT_HEADS, VIT_EPS = 1408, 6144, 14, 257, 16, 1e-6
VIT_BATCHES = (1, 2, 3)                         # M = 257, 514, 771: one row, two rows, three rows past the 256-row tiles
VIT_COT_TOKENS = (0, 1, 255, 256)               # cls, the first patch, the last row of a 256-row tile, the row past it
VIT_PATCHES = (0, 254, 255)                     # token rows 1, 255, 256
# Under a cotangent in row (b, t) of the LAST block's output:  out = x1 + fc2(gelu(fc1(LN2(x1)))),  x1 = x0 + proj(attn(LN1(x0))).
# fc2, gelu, fc1, LN2, the residual, proj and d(attention output) -> dq act on each row alone, so dY of fc2, fc1, proj and the q
# columns of qkv is nonzero in that row only: those weight gradients are one outer product, their biases / LayerNorm parameters
# that row's term.  dk and dv reach every row of sample b, so the k / v thirds and everything below them are spread.
_VIT_LOCAL = ("mlp.fc2.weight", "mlp.fc2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "norm2.weight", "norm2.bias",
              "attn.proj.weight", "attn.proj.bias", "attn.q_bias")


def vit_weights(depth: int, seed: int = 5) -> Dict[str, torch.Tensor]:
    from tests.test_vit_train_gpu import _vit_weights
    return _vit_weights(depth, seed=seed)


def vit_samples(B: int) -> List[int]:
    return sorted({0, B - 1})


def vit_image(B: int) -> torch.Tensor:
    return _randn((max(VIT_BATCHES), 3, 224, 224), 21)[:B].contiguous()


def vit_dense_cot(B: int) -> torch.Tensor:
    return _randn((max(VIT_BATCHES), VIT_TOK, VIT_D), 22, 0.1)[:B].contiguous()


def vit_row_cot(B: int, b: int, t: int) -> torch.Tensor:
    dout = torch.zeros(B, VIT_TOK, VIT_D)
    dout[b, t] = _randn((VIT_D,), 7000 + 1000 * b + t, 0.1)
    return dout


def vit_patch_image(B: int, b: int, p: int) -> torch.Tensor:
    """Zero but for the 14 x 14 patch p (row-major over the 16 x 16 grid: token row p + 1) of sample b."""
    image = torch.zeros(B, 3, 224, 224)
    y, x = (p // 16) * VIT_P, (p % 16) * VIT_P
    image[b, :, y:y + VIT_P, x:x + VIT_P] = _randn((3, VIT_P, VIT_P), 8000 + 1000 * b + p)
    return image


def vit_split(grads: Dict[str, torch.Tensor], local_block: Optional[int]):
    """(localised parts, ordinary tensors) of a ViT gradient dict under a one-row cotangent; the qkv weight of the localised
    block is cut into its q third (localised) and its k|v thirds (ordinary).  local_block None: everything is ordinary."""
    local, rest = {}, {}
    for n, g in grads.items():
        blk = f"blocks.{local_block}."
        if local_block is not None and blk in n:
            if n.endswith(_VIT_LOCAL):
                local[n] = g
                continue
            if n.endswith("attn.qkv.weight"):
                local[n + "[q]"] = g[:VIT_D]
                rest[n + "[kv]"] = g[VIT_D:]
                continue
        rest[n] = g
    return local, rest


class VitRef:
    """float64 autograd through R.vit_forward, the GEMM weights rounded to bf16 as the kernels hold them
    (tests/test_vit_train_gpu.py::_ref_grads).  The oracle never mixes samples, so the batch is a sum of per-sample graphs:
    each sample is run forward once, and a sample whose cotangent is all zero adds exactly zero and is not walked.  Built on
    `samples` only, it returns those samples' share of the gradients."""

    def __init__(self, sd: Dict[str, torch.Tensor], image: torch.Tensor, samples=None):
        self.leaves = {}
        for k, t in sd.items():
            t = t.double()
            if k.endswith(("qkv.weight", "proj.weight", "fc1.weight", "fc2.weight")):
                t = t.to(BF16).double()
            self.leaves[k] = t.requires_grad_(True)
        self.B = image.shape[0]
        self.outs = {}
        for b in (range(self.B) if samples is None else samples):
            self.outs[b] = R.vit_forward(self.leaves, image[b:b + 1].double(), num_heads=VIT_HEADS, eps=VIT_EPS)

    def grads(self, dout: torch.Tensor, skip_zero: bool = True) -> Dict[str, torch.Tensor]:
        names = list(self.leaves)
        total = {n: torch.zeros_like(self.leaves[n]) for n in names}
        for b in self.outs:
            if skip_zero and not bool(dout[b].any()):
                continue
            gs = torch.autograd.grad(self.outs[b], [self.leaves[n] for n in names], dout[b:b + 1].double(), retain_graph=True)
            for n, g in zip(names, gs):
                total[n] += g
        return total


@functools.lru_cache(maxsize=None)
def vit_ref(depth: int, B: int, only_last: bool = False) -> VitRef:
    """The reference of the dense image at batch B (only_last: the last sample's graph alone, for cotangents that live there)."""
    return VitRef(vit_weights(depth), vit_image(B), samples=[B - 1] if only_last else None)


# ------------------------------------------------------------------------------------------------ Q-Former
QF_D, QF_HEADS, QF_INTER, QF_ENC, QF_NQ, QF_NE, QF_EPS = 768, 12, 3072, 1408, 32, 257, 1e-12
QF_BATCHES = (1, 3)
QF_QUERIES = (0, 31)
QF_ENC_ROWS = (0, 255, 256)
QF_PREFIX = "Qformer.bert."
# (layers, batches).  Two layers: layer 0 holds the cross-attention, layer 1 is the last.  Under a cotangent in query row (b, q)
# everything of the LAST layer from its self-attention's query projection upwards acts on that row alone (the cross-attention's
# dk / dv go to the image tokens, not to other queries), while the self-attention's dk / dv spread over the 32 queries of
# sample b -- so in the two-layer module layer 0's cross-attention is NOT localised.  The one-layer module, whose last layer is
# the cross layer, is what localises the cross-attention's query projection, output dense and LayerNorm.
QF_MODULES = ((2, QF_BATCHES), (1, (3,)))


def qf_weights(layers: int) -> Dict[str, torch.Tensor]:
    sd = gu.qformer_weights(QF_D, layers, QF_INTER, QF_ENC, seed=900 + layers, std=0.04)
    sd["query_tokens"] = _randn((1, QF_NQ, QF_D), 910, 0.02)
    return sd


def qf_local_names(layers: int) -> List[str]:
    p = QF_PREFIX + f"encoder.layer.{layers - 1}."
    blocks = ["attention."] + (["crossattention."] if (layers - 1) % 2 == 0 else [])
    names = []
    for a in blocks:
        names += [p + a + s for s in ("self.query.weight", "self.query.bias", "output.dense.weight", "output.dense.bias",
                                      "output.LayerNorm.weight", "output.LayerNorm.bias")]
    names += [p + s for s in ("intermediate_query.dense.weight", "intermediate_query.dense.bias", "output_query.dense.weight",
                              "output_query.dense.bias", "output_query.LayerNorm.weight", "output_query.LayerNorm.bias")]
    return names


def qf_enc_local_names(layers: int) -> List[str]:
    """One nonzero image-token row: dK^T . enc and dV^T . enc of every cross layer are that row's outer product."""
    return [QF_PREFIX + f"encoder.layer.{i}.crossattention.self.{w}.weight" for i in range(0, layers, 2) for w in ("key", "value")]


def qf_zero_sibling(name: str) -> Optional[str]:
    """A key bias shifts every score of a softmax row alike: its exact gradient is zero, and it is measured against the value
    bias of the same attention (tests/test_qformer_train_gpu.py)."""
    return name.replace("key.bias", "value.bias") if name.endswith("self.key.bias") else None


def qf_inputs(B: int):
    """(query_embeds f32, image tokens as the bf16 values the kernels read, dense cotangent)."""
    top = max(QF_BATCHES)
    return (_randn((top, QF_NQ, QF_D), 31)[:B].contiguous(), _randn((top, QF_NE, QF_ENC), 32)[:B].to(BF16).contiguous(),
            _randn((top, QF_NQ, QF_D), 33, 0.1)[:B].contiguous())


def qf_row_cot(B: int, b: int, q: int) -> torch.Tensor:
    dout = torch.zeros(B, QF_NQ, QF_D)
    dout[b, q] = _randn((QF_D,), 6000 + 100 * b + q, 0.1)
    return dout


def qf_row_enc(B: int, b: int, r: int) -> torch.Tensor:
    enc = torch.zeros(B, QF_NE, QF_ENC, dtype=BF16)
    enc[b, r] = _randn((QF_ENC,), 5000 + 1000 * b + r).to(BF16)
    return enc


class QfRef:
    """float64 autograd through R.qformer_forward; every matrix rounded to bf16 (the trainable Q-Former's working copies), the
    image tokens given as the bf16 values the kernels read.  grads() also returns "d_query_embeds" and "d_enc"."""

    def __init__(self, sd: Dict[str, torch.Tensor], query_embeds: torch.Tensor, enc: torch.Tensor):
        self.leaves = {}
        for k, t in sd.items():
            if k == "query_tokens":
                continue
            self.leaves[k] = (t.to(BF16) if t.dim() >= 2 else t).double().requires_grad_(True)
        self.leaves["d_query_embeds"] = query_embeds.double().requires_grad_(True)
        self.leaves["d_enc"] = enc.double().requires_grad_(True)
        self.out = R.qformer_forward(self.leaves, self.leaves["d_query_embeds"], self.leaves["d_enc"], heads=QF_HEADS, eps=QF_EPS)

    def grads(self, dout: torch.Tensor) -> Dict[str, torch.Tensor]:
        names = list(self.leaves)
        gs = torch.autograd.grad(self.out, [self.leaves[n] for n in names], dout.double(), retain_graph=True)
        return dict(zip(names, gs))


@functools.lru_cache(maxsize=None)
def qf_ref(layers: int, B: int) -> QfRef:
    q, enc, _ = qf_inputs(B)
    return QfRef(qf_weights(layers), q, enc)


# ------------------------------------------------------------------------------------------------ LLaMA + q/v LoRA
LL_D, LL_LAYERS, LL_HEADS, LL_INTER, LL_V, LL_R, LL_ALPHA = 4096, 1, 32, 11008, 1000, 8, 16.0
LL_B, LL_S, LL_PAD = 2, 81, 4                   # S = 81: no multiple of 16, past 64; sample 1's mask is zero on its last 4 rows
LL_SINGLE = ((0, 1), (0, 16), (0, 17), (0, 64), (0, 65), (0, 80), (1, 76))       # (sample, the one labelled position t)
# first labelled position of the dense cases: 10 leaves 138 label rows of 162 (every row runs), 45 leaves 68 -- the last layer
# then runs its o_proj / MLP on the label rows only (LlamaHIP.forward_loss: 16 < rows <= M / 2)
LL_DENSE = (10, 45)


def llama_case():
    """(base weights bf16-rounded as the kernels hold them, LoRA tensors, inputs_embeds, attention mask, token ids): the
    settings of tests/test_model_gpu.py::test_llama_lora_qv_vs_oracle at S = 81."""
    from myriad_amd.lora import lora_param_specs
    sd = gu.llama_weights(LL_D, LL_LAYERS, LL_INTER, LL_V, seed=611)
    sd = {k: (v.to(BF16).float() if v.numel() > 4096 else v) for k, v in sd.items()}
    gen = torch.Generator().manual_seed(612)
    lora_sd = {}
    for name, ishape, _ in lora_param_specs(LL_LAYERS, LL_D, LL_R):
        lora_sd[name] = torch.randn(ishape, generator=gen) * (0.02 if "lora_A" in name else 0.05)
    emb = torch.randn(LL_B, LL_S, LL_D, generator=gen) * 0.02
    mask = torch.ones(LL_B, LL_S, dtype=torch.long)
    mask[1, -LL_PAD:] = 0
    ids = torch.randint(3, LL_V, (LL_B, LL_S), generator=gen)
    return sd, lora_sd, emb, mask, ids


def llama_single_labels(ids: torch.Tensor, b: int, t: int) -> torch.Tensor:
    labels = torch.full_like(ids, -100)
    labels[b, t] = ids[b, t]
    return labels


def llama_zero_sibling(name: str, t: int) -> Optional[str]:
    """The label at t = 1 is predicted by row 0, which attends to one key: its softmax is the constant 1, the query has no
    say, and the exact gradient of the q-side LoRA pair is zero.  It is measured against the v-side tensor of the same shape."""
    return name.replace("q_proj", "v_proj") if t == 1 and "q_proj" in name else None


def llama_dense_labels(ids: torch.Tensor, mask: torch.Tensor, first: int) -> torch.Tensor:
    labels = ids.clone()
    labels[:, :first] = -100
    labels[mask == 0] = -100
    return labels


def llama_live_rows(labels: torch.Tensor) -> torch.Tensor:
    """[B, S] bool: the rows of inputs_embeds the loss depends on.  R.llama_causal_lm pairs logits[:, :-1] with labels[:, 1:]
    (the shift of modeling_llama.py:695-703): the label at position t is predicted by the logit row t - 1, and under the causal
    mask that row reads the inputs of rows 0 .. t - 1.  So row s of sample b is live exactly when s < the last labelled
    position of b; every other row -- a sample without labels included -- has an exactly zero gradient."""
    B, S = labels.shape
    pos = torch.arange(S)[None].expand(B, S)
    last = torch.where(labels != -100, pos, torch.full_like(pos, -1)).max(dim=1).values
    return pos < last[:, None]


class LlamaRef:
    """Autograd through R.llama_causal_lm in float32, as tests/test_model_gpu.py runs it: the oracle's attention casts its
    softmax to float32 (modeling_llama.py:214), so its current signature does not run in float64.  One forward to the logits;
    each label set's loss is the oracle's own clamp_ce_loss on its own shift, back-propagated through the kept graph."""

    def __init__(self, dropout_mask=None):
        """dropout_mask: the keep / (1 - p) factors of the q_proj and v_proj LoRA inputs, as the oracle takes them."""
        from myriad_amd.lora import PEFT_PREFIX
        sd, lora_sd, emb, mask, ids = llama_case()
        self.mask, self.ids = mask, ids
        self.emb = emb.clone().requires_grad_(True)
        self.lora = {n: t.clone().requires_grad_(True) for n, t in lora_sd.items()}
        osd = dict(sd)
        for n, t in self.lora.items():
            osd[n.replace(PEFT_PREFIX, "llama_model.model.layers.")] = t
        _, self.logits = R.llama_causal_lm(osd, self.emb, mask, None, LL_HEADS,
                                           lora=dict(r=LL_R, alpha=LL_ALPHA, dropout_mask=dropout_mask))

    def loss_and_grads(self, labels: torch.Tensor):
        V = self.logits.shape[-1]
        loss = R.clamp_ce_loss(self.logits[..., :-1, :].reshape(-1, V), labels[..., 1:].reshape(-1))
        names = list(self.lora)
        gs = torch.autograd.grad(loss, [self.emb] + [self.lora[n] for n in names], retain_graph=True)
        return float(loss.detach()), gs[0], dict(zip(names, gs[1:]))


@functools.lru_cache(maxsize=None)
def llama_ref() -> LlamaRef:
    return LlamaRef()
