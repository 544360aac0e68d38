"""Independent statements of stochastic depth in the trainable EVA ViT, for the drop-path tests:
the keep-bit draw rule in plain Python integers, and a float64 forward with the masks applied as the reference applies them
(eva_vit.py:173-176 with timm's drop_path, scale_by_keep=True), differentiable by torch autograd."""
import torch
import torch.nn.functional as F

M32 = 0xFFFFFFFF


def mix(h: int, v: int) -> int:
    h = ((h ^ (v & M32)) * 0x9E3779B1) & M32
    h ^= h >> 15
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def keep_bit(seed: int, rank: int, step: int, micro: int, block: int, branch: int, sample: int, depth: int, rate: float) -> bool:
    """One keep bit: the nine 32-bit words are absorbed in order from 0x243F6A88; u = the hash's upper 24 bits; dropped iff
    u * (depth - 1) < round(rate * 2^24) * block."""
    h = 0x243F6A88
    for v in (seed, seed >> 32, rank, step, step >> 32, micro, block, branch, sample):
        h = mix(h, v)
    u = h >> 8
    return not (u * max(depth - 1, 1) < int(round(rate * (1 << 24))) * block)


def keep_bits(seed, rank, step, micro, depth, batch, rate) -> torch.Tensor:
    return torch.tensor([[[keep_bit(seed, rank, step, micro, i, j, b, depth, rate) for b in range(batch)] for j in range(2)]
                         for i in range(depth)], dtype=torch.bool).view(depth, 2, batch)


def bf16_weights(sd):
    """float64 leaves of a ViT state dict, the GEMM weights rounded to bf16 as the kernels hold them."""
    leaves = {}
    for k, t in sd.items():
        t = t.detach().double().cpu()
        if k.endswith(("qkv.weight", "proj.weight", "fc1.weight", "fc2.weight")):
            t = t.to(torch.bfloat16).double()
        leaves[k] = t.requires_grad_(True)
    return leaves


def vit_forward_drop(sd, image, keep, keep_prob, num_heads: int = 16, eps: float = 1e-6, prefix: str = "visual_encoder."):
    """oracle.myriad_ref.vit_forward with stochastic depth: block i adds mask / keep_prob[i] * branch(LN(x)) per sample, mask =
    keep[i, 0] for the attention branch and keep[i, 1] for the MLP (1 kept, 0 dropped)."""
    from oracle import myriad_ref as R
    w = sd[prefix + "patch_embed.proj.weight"]
    Bi, C, Hh, Ww = image.shape
    P = w.shape[-1]                                                 # PatchEmbed: a convolution with kernel = stride = P, as a product
    patches = image.reshape(Bi, C, Hh // P, P, Ww // P, P).permute(0, 2, 4, 1, 3, 5).reshape(Bi, -1, C * P * P)
    x = F.linear(patches, w.reshape(w.shape[0], -1), sd[prefix + "patch_embed.proj.bias"])
    x = torch.cat((sd[prefix + "cls_token"].expand(x.shape[0], -1, -1), x), dim=1)
    if (prefix + "pos_embed") in sd:
        x = x + sd[prefix + "pos_embed"]
    depth = len(keep_prob)
    for i in range(depth):
        p = prefix + f"blocks.{i}."
        ma = keep[i, 0].to(x.dtype).view(-1, 1, 1) / keep_prob[i]
        mm = keep[i, 1].to(x.dtype).view(-1, 1, 1) / keep_prob[i]
        h = F.layer_norm(x, x.shape[-1:], sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        x = x + ma * R.vit_attention(sd, p + "attn.", h, num_heads)
        h = F.layer_norm(x, x.shape[-1:], sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        h = F.linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])
        h = F.gelu(h)
        h = F.linear(h, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
        x = x + mm * h
    return x
