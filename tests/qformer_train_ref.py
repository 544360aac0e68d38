"""torch references for the trainable Q-Former's dropout kernels, fed the kernels' own keep masks (ops.dropout_keep_mask)."""
import torch


def attn_dropout_ref(q, k, v, H, D, scale, keep):
    """q [B,Sq,H*D], k/v [B,Sk,H*D] (float, may require grad); keep [B,H,Sq,Sk] = 1/(1-p) or 0.
    Returns (O = (softmax(q k^T * scale) * keep) v as [B,Sq,H*D], LSE of the undropped scores [B,H,Sq])."""
    B, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    qh = q.view(B, Sq, H, D).transpose(1, 2)
    kh = k.view(B, Sk, H, D).transpose(1, 2)
    vh = v.view(B, Sk, H, D).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) * scale
    lse = torch.logsumexp(s, -1)
    o = (torch.softmax(s, -1) * keep) @ vh
    return o.transpose(1, 2).reshape(B, Sq, H * D), lse


def ln_dropout_ref(z, res, w, b, eps, keep_in=None, keep_out=None):
    """LN(z * keep_in + res) * keep_out (res None: LN(z) * keep_out).  Returns (LayerNorm input, output)."""
    x = z * keep_in + res if res is not None else z
    y = torch.nn.functional.layer_norm(x, (x.shape[-1],), w, b, eps)
    return x, (y * keep_out if keep_out is not None else y)
