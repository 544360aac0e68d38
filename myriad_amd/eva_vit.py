"""EVA ViT-g/14 vision encoder on the HIP kernels: the frozen forward, and a training forward + backward.

Mirrors `VisionTransformer.forward_features` (reference minigpt4/models/eva_vit.py:324-340; no final norm/head),
`PatchEmbed.forward` (:198-204), `Block.forward` (:173-180), `Attention.forward` (:118-148: fused qkv with bias
cat(q_bias, 0, v_bias), q scaled by head_dim^-0.5, optional additive rel-pos bias) and `Mlp.forward` (:54-61).

MI355X mapping: patch embedding = patchify + MFMA GEMM with the positional embedding fused as the residual
epilogue; per block LN(fp32->bf16) -> qkv GEMM(+bias) -> fused attention (head_dim 88 padded to 96 in LDS) ->
proj GEMM(+bias +fp32 residual) -> LN -> fc1 GEMM(+bias +erf-GELU epilogue) -> fc2 GEMM(+bias +residual).

Training (forward_train / backward): the same launches as the frozen forward plus what the backward reads (the attention's
LSE, the fc1 pre-activation); per block, in reverse: fc2 weight gradient -> dgrad with gelu' in the epilogue -> fc1 weight
gradient -> dgrad + LN2 backward (+ its parameter gradients, ops.gemm_layernorm_bwd) -> proj weight gradient -> dgrad ->
attention backward into one [M, 3D] dqkv -> qkv weight gradient -> dgrad + LN1 backward; then the patch embedding.  With
`checkpoint` the forward keeps only each block's input and the backward recomputes the block (use_checkpoint, eva_vit.py:
176-180), which gives the same bits.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import ops

BF16, F32 = torch.bfloat16, torch.float32


def vit_param_shapes(D: int, C: int, P: int, n_tok: int, hidden: List[int], prefix: str = "visual_encoder.") -> Dict[str, tuple]:
    """Reference names -> shapes of an EVA ViT's parameters (hidden: the MLP width of each block), in the order the flat
    parameter buffer keeps them: q_bias and v_bias of a block adjacent, every block laid out alike."""
    pre = prefix
    out = {pre + "cls_token": (1, 1, D), pre + "pos_embed": (1, n_tok, D),
           pre + "patch_embed.proj.weight": (D, C, P, P), pre + "patch_embed.proj.bias": (D,)}
    for i, Hd in enumerate(hidden):
        b = pre + f"blocks.{i}."
        out.update({b + "norm1.weight": (D,), b + "norm1.bias": (D,), b + "attn.q_bias": (D,), b + "attn.v_bias": (D,),
                    b + "attn.qkv.weight": (3 * D, D), b + "attn.proj.weight": (D, D), b + "attn.proj.bias": (D,),
                    b + "norm2.weight": (D,), b + "norm2.bias": (D,), b + "mlp.fc1.weight": (Hd, D),
                    b + "mlp.fc1.bias": (Hd,), b + "mlp.fc2.weight": (D, Hd), b + "mlp.fc2.bias": (D,)})
    return out


def vit_param_specs(shapes: Dict[str, tuple]):
    """ParamStore specs (name, internal shape, reference shape): the ViT's masters keep the reference's own layout."""
    return [(n, tuple(shp), tuple(shp)) for n, shp in shapes.items()]


def drop_path_keep_prob(rate: float, depth: int) -> List[float]:
    """q_i = 1 - rate * i / (depth - 1): the keep probability of block i (eva_vit.py:276, dpr = linspace(0, rate, depth))."""
    return [1.0 - (float(rate) * i / (depth - 1) if depth > 1 else 0.0) for i in range(depth)]


_M32 = 0xFFFFFFFF
DROP_PATH_HASH0 = 0x243F6A88


def _dp_mix(h, v):
    """One absorption step of the keep-bit hash on 32-bit words held in int64 (a tensor or an int): xor the word in, multiply by
    the golden-ratio constant, then the murmur3 finaliser."""
    h = ((h ^ (v & _M32)) * 0x9E3779B1) & _M32
    h = h ^ (h >> 15)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def drop_path_keep_bits(seed: int, rank: int, step: int, micro: int, depth: int, batch: int, rate: float) -> torch.Tensor:
    """The stochastic-depth keep bits of one training forward: host bool [depth, 2, batch] (attention, MLP).  A pure function of
    its arguments in integer arithmetic: the 32-bit words seed lo, seed hi, rank, step lo, step hi, micro,
    block, branch, sample are absorbed in that order by _dp_mix from DROP_PATH_HASH0; u = the hash's upper 24 bits; the sample is
    DROPPED iff u * (depth - 1) < R * block with R = round(rate * 2^24), i.e. with probability p_i = rate * i / (depth - 1) to
    within 2^-24.  Block 0 never drops."""
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"drop_path_rate {rate}: must be in [0, 1)")
    seed, step = int(seed), int(step)
    h = DROP_PATH_HASH0
    for v in (seed, seed >> 32, int(rank), step, step >> 32, int(micro)):
        h = _dp_mix(h, v)
    i = torch.arange(depth, dtype=torch.int64).view(depth, 1, 1)
    j = torch.arange(2, dtype=torch.int64).view(1, 2, 1)
    b = torch.arange(batch, dtype=torch.int64).view(1, 1, batch)
    hh = _dp_mix(_dp_mix(_dp_mix(torch.full((depth, 1, 1), h, dtype=torch.int64), i), j), b)
    u = hh >> 8
    R = int(round(float(rate) * (1 << 24)))
    return ~(u * max(depth - 1, 1) < R * i)


class EvaViTHIP:
    def __init__(self, sd: Dict[str, torch.Tensor], n_heads: int, device, eps: float = 1e-6,
                 prefix: str = "visual_encoder."):
        dev = self.dev = torch.device(device)
        self.H, self.eps = n_heads, eps

        # always copies: load_weights writes these in place, and must not write through into the caller's tensors
        def bf(t):
            return t.detach().to(device=dev, dtype=BF16, copy=True).contiguous()

        def f32(t):
            return t.detach().to(device=dev, dtype=F32, copy=True).contiguous()

        pw = sd[prefix + "patch_embed.proj.weight"]
        self.D, self.C, self.P = pw.shape[0], pw.shape[1], pw.shape[2]
        K = self.C * self.P * self.P
        Kpad = ops.round_up(K, 64)
        w = torch.zeros(self.D, Kpad, dtype=pw.dtype, device=pw.device)
        w[:, :K] = pw.reshape(self.D, K)
        self.patch_w = bf(w)
        self.patch_b = f32(sd[prefix + "patch_embed.proj.bias"])
        cls = sd[prefix + "cls_token"].reshape(1, self.D).float()
        pos = sd.get(prefix + "pos_embed")
        pos = pos.reshape(-1, self.D).float() if pos is not None else torch.zeros(1, self.D, device=pw.device)
        self.n_tok = pos.shape[0] if (prefix + "pos_embed") in sd else None
        self.prefix = prefix
        self.cls_f32, self.pos_f32 = f32(cls), f32(pos)   # (load_weights rebuilds the rows below from either key)
        self.cls_row = f32(cls + pos[:1])          # x[:,0] = cls + pos[0]
        self.pos_patches = f32(pos[1:]) if pos.shape[0] > 1 else None
        self.hd = self.D // n_heads
        self.blocks: List[dict] = []
        i = 0
        while (prefix + f"blocks.{i}.norm1.weight") in sd:
            p = prefix + f"blocks.{i}."
            qb, vb = sd[p + "attn.q_bias"], sd[p + "attn.v_bias"]
            w1, b1, w2 = sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"], sd[p + "mlp.fc2.weight"]
            Hd = w1.shape[0]
            Hp = ops.round_up(Hd, 64)   # int(1408*4.3637)=6144 already; tiny configs get zero-padded
            if Hp != Hd:
                w1 = torch.cat([w1, torch.zeros(Hp - Hd, w1.shape[1], dtype=w1.dtype, device=w1.device)], 0)
                b1 = torch.cat([b1, torch.zeros(Hp - Hd, dtype=b1.dtype, device=b1.device)], 0)
                w2 = torch.cat([w2, torch.zeros(w2.shape[0], Hp - Hd, dtype=w2.dtype, device=w2.device)], 1)
            self.blocks.append(dict(
                n1w=f32(sd[p + "norm1.weight"]), n1b=f32(sd[p + "norm1.bias"]),
                wqkv=bf(sd[p + "attn.qkv.weight"]), bqkv=f32(torch.cat([qb, torch.zeros_like(vb), vb])),
                wproj=bf(sd[p + "attn.proj.weight"]), bproj=f32(sd[p + "attn.proj.bias"]),
                n2w=f32(sd[p + "norm2.weight"]), n2b=f32(sd[p + "norm2.bias"]),
                w1=bf(w1), b1=f32(b1), w2=bf(w2), b2=f32(sd[p + "mlp.fc2.bias"]), Hd=Hd))
            i += 1
        self._T: Optional[List[dict]] = None       # transposed bf16 weights for the dgrad GEMMs (built by the first backward)
        self._ctx = None
        self.trainable = False
        self.last_drop_stats: Optional[dict] = None   # forward_train: branch rows run / dense / branches skipped

    @torch.no_grad()
    def forward(self, image: torch.Tensor, rel_pos_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """image [B,3,H,W] f32 (device) -> [B, 1+np, D] f32."""
        state = self.embed(image)
        state = self.run_blocks(state, 0, len(self.blocks), rel_pos_bias)
        return self.finish(state)

    @torch.no_grad()
    def embed(self, image: torch.Tensor):
        """Patch embedding + cls / positional rows and the first block's LayerNorm: the state that run_blocks carries."""
        return self._embed(image)[0]

    def _embed(self, image: torch.Tensor):
        B = image.shape[0]
        D = self.D
        patches = ops.patchify(image.contiguous(), self.P)               # [B*np, Kpad] bf16
        np_ = patches.shape[0] // B
        N = np_ + 1
        x = torch.empty((B, N, D), dtype=F32, device=self.dev)
        ops.copy3d(self.cls_row.view(1, 1, D).expand(B, 1, D), x[:, :1])
        for b in range(B):   # per image so the pos-embed rides the residual epilogue and rows land at x[b,1:]
            ops.gemm(patches[b * np_:(b + 1) * np_], self.patch_w, out=x[b, 1:], bias=self.patch_b,
                     residual=self.pos_patches)
        h = x.view(B * N, D)
        xn = ops.layernorm_fwd(h, self.blocks[0]["n1w"], self.blocks[0]["n1b"], self.eps)[0] if self.blocks else None
        return (h, xn, B, N), patches

    @torch.no_grad()
    def run_blocks(self, state, lo: int, hi: int, rel_pos_bias: Optional[torch.Tensor] = None):
        """Blocks lo .. hi-1 on a state from embed() / an earlier run_blocks (a forward may be issued in pieces)."""
        h, xn, B, N = state
        D, H, hd = self.D, self.H, self.hd
        M = B * N
        scale = hd ** -0.5
        # each LayerNorm rides the split-K reduce of the GEMM that produces its input when that GEMM is split
        # (ops.gemm_residual_layernorm: fc2 -> next block's norm1, proj -> norm2); only block 0's norm1 is its own launch
        nb = len(self.blocks)
        for bi in range(lo, hi):
            blk = self.blocks[bi]
            qkv = ops.gemm(xn, blk["wqkv"], bias=blk["bqkv"]).view(B, N, 3 * D)
            o, _ = ops.attn_fwd(qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:], H, hd, scale, bias=rel_pos_bias,
                                need_lse=False)
            h, xn = ops.gemm_residual_layernorm(o.view(M, D), blk["wproj"], blk["bproj"], h, blk["n2w"], blk["n2b"], self.eps)
            a = ops.gemm(xn, blk["w1"], bias=blk["b1"], gelu=True)
            if bi + 1 < nb:
                nxt = self.blocks[bi + 1]
                h, xn = ops.gemm_residual_layernorm(a, blk["w2"], blk["b2"], h, nxt["n1w"], nxt["n1b"], self.eps)
            else:
                h = ops.gemm(a, blk["w2"], bias=blk["b2"], residual=h, out_dtype=F32)
        return (h, xn, B, N)

    @staticmethod
    def finish(state) -> torch.Tensor:
        h, _, B, N = state
        return h.view(B, N, -1)

    # ------------------------------------------------------------------ weights
    @torch.no_grad()
    def load_weights(self, sd: Dict[str, torch.Tensor]) -> List[str]:
        """Write the `visual_encoder.*` entries of a (reference-named) state dict into the working weights, in place -- a
        captured forward keeps reading the same storage -- including the padded layouts (patch_w's K, fc1 / fc2's hidden
        width).  Keys it does not hold are left as they are.  Returns the names it wrote.  Ordered on the current stream."""
        pre, D, done = self.prefix, self.D, []

        def get(name):
            t = sd.get(pre + name)
            if t is not None:
                done.append(pre + name)
                return t.detach().to(device=self.dev, dtype=F32)
            return None

        t = get("patch_embed.proj.weight")
        if t is not None:
            self.patch_w[:, :t[0].numel()].copy_(t.reshape(D, -1))
        t = get("patch_embed.proj.bias")
        if t is not None:
            self.patch_b.copy_(t)
        c, p = get("cls_token"), get("pos_embed")
        if c is not None:
            self.cls_f32.copy_(c.reshape(1, D))
        if p is not None:
            self.pos_f32.copy_(p.reshape(-1, D))
            if self.pos_patches is not None:
                self.pos_patches.copy_(self.pos_f32[1:])
        if c is not None or p is not None:
            self.cls_row.copy_(self.cls_f32 + self.pos_f32[:1])
        for i, blk in enumerate(self.blocks):
            b = f"blocks.{i}."
            Hd = blk["Hd"]
            for key, name in (("n1w", "norm1.weight"), ("n1b", "norm1.bias"), ("wqkv", "attn.qkv.weight"),
                              ("wproj", "attn.proj.weight"), ("bproj", "attn.proj.bias"), ("n2w", "norm2.weight"),
                              ("n2b", "norm2.bias"), ("b2", "mlp.fc2.bias")):
                t = get(b + name)
                if t is not None:
                    blk[key].copy_(t)
            t = get(b + "attn.q_bias")
            if t is not None:
                blk["bqkv"][:D].copy_(t)
            t = get(b + "attn.v_bias")
            if t is not None:
                blk["bqkv"][2 * D:].copy_(t)
            t = get(b + "mlp.fc1.weight")
            if t is not None:
                blk["w1"][:Hd].copy_(t)
            t = get(b + "mlp.fc1.bias")
            if t is not None:
                blk["b1"][:Hd].copy_(t)
            t = get(b + "mlp.fc2.weight")
            if t is not None:
                blk["w2"][:, :Hd].copy_(t)
        if done and self._T is not None:
            self._refresh_T()
        return done

    # ------------------------------------------------------------------ trainable ViT (freeze_vit: False)
    def param_specs(self):
        """ParamStore specs (name, internal shape, reference shape) of the trainable ViT: the reference's names and shapes
        (grad_shapes()), held in the reference's own layout."""
        return vit_param_specs(self.grad_shapes())

    @torch.no_grad()
    def bind_trainable(self, store, need_backward: bool = True) -> None:
        """The ViT's parameters are `store`'s fp32 masters from now on (a ParamStore holding param_specs()).
        The bf16 weight matrices -- wqkv, wproj, w1, w2, patch_w, with their padding -- keep their storage and their transposed
        copies for the dgrad GEMMs exist from here on; refresh() rewrites both from the masters in one launch
        (ops.RefreshTable).  Norm weights, biases, cls_token and pos_embed are read in place (fp32 views of the flat buffer;
        pos_patches is rows 1.. of the pos_embed master); what is assembled from two tensors -- bqkv = q_bias | 0 | v_bias of
        every block in one [blocks, 3, D] buffer, cls_row = cls_token + pos_embed[0] -- and a zero-padded fc1 bias are rewritten
        by refresh() with the copy kernels.  grad_views maps every parameter to its gradient view for backward(grads=...)."""
        pre, D, P = self.prefix, self.D, store.p
        self._store = store
        self.grad_views = {n: store.g[n] for n in self.grad_shapes()}
        self.cls_f32 = P[pre + "cls_token"].view(1, D)
        self.pos_f32 = P[pre + "pos_embed"].view(-1, D)
        if self.pos_patches is not None:
            self.pos_patches = self.pos_f32[1:]
        self.patch_b = P[pre + "patch_embed.proj.bias"]
        K = self.C * self.P * self.P
        entries = [(P[pre + "patch_embed.proj.weight"].view(D, K), self.patch_w, None)]
        if need_backward and self._T is None:
            # zeros: the rows / columns of a padded hidden width are never written and must read as zero
            self._T = [{k: torch.zeros((blk[k].shape[1], blk[k].shape[0]), dtype=BF16, device=self.dev)
                        for k in ("wqkv", "wproj", "w1", "w2")} for blk in self.blocks]
        nb = len(self.blocks)
        self._bqkv_all = torch.zeros((max(nb, 1), 3, D), dtype=F32, device=self.dev)
        self._b1_padded = []
        q_off = []
        for i, blk in enumerate(self.blocks):
            b = pre + f"blocks.{i}."
            for key, name in (("n1w", "norm1.weight"), ("n1b", "norm1.bias"), ("bproj", "attn.proj.bias"),
                              ("n2w", "norm2.weight"), ("n2b", "norm2.bias"), ("b2", "mlp.fc2.bias")):
                blk[key] = P[b + name]
            if blk["Hd"] == blk["w1"].shape[0]:
                blk["b1"] = P[b + "mlp.fc1.bias"]
            else:
                # the master's slot in the flat buffer is rounded up to four elements and its tail is zero for good (no
                # gradient, no weight decay on a bias): copying the whole slot keeps the copy kernel's 16-byte granule and
                # writes zeros into the working bias's zero padding
                o, n4 = store.offsets[b + "mlp.fc1.bias"][0], ops.round_up(blk["Hd"], 4)
                self._b1_padded.append((store.flat_p[o:o + n4].view(1, n4), blk["b1"][:n4].view(1, n4)))
            blk["bqkv"] = self._bqkv_all[i].view(3 * D)
            oq, ov = store.offsets[b + "attn.q_bias"][0], store.offsets[b + "attn.v_bias"][0]
            if ov != oq + D:
                raise RuntimeError(f"{b}attn.q_bias / v_bias: not adjacent in the flat buffer")
            q_off.append(oq)
            for key, name in (("wqkv", "attn.qkv.weight"), ("wproj", "attn.proj.weight"), ("w1", "mlp.fc1.weight"),
                              ("w2", "mlp.fc2.weight")):
                entries.append((P[b + name], blk[key], self._T[i][key] if self._T is not None else None))
        step = (q_off[1] - q_off[0]) if nb > 1 else 2 * D
        if any(q_off[i + 1] - q_off[i] != step for i in range(nb - 1)):
            raise RuntimeError("the blocks' q_bias / v_bias are not evenly spaced in the flat buffer")
        # [blocks, 2, D]: q_bias, v_bias of every block, read where they lie in the flat buffer
        self._qv_src = torch.as_strided(store.flat_p, (nb, 2, D), (step, D, 1), q_off[0]) if nb else None
        self._table = ops.RefreshTable(entries, self.dev)
        self.trainable = True
        self.refresh()

    @torch.no_grad()
    def refresh(self) -> None:
        """Rewrite everything the forward / backward read that is not the masters themselves, in place, on the current stream:
        all bf16 matrices and their transposed copies (one launch), bqkv of all blocks (one), cls_row (two)."""
        D = self.D
        self._table.run()
        if self._qv_src is not None:
            ops.copy3d(self._qv_src, self._bqkv_all[:len(self.blocks), 0::2])
        row = self.cls_row.view(1, D)
        ops.copy2d(self.cls_f32, row)
        ops.copy2d(self.pos_f32[:1], row, accumulate=True)
        for src, dst in self._b1_padded:
            ops.copy2d(src, dst)

    def _refresh_T(self) -> None:
        """The transposed bf16 copies the dgrad GEMMs read, rewritten in place from the working weights."""
        for blk, T in zip(self.blocks, self._T):
            for key in ("wqkv", "wproj", "w1", "w2"):
                ops.transpose_to_bf16(blk[key], pad_to=1, out=T[key])

    # ------------------------------------------------------------------ training
    def _block_save(self, bi: int, h, xn, B: int, N: int, rel_pos_bias, want_pre: bool = True):
        """Block bi up to its fc1 activation, run as run_blocks runs it, keeping what the backward reads (want_pre: also
        the fc1 pre-activation, which costs a second fc1 GEMM)."""
        blk, D, H, hd = self.blocks[bi], self.D, self.H, self.hd
        M = B * N
        qkv = ops.gemm(xn, blk["wqkv"], bias=blk["bqkv"]).view(B, N, 3 * D)
        o, lse = ops.attn_fwd(qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:], H, hd, hd ** -0.5, bias=rel_pos_bias,
                              need_lse=True)
        h_mid, xn2 = ops.gemm_residual_layernorm(o.view(M, D), blk["wproj"], blk["bproj"], h, blk["n2w"], blk["n2b"], self.eps)
        a = ops.gemm(xn2, blk["w1"], bias=blk["b1"], gelu=True)
        # gelu's input for gelu': the frozen launch above applies gelu to the f32 product, which keeps the frozen forward's bits,
        # so the bf16 pre-activation comes from a second product
        pre = ops.gemm(xn2, blk["w1"], bias=blk["b1"]) if want_pre else None
        return dict(h_in=h, xn1=xn, qkv=qkv, o=o, lse=lse, h_mid=h_mid, xn2=xn2, pre=pre, a=a)

    # ------------------------------------------------------------------ stochastic depth (drop_path_rate)
    def _drop_plan(self, keep, keep_prob, B: int):
        """Per block (attention map, attention scale, MLP map, MLP scale) from the keep bits [depth, 2, B] (host bool) and the
        blocks' keep probabilities.  A block with keep probability 1 never drops: its maps are None and it runs the fused
        launches of the dense path.  Otherwise a map is the ops.DropPathMap of the kept samples and the scale is 1 / q."""
        nb = len(self.blocks)
        if not isinstance(keep, torch.Tensor) or keep.is_cuda or keep.dtype != torch.bool or tuple(keep.shape) != (nb, 2, B):
            raise ValueError(f"forward_train: keep must be a host bool tensor [{nb}, 2, {B}]")
        if keep_prob is None or len(keep_prob) != nb:
            raise ValueError(f"forward_train: keep_prob must list {nb} keep probabilities")
        plan = []
        for bi in range(nb):
            q = float(keep_prob[bi])
            if not 0.0 < q <= 1.0:
                raise ValueError(f"forward_train: keep_prob[{bi}] = {q} must be in (0, 1]")
            if q == 1.0:
                if not bool(keep[bi].all()):
                    raise ValueError(f"forward_train: block {bi} has keep probability 1 and a dropped sample")
                plan.append((None, 1.0, None, 1.0))
            else:
                plan.append((ops.DropPathMap.from_keep(keep[bi, 0]), 1.0 / q, ops.DropPathMap.from_keep(keep[bi, 1]), 1.0 / q))
        return plan

    def _norm_for(self, h, norm, m_next, N: int):
        """LayerNorm of the residual stream for the branch that reads it: full, the rows of its kept samples, or None."""
        if norm is None or (m_next is not None and m_next.K == 0):
            return None
        if m_next is None or m_next.full:
            return ops.layernorm_fwd(h, norm[0], norm[1], self.eps)[0]
        return ops.drop_path_residual_layernorm(h, None, None, 1.0, N, norm[0], norm[1], self.eps, keep_out=m_next,
                                                want_h=False)[1]

    def _branch_out(self, a, wt, bias, h, m, scale: float, norm, m_next, N: int):
        """A branch's last GEMM (a @ wt^T + bias) joined to the residual stream h, and the LayerNorm `norm` = (weight, bias)
        of the branch that follows (kept samples m_next).  m None: the dense branch with today's fused launch."""
        need_xn = norm is not None and (m_next is None or m_next.K > 0)
        compact_next = m_next is not None and not m_next.full
        if m is None:
            if need_xn and not compact_next:
                return ops.gemm_residual_layernorm(a, wt, bias, h, norm[0], norm[1], self.eps)
            h2 = ops.gemm(a, wt, bias=bias, residual=h, out_dtype=F32)
            return h2, self._norm_for(h2, norm, m_next, N)
        y = ops.gemm(a, wt, bias=bias, out_dtype=F32)                     # the kept samples' rows only
        w, b = norm if need_xn else (None, None)
        return ops.drop_path_residual_layernorm(h, y, m, scale, N, w, b, self.eps,
                                                keep_out=m_next if (need_xn and compact_next) else None)

    def _block_save_drop(self, bi: int, h, xn, B: int, N: int, rel_pos_bias, plan, want_pre: bool = True):
        """_block_save under stochastic depth: xn holds the rows of the attention branch's kept samples, every branch matrix
        is compact, and a branch that keeps nothing is not run at all."""
        blk, D, H, hd = self.blocks[bi], self.D, self.H, self.hd
        mA, sA, mM, _ = plan[bi]
        s = dict(h_in=h, xn1=xn, qkv=None, o=None, lse=None, pre=None, a=None)
        n2 = (blk["n2w"], blk["n2b"])
        if mA is not None and mA.K == 0:
            s["h_mid"], s["xn2"] = h, self._norm_for(h, n2, mM, N)
        else:
            Ka = B if mA is None else mA.K
            qkv = ops.gemm(xn, blk["wqkv"], bias=blk["bqkv"]).view(Ka, N, 3 * D)
            o, lse = ops.attn_fwd(qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:], H, hd, hd ** -0.5, bias=rel_pos_bias,
                                  need_lse=True)
            s.update(qkv=qkv, o=o, lse=lse)
            s["h_mid"], s["xn2"] = self._branch_out(o.view(Ka * N, D), blk["wproj"], blk["bproj"], h, mA, sA, n2, mM, N)
        if s["xn2"] is not None:
            s["a"] = ops.gemm(s["xn2"], blk["w1"], bias=blk["b1"], gelu=True)
            s["pre"] = ops.gemm(s["xn2"], blk["w1"], bias=blk["b1"]) if want_pre else None
        return s

    def _forward_train_drop(self, image, rel_pos_bias, checkpoint: bool, keep, keep_prob) -> torch.Tensor:
        (h, xn, B, N), patches = self._embed(image)
        D, nb = self.D, len(self.blocks)
        plan = self._drop_plan(keep, keep_prob, B)
        if nb and plan[0][0] is not None and not plan[0][0].full:          # (a first block that drops: its norm1 rows again)
            xn = self._norm_for(h, (self.blocks[0]["n1w"], self.blocks[0]["n1b"]), plan[0][0], N)
        saved = []
        for bi in range(nb):
            blk = self.blocks[bi]
            mM, sM = plan[bi][2], plan[bi][3]
            s = self._block_save_drop(bi, h, xn, B, N, rel_pos_bias, plan, want_pre=not checkpoint)
            saved.append(dict(h_in=h, xn1=xn) if checkpoint else s)
            nxt = self.blocks[bi + 1] if bi + 1 < nb else None
            norm = (nxt["n1w"], nxt["n1b"]) if nxt is not None else None
            m_next = plan[bi + 1][0] if nxt is not None else None
            if mM is not None and mM.K == 0:
                h, xn = s["h_mid"], self._norm_for(s["h_mid"], norm, m_next, N)
            else:
                h, xn = self._branch_out(s["a"], blk["w2"], blk["b2"], s["h_mid"], mM, sM, norm, m_next, N)
            del s
        run = sum((B if m is None else m.K) * N for p in plan for m in (p[0], p[2]))
        self.last_drop_stats = dict(branch_rows_run=run, branch_rows_dense=2 * nb * B * N,
                                    branches_skipped=sum(m is not None and m.K == 0 for p in plan for m in (p[0], p[2])))
        self._ctx = dict(patches=patches, saved=saved, B=B, N=N, rel_pos_bias=rel_pos_bias, checkpoint=checkpoint, plan=plan)
        return h.view(B, N, D)

    @torch.no_grad()
    def forward_train(self, image: torch.Tensor, rel_pos_bias: Optional[torch.Tensor] = None,
                      checkpoint: bool = False, keep: Optional[torch.Tensor] = None, keep_prob=None) -> torch.Tensor:
        """forward() with the state for backward() kept (checkpoint: only each block's input).  Same output bits.
        keep (host bool [depth, 2, B]: attention, MLP) with keep_prob (depth floats): stochastic depth -- a kept sample's branch
        output is scaled by 1 / keep_prob[block], a dropped sample's branch is not computed (eva_vit.py:173-176).  keep None:
        the dense path, launch for launch.  last_drop_stats records the branch rows run / a dense step would run / skipped."""
        if keep is not None:
            return self._forward_train_drop(image, rel_pos_bias, checkpoint, keep, keep_prob)
        if keep_prob is not None:
            raise ValueError("forward_train: keep_prob without keep")
        (h, xn, B, N), patches = self._embed(image)
        D, M, nb = self.D, B * N, len(self.blocks)
        self.last_drop_stats = dict(branch_rows_run=2 * nb * M, branch_rows_dense=2 * nb * M, branches_skipped=0)
        saved = []
        for bi in range(nb):
            blk = self.blocks[bi]
            s = self._block_save(bi, h, xn, B, N, rel_pos_bias, want_pre=not checkpoint)
            saved.append(dict(h_in=h, xn1=xn) if checkpoint else s)
            if bi + 1 < nb:
                nxt = self.blocks[bi + 1]
                h, xn = ops.gemm_residual_layernorm(s["a"], blk["w2"], blk["b2"], s["h_mid"], nxt["n1w"], nxt["n1b"], self.eps)
            else:
                h = ops.gemm(s["a"], blk["w2"], bias=blk["b2"], residual=s["h_mid"], out_dtype=F32)
            del s
        self._ctx = dict(patches=patches, saved=saved, B=B, N=N, rel_pos_bias=rel_pos_bias, checkpoint=checkpoint)
        return h.view(B, N, D)

    def grad_shapes(self) -> Dict[str, tuple]:
        """Reference names and shapes of the ViT's parameters (the keys backward() fills)."""
        return vit_param_shapes(self.D, self.C, self.P, self.pos_f32.shape[0], [blk["Hd"] for blk in self.blocks], self.prefix)

    @torch.no_grad()
    def backward(self, dout: torch.Tensor, grads: Optional[Dict[str, torch.Tensor]] = None,
                 accumulate: bool = False) -> Dict[str, torch.Tensor]:
        """dout [B, N, D] f32: the gradient of forward_train's output.  Writes every ViT parameter gradient (f32, reference
        names and shapes) into `grads` (allocated when None) and returns it.  Frees the saved state.
        accumulate: the gradients are added to what `grads` holds (it must be given).  After a forward_train with keep bits the
        parameters of a branch that kept nothing read exact zeros, or are left as they were when accumulating."""
        ctx, self._ctx = self._ctx, None
        if ctx is None:
            raise RuntimeError("EvaViTHIP.backward: no forward_train to differentiate")
        if accumulate and grads is None:
            raise ValueError("EvaViTHIP.backward: accumulate needs the gradients to add to")
        if self._T is None:
            self._T = [{k: torch.empty((blk[k].shape[1], blk[k].shape[0]), dtype=BF16, device=self.dev)
                        for k in ("wqkv", "wproj", "w1", "w2")} for blk in self.blocks]
            self._refresh_T()
        if grads is None:
            grads = {k: torch.empty(v, dtype=F32, device=self.dev) for k, v in self.grad_shapes().items()}
        if accumulate or ctx.get("plan") is not None:
            return self._backward_drop(dout, grads, ctx, accumulate)
        B, N, rpb = ctx["B"], ctx["N"], ctx["rel_pos_bias"]
        D, H, hd, pre = self.D, self.H, self.hd, self.prefix
        M = B * N
        scale = hd ** -0.5
        dh = dout.reshape(M, D)
        if dh.dtype != F32 or not dh.is_contiguous():
            raise ValueError("EvaViTHIP.backward: dout must be contiguous f32 [B, N, D]")
        dhb = ops.to_bf16(dh)                  # later blocks take it from the LayerNorm backward that writes dh
        for bi in range(len(self.blocks) - 1, -1, -1):
            blk, T, s = self.blocks[bi], self._T[bi], ctx["saved"][bi]
            if ctx["checkpoint"]:
                s = self._block_save(bi, s["h_in"], s["xn1"], B, N, rpb)
            ctx["saved"][bi] = None
            b, Hd, Hp = pre + f"blocks.{bi}.", blk["Hd"], blk["w1"].shape[0]
            g_w1 = grads[b + "mlp.fc1.weight"] if Hd == Hp else torch.empty((Hp, D), dtype=F32, device=self.dev)
            g_b1 = grads[b + "mlp.fc1.bias"] if Hd == Hp else torch.empty((Hp,), dtype=F32, device=self.dev)
            g_w2 = grads[b + "mlp.fc2.weight"] if Hd == Hp else torch.empty((D, Hp), dtype=F32, device=self.dev)
            ops.gemm_tn_wgrad(dhb, s["a"], g_w2, bias=grads[b + "mlp.fc2.bias"])
            dpre = ops.gemm_gelu_bwd(dhb, T["w2"], s["pre"])                           # [M, Hp] bf16, gelu' in the epilogue
            ops.gemm_tn_wgrad(dpre, s["xn2"], g_w1, bias=g_b1)
            dh_mid, dh_mid_b = ops.gemm_layernorm_bwd(dpre, T["w1"], s["h_mid"], blk["n2w"], self.eps, dres=dh,
                                                      dgamma=grads[b + "norm2.weight"], dbeta=grads[b + "norm2.bias"])
            if Hd != Hp:
                grads[b + "mlp.fc1.weight"].copy_(g_w1[:Hd])
                grads[b + "mlp.fc1.bias"].copy_(g_b1[:Hd])
                grads[b + "mlp.fc2.weight"].copy_(g_w2[:, :Hd])
            ops.gemm_tn_wgrad(dh_mid_b, s["o"].view(M, D), grads[b + "attn.proj.weight"], bias=grads[b + "attn.proj.bias"])
            do = ops.gemm(dh_mid_b, T["wproj"]).view(B, N, D)
            qkv = s["qkv"]
            dqkv = torch.empty((M, 3 * D), dtype=BF16, device=self.dev)
            d3 = dqkv.view(B, N, 3 * D)
            ops.attn_bwd(qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:], s["o"], do, s["lse"], H, hd, scale, bias=rpb,
                         dq=d3[:, :, :D], dk=d3[:, :, D:2 * D], dv=d3[:, :, 2 * D:])
            g_bqkv = torch.empty((3 * D,), dtype=F32, device=self.dev)
            ops.gemm_tn_wgrad(dqkv, s["xn1"], grads[b + "attn.qkv.weight"], bias=g_bqkv)
            grads[b + "attn.q_bias"].copy_(g_bqkv[:D])                                 # there is no k bias: its third is dropped
            grads[b + "attn.v_bias"].copy_(g_bqkv[2 * D:])
            dh, dhb = ops.gemm_layernorm_bwd(dqkv, T["wqkv"], s["h_in"], blk["n1w"], self.eps, dres=dh_mid,
                                             dgamma=grads[b + "norm1.weight"], dbeta=grads[b + "norm1.bias"])
            del s, dh_mid, dh_mid_b, dpre, dqkv, do
        self._embed_backward(dh, dhb, ctx, grads)
        return grads

    @staticmethod
    def _add_into(src: torch.Tensor, dst: torch.Tensor) -> None:
        n = src.numel()
        if n % 4 == 0 and dst.is_contiguous():
            ops.copy2d(src.view(1, n), dst.view(1, n), accumulate=True)
        else:
            dst.add_(src)

    def _backward_drop(self, dout, grads, ctx, accumulate: bool):
        """backward() after a forward_train with keep bits, and / or accumulating.  A branch's weight-gradient and dgrad GEMMs,
        its attention backward and its LayerNorm's parameter gradients see the rows of its kept samples only; the LayerNorm
        backward scatters them into the full residual gradient (ops.drop_path_layernorm_bwd) and writes the scaled bf16 rows
        the next branch reads.  Blocks that never drop (maps None) run the dense path's launches.  A branch that kept nothing
        launches nothing: its gradients are zero-filled, or left alone when accumulating.  accumulate: a block's gradients are
        computed into scratch of that block's size and added to `grads`."""
        B, N, rpb = ctx["B"], ctx["N"], ctx["rel_pos_bias"]
        D, H, hd, pre, eps = self.D, self.H, self.hd, self.prefix, self.eps
        M, nb = B * N, len(self.blocks)
        plan = ctx.get("plan") or [(None, 1.0, None, 1.0)] * nb
        dh = dout.reshape(M, D)
        if dh.dtype != F32 or not dh.is_contiguous():
            raise ValueError("EvaViTHIP.backward: dout must be contiguous f32 [B, N, D]")

        def grad_for(g, m, sc):
            """The bf16 gradient a branch reads: scale * g on the rows of its kept samples (None: it kept nothing)."""
            if m is None:
                return ops.to_bf16(g)
            if m.K == 0:
                return None
            return ops.drop_path_gather_scale(g, None if m.full else m, sc, N)

        def out_map(m):
            return None if (m is None or m.full or m.K == 0) else m

        dyb = grad_for(dh, plan[nb - 1][2], plan[nb - 1][3]) if nb else ops.to_bf16(dh)
        for bi in range(nb - 1, -1, -1):
            blk, T, s = self.blocks[bi], self._T[bi], ctx["saved"][bi]
            mA, sA, mM, sM = plan[bi]
            if ctx["checkpoint"]:
                s = self._block_save_drop(bi, s["h_in"], s["xn1"], B, N, rpb, plan)
            ctx["saved"][bi] = None
            b, Hd, Hp = pre + f"blocks.{bi}.", blk["Hd"], blk["w1"].shape[0]
            mlp = [b + n for n in ("mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "norm2.weight", "norm2.bias")]
            att = [b + n for n in ("norm1.weight", "norm1.bias", "attn.q_bias", "attn.v_bias", "attn.qkv.weight",
                                   "attn.proj.weight", "attn.proj.bias")]
            G = {n: torch.empty_like(grads[n]) for n in mlp + att} if accumulate else grads
            skipped = []
            # ---- MLP branch
            if mM is not None and mM.K == 0:
                skipped += mlp
                dh_mid, dyA = dh, grad_for(dh, mA, sA)
            else:
                g_w1 = G[b + "mlp.fc1.weight"] if Hd == Hp else torch.empty((Hp, D), dtype=F32, device=self.dev)
                g_b1 = G[b + "mlp.fc1.bias"] if Hd == Hp else torch.empty((Hp,), dtype=F32, device=self.dev)
                g_w2 = G[b + "mlp.fc2.weight"] if Hd == Hp else torch.empty((D, Hp), dtype=F32, device=self.dev)
                ops.gemm_tn_wgrad(dyb, s["a"], g_w2, bias=G[b + "mlp.fc2.bias"])
                dpre = ops.gemm_gelu_bwd(dyb, T["w2"], s["pre"])
                ops.gemm_tn_wgrad(dpre, s["xn2"], g_w1, bias=g_b1)
                if mM is None:
                    dh_mid, dyA = ops.gemm_layernorm_bwd(dpre, T["w1"], s["h_mid"], blk["n2w"], eps, dres=dh, want_bf16=mA is None,
                                                         dgamma=G[b + "norm2.weight"], dbeta=G[b + "norm2.bias"])
                    if mA is not None:
                        dyA = grad_for(dh_mid, mA, sA)
                else:
                    dxn = ops.gemm(dpre, T["w1"], out_dtype=F32)
                    ops.drop_path_layernorm_param_grads(dxn, s["h_mid"], eps, mM, N, G[b + "norm2.weight"], G[b + "norm2.bias"])
                    dh_mid, dyA = ops.drop_path_layernorm_bwd(dxn, s["h_mid"], blk["n2w"], eps, dh, mM, N, keep_out=out_map(mA),
                                                              out_scale=sA if mA is not None else 1.0,
                                                              want_bf16=not (mA is not None and mA.K == 0))
                    del dxn
                if Hd != Hp:
                    G[b + "mlp.fc1.weight"].copy_(g_w1[:Hd])
                    G[b + "mlp.fc1.bias"].copy_(g_b1[:Hd])
                    G[b + "mlp.fc2.weight"].copy_(g_w2[:, :Hd])
                del dpre, g_w1, g_b1, g_w2
            # ---- attention branch; its LayerNorm backward writes what the block before reads (its MLP; the embedding: all rows)
            mP, sP = (plan[bi - 1][2], plan[bi - 1][3]) if bi > 0 else (None, 1.0)
            if mA is not None and mA.K == 0:
                skipped += att
                dh_in, dyP = dh_mid, grad_for(dh_mid, mP, sP)
            else:
                Ka = B if mA is None else mA.K
                ops.gemm_tn_wgrad(dyA, s["o"].view(Ka * N, D), G[b + "attn.proj.weight"], bias=G[b + "attn.proj.bias"])
                do = ops.gemm(dyA, T["wproj"]).view(Ka, N, D)
                qkv = s["qkv"]
                dqkv = torch.empty((Ka * N, 3 * D), dtype=BF16, device=self.dev)
                d3 = dqkv.view(Ka, N, 3 * D)
                ops.attn_bwd(qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:], s["o"], do, s["lse"], H, hd, hd ** -0.5, bias=rpb,
                             dq=d3[:, :, :D], dk=d3[:, :, D:2 * D], dv=d3[:, :, 2 * D:])
                g_bqkv = torch.empty((3 * D,), dtype=F32, device=self.dev)
                ops.gemm_tn_wgrad(dqkv, s["xn1"], G[b + "attn.qkv.weight"], bias=g_bqkv)
                G[b + "attn.q_bias"].copy_(g_bqkv[:D])
                G[b + "attn.v_bias"].copy_(g_bqkv[2 * D:])
                if mA is None:
                    dh_in, dyP = ops.gemm_layernorm_bwd(dqkv, T["wqkv"], s["h_in"], blk["n1w"], eps, dres=dh_mid, want_bf16=mP is None,
                                                        dgamma=G[b + "norm1.weight"], dbeta=G[b + "norm1.bias"])
                    if mP is not None:
                        dyP = grad_for(dh_in, mP, sP)
                else:
                    dxn = ops.gemm(dqkv, T["wqkv"], out_dtype=F32)
                    ops.drop_path_layernorm_param_grads(dxn, s["h_in"], eps, mA, N, G[b + "norm1.weight"], G[b + "norm1.bias"])
                    dh_in, dyP = ops.drop_path_layernorm_bwd(dxn, s["h_in"], blk["n1w"], eps, dh_mid, mA, N, keep_out=out_map(mP),
                                                             out_scale=sP if mP is not None else 1.0,
                                                             want_bf16=not (mP is not None and mP.K == 0))
                    del dxn
                del dqkv, do
            for n in mlp + att:
                if n in skipped:
                    if not accumulate:
                        grads[n].zero_()
                elif accumulate:
                    self._add_into(G[n], grads[n])
            dh, dyb = dh_in, dyP
            del s, G, dh_mid, dh_in, dyA, dyP
        if not accumulate:
            self._embed_backward(dh, dyb, ctx, grads)
            return grads
        emb = [pre + n for n in ("cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias")]
        G = {n: torch.empty_like(grads[n]) for n in emb}
        self._embed_backward(dh, dyb, ctx, G)
        for n in emb:
            self._add_into(G[n], grads[n])
        return grads

    def _embed_backward(self, dh, dhb, ctx, grads) -> None:
        """The patch embedding's gradients from the residual gradient at the first block's input (dh f32, dhb its bf16 copy)."""
        B, N, D, pre = ctx["B"], ctx["N"], self.D, self.prefix
        # embedding: x[b, 0] = cls + pos[0], x[b, 1:] = patches_b @ W^T + bias + pos[1:]
        patches = ctx["patches"]
        np_ = N - 1
        dpos = grads[pre + "pos_embed"].view(N * D)
        dpos.copy_(ops.colsum(dh.view(B, N * D)))                                      # pos_embed: the batch sum of every row
        grads[pre + "cls_token"].view(D).copy_(dpos[:D])
        Kpad = self.patch_w.shape[1]
        g_pw = torch.empty((D, Kpad), dtype=F32, device=self.dev)
        for bb in range(B):
            ops.gemm_tn_wgrad(dhb[bb * N + 1:(bb + 1) * N], patches[bb * np_:(bb + 1) * np_], g_pw,
                              bias=grads[pre + "patch_embed.proj.bias"], accumulate=bb > 0)
        K = self.C * self.P * self.P
        grads[pre + "patch_embed.proj.weight"].view(D, K).copy_(g_pw[:, :K])
