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

    @torch.no_grad()
    def forward_train(self, image: torch.Tensor, rel_pos_bias: Optional[torch.Tensor] = None,
                      checkpoint: bool = False) -> torch.Tensor:
        """forward() with the state for backward() kept (checkpoint: only each block's input).  Same output bits."""
        (h, xn, B, N), patches = self._embed(image)
        D, M, nb = self.D, B * N, len(self.blocks)
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
    def backward(self, dout: torch.Tensor, grads: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """dout [B, N, D] f32: the gradient of forward_train's output.  Writes every ViT parameter gradient (f32, reference
        names and shapes) into `grads` (allocated when None) and returns it.  Frees the saved state."""
        ctx, self._ctx = self._ctx, None
        if ctx is None:
            raise RuntimeError("EvaViTHIP.backward: no forward_train to differentiate")
        if self._T is None:
            self._T = [{k: torch.empty((blk[k].shape[1], blk[k].shape[0]), dtype=BF16, device=self.dev)
                        for k in ("wqkv", "wproj", "w1", "w2")} for blk in self.blocks]
            self._refresh_T()
        if grads is None:
            grads = {k: torch.empty(v, dtype=F32, device=self.dev) for k, v in self.grad_shapes().items()}
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
        return grads
