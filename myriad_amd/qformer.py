"""BLIP-2 Q-Former (query-only path) on the HIP kernels: forward + dgrad-only backward to BOTH inputs.

Mirrors `BertModel.forward` (reference minigpt4/models/Qformer.py:804-965) as called by `Myriad.encode_img`
(myriad.py:256-261): `BertEmbeddings` LayerNorm of the raw query embeddings (:104-107), then per `BertLayer`
(:402-474) self-attention + `BertSelfOutput` (:285-289), cross-attention to the image tokens on layers with
layer_num % 2 == 0 (:386-395), and the query FFN `feed_forward_chunk_query` (:481-484).  Post-LN, eps 1e-12,
scores scaled by 1/sqrt(64) after q.k^T (:244), dropout inactive (frozen/eval, myriad.py:159-165).
Frozen (the shipped recipes), gradients flow to the query embeddings (VEInstructor tokens) and to the image tokens
(expert_adaptor), SURVEY 3.3.  With freeze_qformer: False (bind_trainable) the backward also writes every weight, bias and
LayerNorm gradient.  The hidden/residual stream is fp32, GEMM operands bf16.
"""
from __future__ import annotations

import math
from typing import Dict, List

import torch

from . import ops

BF16, F32 = torch.bfloat16, torch.float32

_SELF = ("query", "key", "value")


def qformer_param_specs(sd, prefix: str = "Qformer.bert.", cross_freq: int = 2):
    """ParamStore specs (name, internal shape, reference shape) of a trainable Q-Former + `query_tokens` (freeze_qformer:
    False, myriad.py:159-165), in the flat-buffer order the HIP path reads them in: inside each weight-decay group the
    query / key / value tensors of a layer are adjacent (one [3D, D] product and its bias), and the key / value tensors of
    ALL cross-attention layers come last, adjacent (the single [n_cross * 2D, We] product of QFormerHIP).  The checkpoint's
    optimiser order is the reference's named_parameters() order (checkpoint.reference_param_order), not this one."""
    names = ["query_tokens", prefix + "embeddings.LayerNorm.weight", prefix + "embeddings.LayerNorm.bias"]
    tail = []
    i = 0
    while (prefix + f"encoder.layer.{i}.attention.self.query.weight") in sd:
        p = prefix + f"encoder.layer.{i}."
        for blk in ("attention.",) + (("crossattention.",) if i % cross_freq == 0 else ()):
            for t in ("weight", "bias"):
                for w in (_SELF if blk == "attention." else _SELF[:1]):
                    names.append(p + blk + f"self.{w}.{t}")
                if blk == "crossattention.":
                    tail += [p + blk + f"self.{w}.{t}" for w in _SELF[1:]]
            names += [p + blk + "output.dense.weight", p + blk + "output.dense.bias",
                      p + blk + "output.LayerNorm.weight", p + blk + "output.LayerNorm.bias"]
        names += [p + "intermediate_query.dense.weight", p + "intermediate_query.dense.bias",
                  p + "output_query.dense.weight", p + "output_query.dense.bias",
                  p + "output_query.LayerNorm.weight", p + "output_query.LayerNorm.bias"]
        i += 1
    # the cross layers' key / value: weights of every layer, then biases (each group stays adjacent after the
    # ParamStore's stable split into weight-decay / no-decay runs)
    tail = [n for n in tail if n.endswith("weight")] + [n for n in tail if n.endswith("bias")]
    out = []
    for n in names + tail:
        shp = tuple(sd[n].shape)
        out.append((n, shp, shp))
    return out


def dropout_site_seed(seed: int, site: int) -> int:
    """The mask seed of one dropout site of a step (site 0: embeddings; layer i: 5i+1 self-attention probabilities, 5i+2 its
    output, 5i+3 cross-attention probabilities, 5i+4 its output, 5i+5 the query FFN output): a splitmix64 step of
    (step seed, site), below 2^63."""
    x = (int(seed) * 0x9E3779B97F4A7C15 + (int(site) + 1) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & ((1 << 64) - 1)
    return (x ^ (x >> 31)) & ((1 << 63) - 1)


class QFormerHIP:
    def __init__(self, sd: Dict[str, torch.Tensor], n_heads: int, device, eps: float = 1e-12, cross_freq: int = 2,
                 prefix: str = "Qformer.bert.", need_backward: bool = True):
        dev = self.dev = torch.device(device)
        self.H, self.eps = n_heads, eps

        def bf(t):
            return t.detach().to(device=dev, dtype=BF16).contiguous()

        def f32(t):
            return t.detach().to(device=dev, dtype=F32).contiguous()

        self.emb_w = f32(sd[prefix + "embeddings.LayerNorm.weight"])
        self.emb_b = f32(sd[prefix + "embeddings.LayerNorm.bias"])
        self.D = self.emb_w.numel()
        self.hd = self.D // n_heads
        self.layers: List[dict] = []
        i = 0
        while (prefix + f"encoder.layer.{i}.attention.self.query.weight") in sd:
            p = prefix + f"encoder.layer.{i}."
            a = p + "attention."
            L = dict(
                wqkv=bf(torch.cat([sd[a + "self.query.weight"], sd[a + "self.key.weight"], sd[a + "self.value.weight"]], 0)),
                bqkv=f32(torch.cat([sd[a + "self.query.bias"], sd[a + "self.key.bias"], sd[a + "self.value.bias"]], 0)),
                wo=bf(sd[a + "output.dense.weight"]), bo=f32(sd[a + "output.dense.bias"]),
                ln_a_w=f32(sd[a + "output.LayerNorm.weight"]), ln_a_b=f32(sd[a + "output.LayerNorm.bias"]),
                w1=bf(sd[p + "intermediate_query.dense.weight"]), b1=f32(sd[p + "intermediate_query.dense.bias"]),
                w2=bf(sd[p + "output_query.dense.weight"]), b2=f32(sd[p + "output_query.dense.bias"]),
                ln_f_w=f32(sd[p + "output_query.LayerNorm.weight"]), ln_f_b=f32(sd[p + "output_query.LayerNorm.bias"]),
                cross=(i % cross_freq == 0))
            if L["cross"]:
                c = p + "crossattention."
                L.update(cwq=bf(sd[c + "self.query.weight"]), cbq=f32(sd[c + "self.query.bias"]),
                         cwkv=bf(torch.cat([sd[c + "self.key.weight"], sd[c + "self.value.weight"]], 0)),
                         cbkv=f32(torch.cat([sd[c + "self.key.bias"], sd[c + "self.value.bias"]], 0)),
                         cwo=bf(sd[c + "output.dense.weight"]), cbo=f32(sd[c + "output.dense.bias"]),
                         ln_c_w=f32(sd[c + "output.LayerNorm.weight"]), ln_c_b=f32(sd[c + "output.LayerNorm.bias"]))
                if L["cwkv"].shape[1] % 64:
                    raise ValueError("encoder width must be a multiple of 64 (GEMM K granule)")
            if need_backward:
                for k in ("wqkv", "wo", "w1", "w2", "cwq", "cwkv", "cwo"):
                    if k in L:
                        L[k + "T"] = L[k].t().contiguous()
            self.layers.append(L)
            i += 1
        # The key / value projections of every cross-attention layer read the same image tokens (Qformer.py:172-176 with
        # encoder_hidden_states): one [n_cross * 2D, We] matrix turns 6 GEMMs inside the dependent layer chain into ONE in front
        # of it (forward) and 6 accumulating dgrad GEMMs into ONE K = n_cross * 2D product behind it (backward); same values
        # per layer -- each output column is the same dot product.
        cross = [L for L in self.layers if L["cross"]]
        self.n_cross = len(cross)
        if cross:
            self.cwkv_all = torch.cat([L["cwkv"] for L in cross], 0).contiguous()
            self.cbkv_all = torch.cat([L["cbkv"] for L in cross], 0).contiguous()
            self.cwkvT_all = torch.cat([L["cwkvT"] for L in cross], 1).contiguous() if need_backward else None
            for L in cross:
                L.pop("cwkv"); L.pop("cbkv"); L.pop("cwkvT", None)
        self._saved = None
        self.trainable = False

    # ------------------------------------------------------------------ trainable Q-Former (freeze_qformer: False)
    def bind_trainable(self, store, prefix: str = "Qformer.bert.", need_denc: bool = True) -> None:
        """Read the Q-Former's parameters from `store` (a ParamStore holding qformer_param_specs) from now on.  Biases, LayerNorm
        parameters and query_tokens are used in place (fp32 views of the flat buffer); the weight matrices as bf16 copies: ONE
        bf16 mirror of the Q-Former's weight-decay run of the flat buffer (query/key/value, cross key/value adjacent there, so
        wqkv / cwkv_all are plain views of it) plus the transposed copies the dgrad reads.  refresh() rewrites both in place, so
        the addresses never change.  `need_denc`: keep the transposed cross key/value matrix (d(image tokens) is needed)."""
        rng = store.module_range("Qformer", True)
        if rng is None:
            raise ValueError("the ParamStore holds no trainable Q-Former")
        a0, b0 = rng
        self._store, self._rng = store, rng
        self._mirror = torch.empty((b0 - a0,), dtype=BF16, device=self.dev)

        def span(names):
            o0 = store.offsets[names[0]][0]
            o = o0
            for n in names:
                if store.offsets[n][0] != o:
                    raise RuntimeError(f"{n}: not adjacent in the flat buffer")
                o += store.offsets[n][1]
            return o0, o

        def vec(names):
            lo, hi = span(names)
            return store.flat_p[lo:hi], store.flat_g[lo:hi]

        def mat(names):
            lo, hi = span(names)
            cols = store.ref_shape[names[0]][1]
            rows = (hi - lo) // cols
            return (self._mirror[lo - a0:hi - a0].view(rows, cols), store.flat_g[lo:hi].view(rows, cols))

        self.emb_w, self.g_emb_w = vec([prefix + "embeddings.LayerNorm.weight"])
        self.emb_b, self.g_emb_b = vec([prefix + "embeddings.LayerNorm.bias"])
        self._T = []                                      # (bf16 matrix, its transposed copy)
        cross_k, cross_kb = [], []
        for i, L in enumerate(self.layers):
            p = prefix + f"encoder.layer.{i}."
            a = p + "attention."
            keys = dict(wqkv=[a + f"self.{w}.weight" for w in ("query", "key", "value")],
                        bqkv=[a + f"self.{w}.bias" for w in ("query", "key", "value")],
                        wo=[a + "output.dense.weight"], bo=[a + "output.dense.bias"],
                        ln_a_w=[a + "output.LayerNorm.weight"], ln_a_b=[a + "output.LayerNorm.bias"],
                        w1=[p + "intermediate_query.dense.weight"], b1=[p + "intermediate_query.dense.bias"],
                        w2=[p + "output_query.dense.weight"], b2=[p + "output_query.dense.bias"],
                        ln_f_w=[p + "output_query.LayerNorm.weight"], ln_f_b=[p + "output_query.LayerNorm.bias"])
            if L["cross"]:
                c = p + "crossattention."
                keys.update(cwq=[c + "self.query.weight"], cbq=[c + "self.query.bias"], cwo=[c + "output.dense.weight"],
                            cbo=[c + "output.dense.bias"], ln_c_w=[c + "output.LayerNorm.weight"],
                            ln_c_b=[c + "output.LayerNorm.bias"])
                cross_k += [c + "self.key.weight", c + "self.value.weight"]
                cross_kb += [c + "self.key.bias", c + "self.value.bias"]
            for k, names in keys.items():
                if k.startswith(("w", "cw")):
                    L[k], L["g_" + k] = mat(names)
                    if L.get(k + "T") is None:
                        L[k + "T"] = torch.empty((L[k].shape[1], L[k].shape[0]), dtype=BF16, device=self.dev)
                    self._T.append((L[k], L[k + "T"]))
                else:
                    L[k], L["g_" + k] = vec(names)
        if self.n_cross:
            self.cwkv_all, self.g_cwkv_all = mat(cross_k)
            self.cbkv_all, self.g_cbkv_all = vec(cross_kb)
            if need_denc:
                if self.cwkvT_all is None:
                    self.cwkvT_all = torch.empty((self.cwkv_all.shape[1], self.cwkv_all.shape[0]), dtype=BF16, device=self.dev)
                self._T.append((self.cwkv_all, self.cwkvT_all))
            else:
                self.cwkvT_all = None
        self.trainable = True
        self.refresh()

    def refresh(self) -> None:
        """Rewrite the bf16 working copies from the fp32 masters, in place (after an optimiser update or a load): one cast of
        the Q-Former's weight-decay run + one transpose per matrix."""
        a0, b0 = self._rng
        ops.to_bf16(self._store.flat_p[a0:b0], out=self._mirror)
        for m, mT in self._T:
            ops.transpose_to_bf16(m, pad_to=1, out=mT)

    def forward(self, query_embeds: torch.Tensor, enc_b: torch.Tensor, save_for_backward: bool = True, dropout: float = 0.0,
                seed: int = 0):
        """query_embeds [B,nq,D] f32; enc_b [B,Nenc,We] bf16 image tokens.  Returns [B,nq,D] f32.
        dropout > 0 (train mode of a trainable Q-Former): BERT's dropout at the reference's four sites -- the embeddings'
        output, the attention probabilities (inside the attention kernels), BertSelfOutput and the query FFN output (both in
        the LayerNorm that follows) -- with counter-based masks of dropout_site_seed(seed, site), regenerated by backward()."""
        B, nq, D = query_embeds.shape
        Ne, We = enc_b.shape[1], enc_b.shape[2]
        M, H, hd = B * nq, self.H, self.hd
        scale = 1.0 / math.sqrt(hd)
        pd = float(dropout)
        sd_ = (lambda site: dropout_site_seed(seed, site)) if pd > 0 else (lambda site: 0)
        q_in = query_embeds.reshape(M, D).contiguous()
        if pd > 0:
            _, hb, h = ops.layernorm_fwd_dropout(q_in, None, self.emb_w, self.emb_b, self.eps, p_out=pd, seed_out=sd_(0))
        else:
            hb, h = ops.layernorm_fwd(q_in, self.emb_w, self.emb_b, self.eps, want_bf16=True, want_f32=True)

        def out_ln(a, w, bias, res, lw, lb, site):
            """LN(dropout(a W^T + b) + res) -> (LayerNorm input, bf16 out, f32 out); p = 0: the residual in the GEMM."""
            if pd == 0:
                y = ops.gemm(a, w, bias=bias, residual=res, out_dtype=F32)
                yb, yf = ops.layernorm_fwd(y, lw, lb, self.eps, want_bf16=True, want_f32=True)
                return y, yb, yf
            z = ops.gemm(a, w, bias=bias, out_dtype=F32)
            return ops.layernorm_fwd_dropout(z, res, lw, lb, self.eps, p_in=pd, seed_in=sd_(site))
        enc2 = enc_b.reshape(B * Ne, We)
        ckv_all = ops.gemm(enc2, self.cwkv_all, bias=self.cbkv_all).view(B, Ne, self.n_cross * 2 * D) if self.n_cross else None
        ci = 0
        saved = []
        tr = self.trainable and save_for_backward
        for li, L in enumerate(self.layers):
            s = dict(hb0=hb) if tr else {}
            # self-attention
            qkv = ops.gemm(hb, L["wqkv"], bias=L["bqkv"]).view(B, nq, 3 * D)
            ctx, lse = ops.attn_fwd_dropout(qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:], H, hd, scale, pd,
                                            sd_(5 * li + 1))
            y, hb, h = out_ln(ctx.view(M, D), L["wo"], L["bo"], h, L["ln_a_w"], L["ln_a_b"], 5 * li + 2)
            s.update(qkv=qkv, ctx=ctx, lse=lse, y_a=y)
            if L["cross"]:
                if tr:
                    s["hb_a"] = hb
                cq = ops.gemm(hb, L["cwq"], bias=L["cbq"]).view(B, nq, D)
                ckv = ckv_all[:, :, ci * 2 * D:(ci + 1) * 2 * D]
                ci += 1
                cctx, clse = ops.attn_fwd_dropout(cq, ckv[:, :, :D], ckv[:, :, D:], H, hd, scale, pd, sd_(5 * li + 3))
                yc, hb, h = out_ln(cctx.view(M, D), L["cwo"], L["cbo"], h, L["ln_c_w"], L["ln_c_b"], 5 * li + 4)
                s.update(cq=cq, ckv=ckv, cctx=cctx, clse=clse, y_c=yc)
            pre, act = ops.gemm_gelu_fwd(hb, L["w1"], L["b1"])       # GELU in the product's epilogue (one launch)
            if tr:
                s.update(hb_f=hb, act=act)
            yf, hb, h = out_ln(act, L["w2"], L["b2"], h, L["ln_f_w"], L["ln_f_b"], 5 * li + 5)
            s.update(pre=pre, y_f=yf)
            saved.append(s)
        if save_for_backward:
            self._saved = dict(layers=saved, q_in=q_in, B=B, nq=nq, Ne=Ne, We=We, scale=scale, enc2=enc2 if tr else None,
                               p=pd, seed=seed)
        return h.view(B, nq, D)

    def backward(self, dout: torch.Tensor, wgrads: bool = False, want_denc: bool = True):
        """dout [B,nq,D] f32 -> (d_query_embeds [B,nq,D] f32, d_enc [B,Nenc,We] f32, or None without want_denc).
        wgrads (trainable Q-Former, bind_trainable()): also write every weight, bias and LayerNorm gradient into the bound
        ParamStore's gradient views (overwritten; the caller zeroes / accumulates the flat buffer) -- weights through the TN
        product dY^T . X of the saved row-major operands, biases in the same launch, LayerNorm parameters beside each dgrad."""
        sv = self._saved
        if sv is None:
            raise RuntimeError("backward() without saved forward")
        if wgrads and (not self.trainable or sv["enc2"] is None):
            raise RuntimeError("backward(wgrads=True) needs bind_trainable() before the forward")
        B, nq, Ne, We, scale = sv["B"], sv["nq"], sv["Ne"], sv["We"], sv["scale"]
        D, H, hd = self.D, self.H, self.hd
        M = B * nq
        dh = dout.reshape(M, D).contiguous()
        dckv_all = torch.empty((B, Ne, self.n_cross * 2 * D), dtype=BF16, device=self.dev) if self.n_cross else None
        ci = self.n_cross
        eps = self.eps
        pd, seed = sv["p"], sv["seed"]
        sd_ = (lambda site: dropout_site_seed(seed, site)) if pd > 0 else (lambda site: 0)

        def ln_bwd(dh_, y, w, site):
            """(dL/dy f32 for the residual, dL/dz bf16 for the product) of LN(dropout(z) + res)."""
            if pd == 0:
                return ops.layernorm_bwd(dh_, y, w, eps, want_bf16=True)
            return ops.layernorm_bwd_dropout(dh_, y, w, eps, p_in=pd, seed_in=sd_(site))

        def wg(dyb, x, L, w, b):
            ops.gemm_tn_wgrad(dyb, x, L["g_" + w], bias=L["g_" + b])

        for li in reversed(range(len(self.layers))):
            L, s = self.layers[li], sv["layers"][li]
            # FFN:  h_out = LN(y_f),  y_f = dropout(act(h W1^T+b1) W2^T + b2) + h
            dy, dyb = ln_bwd(dh, s["y_f"], L["ln_f_w"], 5 * li + 5)
            if wgrads:
                ops.layernorm_param_grads(dh, s["y_f"], eps, L["g_ln_f_w"], L["g_ln_f_b"])
                wg(dyb, s["act"], L, "w2", "b2")
            dpre = ops.gemm_gelu_bwd(dyb, L["w2T"], s["pre"])        # gelu'(pre) in the dgrad's epilogue (one launch)
            if wgrads:
                wg(dpre, s["hb_f"], L, "w1", "b1")
            dh = ops.gemm(dpre, L["w1T"], residual=dy, out_dtype=F32)
            if L["cross"]:
                dy, dyb = ln_bwd(dh, s["y_c"], L["ln_c_w"], 5 * li + 4)
                if wgrads:
                    ops.layernorm_param_grads(dh, s["y_c"], eps, L["g_ln_c_w"], L["g_ln_c_b"])
                    wg(dyb, s["cctx"].view(M, D), L, "cwo", "cbo")
                dctx = ops.gemm(dyb, L["cwoT"]).view(B, nq, D)
                ckv = s["ckv"]
                ci -= 1
                dckv = dckv_all[:, :, ci * 2 * D:(ci + 1) * 2 * D]
                dcq, _, _ = ops.attn_bwd_dropout(s["cq"], ckv[:, :, :D], ckv[:, :, D:], s["cctx"], dctx, s["clse"], H, hd,
                                                 scale, pd, sd_(5 * li + 3), dk=dckv[:, :, :D], dv=dckv[:, :, D:])
                if wgrads:
                    wg(dcq.view(M, D), s["hb_a"], L, "cwq", "cbq")
                dh = ops.gemm(dcq.view(M, D), L["cwqT"], residual=dy, out_dtype=F32)
            dy, dyb = ln_bwd(dh, s["y_a"], L["ln_a_w"], 5 * li + 2)
            if wgrads:
                ops.layernorm_param_grads(dh, s["y_a"], eps, L["g_ln_a_w"], L["g_ln_a_b"])
                wg(dyb, s["ctx"].view(M, D), L, "wo", "bo")
            dctx = ops.gemm(dyb, L["woT"]).view(B, nq, D)
            qkv = s["qkv"]
            dqkv = torch.empty_like(qkv)
            ops.attn_bwd_dropout(qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:], s["ctx"], dctx, s["lse"], H, hd, scale,
                                 pd, sd_(5 * li + 1), dq=dqkv[:, :, :D], dk=dqkv[:, :, D:2 * D], dv=dqkv[:, :, 2 * D:])
            if wgrads:
                wg(dqkv.view(M, 3 * D), s["hb0"], L, "wqkv", "bqkv")
            dh = ops.gemm(dqkv.view(M, 3 * D), L["wqkvT"], residual=dy, out_dtype=F32)
        if pd > 0:
            dq_in, _ = ops.layernorm_bwd_dropout(dh, sv["q_in"], self.emb_w, eps, p_out=pd, seed_out=sd_(0), want_bf16=False)
        else:
            dq_in, _ = ops.layernorm_bwd(dh, sv["q_in"], self.emb_w, eps)
        if wgrads:
            ops.layernorm_param_grads(dh, sv["q_in"], eps, self.g_emb_w, self.g_emb_b, p_out=pd, seed_out=sd_(0))
            if self.n_cross:                              # every cross layer's key / value weights: ONE product over B*Nenc rows
                ops.gemm_tn_wgrad(dckv_all.view(B * Ne, self.n_cross * 2 * D), sv["enc2"], self.g_cwkv_all,
                                  bias=self.g_cbkv_all)
        if not want_denc:
            denc = None
        elif self.n_cross:                                # d(image tokens) = sum over the cross layers, as one K = n_cross*2D product
            denc = ops.gemm(dckv_all.view(B * Ne, self.n_cross * 2 * D), self.cwkvT_all, out_dtype=F32).view(B, Ne, We)
        else:
            denc = torch.zeros((B, Ne, We), dtype=F32, device=self.dev)
        self._saved = None
        return dq_in.view(B, nq, D), denc
