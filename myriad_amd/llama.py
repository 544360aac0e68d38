"""Vicuna / LLaMA decoder on the HIP kernels: training forward + dgrad-only backward, and KV-cache decode.

Mirrors the reference's `LlamaForCausalLM` (minigpt4/models/modeling_llama.py:629-716), `LlamaModel.forward`
(:466-596), `LlamaDecoderLayer.forward` (:247-299), `LlamaAttention.forward` (:168-231) and
`clamp_CE_loss` (:718-728) for the call patterns Myriad uses (inputs_embeds + attention_mask + labels; greedy
decode from inputs_embeds).  Weights are frozen (myriad.py:202-205), so the backward is dgrad only.

MI355X layout decisions (288 GB HBM): every frozen weight is kept twice in bf16 -- W [out,in] for forward and
W^T [in,out] for dgrad -- so forward and backward both run the single K-contiguous MFMA GEMM; q/k/v and
gate/up are fused into one GEMM each; the residual stream and all norm statistics are fp32; the lm_head and
the clamp-CE loss run only on label-bearing rows (the other rows have zero gradient and no loss term).
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib, ops

BF16, F32 = torch.bfloat16, torch.float32


def _bf(t: torch.Tensor, dev) -> torch.Tensor:
    return t.detach().to(device=dev, dtype=BF16).contiguous()


def _f32(t: torch.Tensor, dev) -> torch.Tensor:
    return t.detach().to(device=dev, dtype=F32).contiguous()


def decode_fp8_from_env() -> bool:
    """The default of LlamaHIP.decode_fp8: MYRIAD_DECODE_FP8=1 turns the FP8 weight-only token step on (off when unset)."""
    return os.environ.get("MYRIAD_DECODE_FP8", "0") != "0"


def decode_fp4_from_env() -> bool:
    """The default of LlamaHIP.decode_fp4: MYRIAD_DECODE_FP4=1 turns the MXFP4 weight-only token step on (off when unset)."""
    return os.environ.get("MYRIAD_DECODE_FP4", "0") != "0"


def decode_merge_lora_from_env() -> bool:
    """The default of LlamaHIP.decode_merge_lora: MYRIAD_DECODE_MERGE_LORA=1 folds the q/v LoRA into the token step's qkv copy
    (off when unset)."""
    return os.environ.get("MYRIAD_DECODE_MERGE_LORA", "0") != "0"


class LlamaHIP:
    def __init__(self, sd: Dict[str, torch.Tensor], n_heads: int, device, eps: float = 1e-6,
                 prefix: str = "llama_model.", max_pos: int = 2048, need_backward: bool = True):
        self.dev = torch.device(device)
        self.H = n_heads
        self.eps = eps
        p = prefix + "model."
        self.embed = _bf(sd[p + "embed_tokens.weight"], self.dev)
        self.V, self.D = self.embed.shape
        self.hd = self.D // n_heads
        self.layers: List[dict] = []
        i = 0
        while (p + f"layers.{i}.input_layernorm.weight") in sd:
            lp = p + f"layers.{i}."
            wq, wk, wv = (sd[lp + f"self_attn.{n}_proj.weight"] for n in "qkv")
            wqkv = _bf(torch.cat([wq, wk, wv], 0), self.dev)
            wo = _bf(sd[lp + "self_attn.o_proj.weight"], self.dev)
            # intermediate size padded to a multiple of 128 (the gate|up interleave block; also the GEMM K granule): zero
            # rows/cols are exact no-ops.  gate and up rows are interleaved in blocks of 128 so that one 256-column tile of the
            # gate|up GEMM holds g and u of the same columns and silu(g)*u rides its epilogue (ops.gemm_swiglu_fwd)
            wg, wu, wdn = sd[lp + "mlp.gate_proj.weight"], sd[lp + "mlp.up_proj.weight"], sd[lp + "mlp.down_proj.weight"]
            I0 = wg.shape[0]
            Ip = ops.round_up(I0, ops.SWIGLU_BLK)
            if Ip != I0:
                z = torch.zeros(Ip - I0, wg.shape[1], dtype=wg.dtype, device=wg.device)
                wg, wu = torch.cat([wg, z], 0), torch.cat([wu, z], 0)
                wdn = torch.cat([wdn, torch.zeros(wdn.shape[0], Ip - I0, dtype=wdn.dtype, device=wdn.device)], 1)
            wgu = ops.interleave_gate_up(_bf(wg, self.dev), _bf(wu, self.dev))
            wd = _bf(wdn, self.dev)
            L = dict(wqkv=wqkv, wo=wo, wgu=wgu, wd=wd,
                     ln1=_f32(sd[lp + "input_layernorm.weight"], self.dev),
                     ln2=_f32(sd[lp + "post_attention_layernorm.weight"], self.dev))
            if need_backward:
                L.update(wqkvT=wqkv.t().contiguous(), woT=wo.t().contiguous(), wguT=wgu.t().contiguous(),
                         wdT=wd.t().contiguous())
            self.layers.append(L)
            i += 1
        self.I = self.layers[0]["wd"].shape[1]
        self.norm = _f32(sd[p + "norm.weight"], self.dev)
        self.lm_head = _bf(sd[prefix + "lm_head.weight"], self.dev)
        self.Vpad = ops.round_up(self.V, 64)
        if need_backward:
            lmT = torch.zeros((self.D, self.Vpad), dtype=BF16, device=self.dev)
            lmT[:, :self.V] = self.lm_head.t()
            self.lm_headT = lmT
        inv_freq = 1.0 / (10000.0 ** (torch.arange(0, self.hd, 2).float() / self.hd))
        fr = torch.einsum("i,j->ij", torch.arange(max_pos).float(), inv_freq)
        self._pos_cache = {}
        self.cos = fr.cos().contiguous().to(self.dev)
        self.sin = fr.sin().contiguous().to(self.dev)
        self._saved = None
        self.lora = None
        # decode keeps a second, stream-ordered copy of the frozen weights (ops.gemv_pack; +1x the LLM's bf16 bytes, 13.5 GB
        # for Vicuna-7B out of 288 GB) built at the first generate(); MYRIAD_PACK_DECODE=0 streams the row-major ones
        self.pack_decode = os.environ.get("MYRIAD_PACK_DECODE", "1") != "0"
        # the LoRA weight gradients feed only the optimiser: queued during the dgrad chain, launched on a side stream after it
        # (55.7 -> 55.1 ms per step: they run beside the Q-Former backward); MYRIAD_LORA_DEFER=0 computes them in place
        self.defer_lora_wgrad = os.environ.get("MYRIAD_LORA_DEFER", "1") != "0"
        self.decode_fused = os.environ.get("MYRIAD_DECODE_FUSED", "1") != "0"
        # do_sample with 1 <= top_k <= 1024 draws on the device inside the token step (mh_sample_rows) instead of on the host;
        # off by default until it has been measured against the host draw (tools/decode_bench.py --sample)
        self.device_sampling = os.environ.get("MYRIAD_DEVICE_SAMPLING", "0") != "0"
        self.last_layer_rows = os.environ.get("MYRIAD_LAST_LAYER_ROWS", "1") != "0"
        # the packed token step streams FP8 (e4m3fn, one fp32 scale per output row) copies of the decoder matrices instead of
        # the bf16 ones (ops.gemv_pack_fp8; half the bytes, weight rounding the only new error); off by default, the attribute
        # wins over MYRIAD_DECODE_FP8
        self.decode_fp8 = decode_fp8_from_env()
        # the same with MXFP4 copies (ops.gemv_pack_fp4: e2m1 codes, one power-of-two scale byte per 32 k; 0.53 bytes per weight,
        # 4-bit round-to-nearest weights the only new error); off by default, the attribute wins over MYRIAD_DECODE_FP4, and it
        # excludes decode_fp8 (both on: ValueError when a decode call starts)
        self.decode_fp4 = decode_fp4_from_env()
        # with LoRA attached, the packed token step streams W_qkv with the q/v LoRA merged in (PEFT merge_adapter on the decode copy
        # only: LoraQV.merge) instead of the bordered wqkv_ext -- four launches per layer instead of five, and fp8 under decode_fp8;
        # the prefill and steps above GEMV_MAX_ROWS rows keep the exact bordered LoRA.  Off by default, the attribute wins over
        # MYRIAD_DECODE_MERGE_LORA.  The merge is redone only when decode_lora_version (set by its owner before a call: MyriadHIP
        # hands ParamStore.version) differs from the merged copy's; None re-merges at every call.
        self.decode_merge_lora = decode_merge_lora_from_env()
        self.decode_lora_version = None
        self._lora_merges = 0                                           # whole-model merges so far (last_generate_stats)
        self._packed = None                                             # the packed copies of the current kind (one of _packs)
        self._packs = {}                                                # "bf16" / "fp8" / "fp4" -> packed copies, each built on first use
        self._merge_rows = None                                         # fp4 merge: the row-major merged qkv of one layer (scratch)
        self._decode_ws = {}

    def _decode_kind(self) -> str:
        """What the packed token step streams: "fp8" / "fp4" under decode_fp8 / decode_fp4, else "bf16"; both on is an error."""
        if self.decode_fp8 and self.decode_fp4:
            raise ValueError("decode_fp8 and decode_fp4 are both on: the token step streams one kind of weight copy, turn one off")
        return "fp8" if self.decode_fp8 else "fp4" if self.decode_fp4 else "bf16"

    def _pack_quantised(self, kind: str, w: torch.Tensor, what: str, out=None):
        """The packed copy of one decoder matrix in `kind`; a matrix the fp4 packer does not take is an error that names it."""
        if kind == "fp4":
            if w.shape[1] % 128 != 0:
                raise _lib.MyriadHipError(f"decode_fp4: {what} has K = {w.shape[1]}, the MXFP4 copy needs a multiple of 128 "
                                          "(there is no fallback to another kind)")
            return ops.gemv_pack_fp4(w, out=out)
        return (ops.gemv_pack_fp8 if kind == "fp8" else ops.gemv_pack)(w, out=out)

    def _pack_for_decode(self) -> None:
        """(Re)build the packed copies the single-token step streams.  Frozen matrices are packed once; the bordered qkv
        weight carries the LoRA B columns, which training moves, so it is re-packed (in place) at every generate().
        With decode_fp8 the decoder matrices wo, wgu, wd -- and wqkv while no LoRA is attached -- are fp8 copies
        (ops.gemv_pack_fp8) in place of the bf16 ones; the bordered wqkv_ext (one row scale would be shared by W and the moving
        B columns) and lm_head (its arg-max picks the ids) stay bf16.  Each kind is built on its first use and kept, so flipping
        the switch between calls works, and the workspace key holds the kind: no graph captured on one is replayed on the other.
        With decode_merge_lora and LoRA attached the qkv entry is instead the [3D, D] copy with the q/v LoRA merged in
        (LoraQV.merge: fp8 under decode_fp8, bf16 otherwise), re-merged in place only when decode_lora_version is None or differs
        from the one it was merged for.  The bordered and the merged copies are both kept once built (the workspace key holds
        which one the step reads), so flipping decode_merge_lora frees no buffer that a captured graph reads.
        decode_fp4 is decode_fp8 with MXFP4 copies (ops.gemv_pack_fp4) -- the same matrices, the same ones left bf16 -- except that
        its merged qkv copy takes two launches per layer, ops.lora_merge into one row-major scratch and the packer."""
        kind = self._decode_kind()
        merge = self.lora is not None and self.decode_merge_lora
        qkv_key = "wqkv" if self.lora is None else ("merged" if merge else "wqkv_ext")
        P = self._packs.get(kind)
        if P is None:
            lm = next(iter(self._packs.values()))["lm_head"] if self._packs else ops.gemv_pack(self.lm_head)
            P = dict(kind=kind, layers=[{k: self._pack_quantised(kind, L[k], f"layer {i} {k}") for k in ("wo", "wgu", "wd")}
                                        for i, L in enumerate(self.layers)], lm_head=lm, qkv_key=None,
                     qkv={}, merged_for=None, merge_id=None)
            self._packs[kind] = P
        copies = P["qkv"].get(qkv_key)
        if merge:
            ver = self.decode_lora_version
            if copies is None or ver is None or P["merged_for"] != ver:
                if kind == "fp4":
                    rows = []
                    for i, L in enumerate(self.layers):
                        self._merge_rows = self.lora.merge_layer(i, L, "rows", self._merge_rows)
                        rows.append(self._pack_quantised(kind, self._merge_rows, f"layer {i} merged wqkv",
                                                         None if copies is None else copies[i]))
                    copies = rows
                else:
                    copies = self.lora.merge(self.layers, kind, copies)
                self._lora_merges += 1
                P["merged_for"], P["merge_id"] = ver, self._lora_merges
        elif copies is None or self.lora is not None:
            qkind = kind if self.lora is None else "bf16"
            copies = [self._pack_quantised(qkind, L[qkv_key], f"layer {i} {qkv_key}", None if copies is None else copies[i])
                      for i, L in enumerate(self.layers)]
        P["qkv"][qkv_key] = copies
        for Pl, c in zip(P["layers"], copies):
            Pl["wqkv"] = c
        P["qkv_key"] = qkv_key
        self._packed = P

    def _prepare_decode_weights(self, rows: int, wide: bool = False) -> dict:
        """Before a decode call at `rows` rows: the LoRA's bordered weights refreshed, the packed copies (re)built when the step
        can stream them (MYRIAD_PACK_DECODE=0 drops them: the step streams the row-major matrices).  Returns last_generate_stats'
        decode_weights ("fp8" / "fp4" / "bf16": what the token step streams) and decode_weight_bytes (the weight bytes of one token
        step: the packed copies, fp8 row scales / fp4 scale bytes included, up to GEMV_MAX_ROWS rows -- GEMV_WIDE_MAX_ROWS with `wide`, the slot engine's call; the row-major bf16 matrices above), lora_merged (the
        step streams the LoRA-merged qkv copy) and lora_merges (whole-model merges this model has made so far)."""
        self._decode_kind()                                             # both kinds on: an error whatever this call streams
        if self.lora is not None:
            self.lora.refresh(self.layers)
        if self.pack_decode and rows <= (ops.GEMV_WIDE_MAX_ROWS if wide else ops.GEMV_MAX_ROWS):
            self._pack_for_decode()                                     # wide: the slot engine's route to the copies above 16 rows
        elif not self.pack_decode:
            self._packed, self._packs = None, {}
        if _packed_step(self, rows, wide):
            mats = [P[k] for P in self._packed["layers"] for k in ("wqkv", "wo", "wgu", "wd")] + [self._packed["lm_head"]]
            nbytes = sum(m.data.numel() * m.data.element_size()
                         + (m.scales.numel() * m.scales.element_size() if hasattr(m, "scales") else 0) for m in mats)
            return dict(decode_weights=self._packed["kind"], decode_weight_bytes=int(nbytes),
                        lora_merged=self._packed["qkv_key"] == "merged", lora_merges=self._lora_merges)
        qkv_key = "wqkv" if self.lora is None else "wqkv_ext"
        mats = [L[k] for L in self.layers for k in (qkv_key, "wo", "wgu", "wd")] + [self.lm_head]
        return dict(decode_weights="bf16", decode_weight_bytes=int(sum(m.numel() * m.element_size() for m in mats)),
                    lora_merged=False, lora_merges=self._lora_merges)

    def attach_lora(self, lora) -> None:
        """Enable PEFT-style LoRA on q_proj/v_proj (myriad_amd.lora.LoraQV); replaces W_qkv by its bordered copy."""
        for L in self.layers:
            lora.extend_weights(L)
        self.lora = lora

    # ------------------------------------------------------------------ training forward
    def forward_loss(self, x: torch.Tensor, attention_mask: torch.Tensor, labels: torch.Tensor,
                     save_for_backward: bool = True, lora_training: Optional[bool] = None) -> torch.Tensor:
        """x: [B,S,D] f32 inputs_embeds (device); attention_mask/labels: [B,S] CPU or device int64.
        Returns the 0-d f32 loss tensor (device).  Stores what `backward()` needs."""
        B, S, D = x.shape
        M = B * S
        H, hd, W = self.H, self.hd, self.D
        am = attention_mask.to("cpu")
        kv_len_host = am.sum(-1).to(torch.int32)
        if not bool((am == (torch.arange(S)[None] < kv_len_host[:, None])).all()):
            raise ValueError("attention_mask must be right-padded (ones then zeros), as the reference builds it")
        kv_len = ops.h2d(kv_len_host, self.dev)                         # async uploads: no launch-thread stall
        pos = self._pos_ids(B, S)                                       # position_ids = arange (modeling_llama.py:519-523)
        scale = 1.0 / math.sqrt(hd)
        h = x.reshape(M, D)
        saved = []
        lora = self.lora
        if lora is not None:
            lora.refresh(self.layers)
        # The RMSNorm that consumes a residual-stream GEMM rides that GEMM's split-K reduce (ops.gemm_residual_rmsnorm):
        # o_proj -> post-attention norm, down_proj -> the NEXT layer's input norm (written straight into that layer's
        # bordered LoRA operand when LoRA is on).  Only layer 0's input norm is a launch of its own.
        def norm_target(li):
            if lora is None:
                return None
            return lora.x_ext(li, M)[:, :D]

        # whole-sequence attention with the rotary embedding fused (csrc/attn_seq.hip) when the sequence fits a CU's LDS:
        # qkv is then saved PRE-rotary and the backward kernel rotates again / un-rotates dq, dk itself
        fused_attn = ops.attn_rope_supported(S, hd) and os.environ.get("MYRIAD_ATTN_SEQ", "1") != "0"
        # loss on label-bearing rows only: row (b,s) predicts labels[b,s+1]
        lab = labels.to("cpu")
        shift = lab[:, 1:]
        bi, si = torch.nonzero(shift != -100, as_tuple=True)
        n_valid = int(bi.numel())
        if n_valid == 0:
            raise ValueError("no valid labels")
        row_idx = (bi * S + si).to(torch.int32)
        rows = ops.h2d(row_idx, self.dev)
        tgt = ops.h2d(shift[bi, si], self.dev)
        # The LAST layer's o_proj, post-attention norm and MLP (modeling_llama.py:281-293) run on those rows only: the other rows
        # of its output feed nothing (the final norm and lm_head read label rows), and in the backward their gradient is exactly
        # zero down to that layer's attention, which mixes rows -- so its k / v projections and everything below stay dense.
        # Identical results, ~1.4 % fewer executed FLOPs at the bench shape; MYRIAD_LAST_LAYER_ROWS=0 keeps every row.
        # (not for <= 16 label rows, the batch-1 step: those products would run on the weight-streaming GEMV, which reads the
        # row-major matrices slower than the 160-row tiles run all 148 rows -- measured +0.25 ms per batch-1 step)
        last_rows = self.last_layer_rows and len(self.layers) > 0 and 16 < n_valid <= M // 2
        inv = None
        if last_rows:
            inv_host = torch.full((M,), -1, dtype=torch.int32)
            inv_host[row_idx.long()] = torch.arange(n_valid, dtype=torch.int32)
            inv = ops.h2d(inv_host, self.dev)
        xn = ops.rmsnorm_fwd(h, self.layers[0]["ln1"], self.eps, out=norm_target(0)) if self.layers else None
        hr = None
        for li, L in enumerate(self.layers):
            lsave = None
            if lora is None:
                qkv = ops.gemm(xn, L["wqkv"])                               # [M, 3W] bf16
            else:   # q/v LoRA rides the qkv GEMM as a 64-column K border (myriad_amd/lora.py)
                x_ext = lora.x_ext(li, M)                                   # [:, :D] already holds rmsnorm(h)
                p_eff, seed = lora.forward_border(li, x_ext, training=save_for_backward if lora_training is None
                                                  else lora_training)
                qkv = ops.gemm(x_ext, L["wqkv_ext"])
                lsave = (x_ext, p_eff, seed)
            q3 = qkv.view(B, S, 3 * W)
            if fused_attn:
                o, lse = ops.attn_rope_fwd(q3, H, hd, scale, pos, self.cos, self.sin, kv_len=kv_len)
            else:
                ops.rope_(qkv, 0, 2 * H, hd, pos, self.cos, self.sin, 1.0)  # q and k heads
                o, lse = ops.attn_fwd(q3[:, :, :W], q3[:, :, W:2 * W], q3[:, :, 2 * W:], H, hd, scale, causal=True,
                                      kv_len=kv_len)
            if last_rows and li + 1 == len(self.layers):
                o_r = ops.gather_rows(o.view(M, W), rows)                   # [R, W] bf16
                h_r = ops.gather_rows(h, rows)                              # [R, D] f32
                h2, xn2 = ops.gemm_residual_rmsnorm(o_r, L["wo"], h_r, L["ln2"], self.eps)
                gu, act = ops.gemm_swiglu_fwd(xn2, L["wgu"])
                hr = ops.gemm(act, L["wd"], residual=h2, out_dtype=F32)     # the final hidden state of the label rows
                if save_for_backward:
                    saved.append((h, qkv, o, lse, h2, gu, lsave))
                break
            h2, xn2 = ops.gemm_residual_rmsnorm(o.view(M, W), L["wo"], h, L["ln2"], self.eps)
            gu, act = ops.gemm_swiglu_fwd(xn2, L["wgu"])                    # [M, 2I] (interleaved g|u blocks), [M, I]
            if li + 1 < len(self.layers):
                h3, xn = ops.gemm_residual_rmsnorm(act, L["wd"], h2, self.layers[li + 1]["ln1"], self.eps,
                                                   y_out=norm_target(li + 1))
            else:
                h3 = ops.gemm(act, L["wd"], residual=h2, out_dtype=F32)     # the final norm runs on label rows only
            if save_for_backward:
                saved.append((h, qkv, o, lse, h2, gu, lsave))
            h = h3
        if hr is None:
            hr = ops.gather_rows_f32(h, rows)
        hn = ops.rmsnorm_fwd(hr, self.norm, self.eps)
        logits = ops.gemm(hn, self.lm_head, out_dtype=F32)                  # [R, V] f32
        row_loss, dlogits = ops.clamp_ce(logits, tgt, 1.0 / n_valid, want_grad=save_for_backward, ldd=self.Vpad)
        loss = ops.sum_f32(row_loss, 1.0 / n_valid)
        if save_for_backward:
            self._saved = dict(layers=saved, rows=rows, hr=hr, dlogits=dlogits, B=B, S=S, kv_len=kv_len, pos=pos,
                               scale=scale, fused_attn=fused_attn, inv=inv)
        return loss.view(())

    # ------------------------------------------------------------------ dgrad-only backward
    def backward(self, loss_scale: float = 1.0, defer_lora_join: bool = False) -> torch.Tensor:
        """Returns d(loss)/d(inputs_embeds) as [B,S,D] f32.  The LoRA weight gradients of all layers are launched on a side
        stream once the dgrad chain is done; with defer_lora_join the caller joins them (lora.join_wgrads()) after its own
        remaining backward work, otherwise they are joined here."""
        sv = self._saved
        if sv is None:
            raise RuntimeError("backward() called without a saved forward")
        B, S = sv["B"], sv["S"]
        M, D, W, H, hd = B * S, self.D, self.D, self.H, self.hd
        dlog = sv["dlogits"]
        if loss_scale != 1.0:
            raise NotImplementedError("loss scaling is unnecessary in bf16; pass 1.0")
        dhn = ops.gemm(dlog, self.lm_headT, out_dtype=F32)                  # [R, D]
        dhr, _ = ops.rmsnorm_bwd(dhn, sv["hr"], self.norm, self.eps)
        inv = sv.get("inv")
        if inv is None:
            dh = torch.zeros((M, D), dtype=F32, device=self.dev)
            ops.scatter_rows(dhr, sv["rows"], dh)
            dh_b = ops.to_bf16(dh)
        n_layers = len(self.layers)
        for ri, (L, (h_in, qkv, o, lse, h2, gu, lsave)) in enumerate(zip(reversed(self.layers), reversed(sv["layers"]))):
            li = n_layers - 1 - ri
            rows_mode = inv is not None and ri == 0      # the last layer ran its o_proj / MLP on the label rows only (forward_loss)
            if rows_mode:
                dgu = ops.gemm_swiglu_bwd(ops.to_bf16(dhr), L["wdT"], gu)   # [R, 2I]: every other row's gradient is exactly zero
                dh2_r, dh2_rb = ops.gemm_rmsnorm_bwd(dgu, L["wguT"], h2, L["ln2"], self.eps, dres=dhr)
                do_r = ops.gemm(dh2_rb, L["woT"])                           # [R, W] bf16
                dh2 = ops.expand_rows(dh2_r, inv, M)                        # back to all rows (zeros elsewhere): the residual path
                do = ops.expand_rows(do_r, inv, M)                          # ... and the attention's dO
            else:
                dgu = ops.gemm_swiglu_bwd(dh_b, L["wdT"], gu)               # down dgrad + gate backward: [M, 2I]
                # gate|up dgrad [M, D] and the post-attention norm's backward in one call (split-K slabs summed in the norm kernel)
                dh2, dh2_b = ops.gemm_rmsnorm_bwd(dgu, L["wguT"], h2, L["ln2"], self.eps, dres=dh)
            q3 = qkv.view(B, S, 3 * W)
            dqkv = torch.empty_like(qkv)
            d3 = dqkv.view(B, S, 3 * W)
            if rows_mode:
                if sv["fused_attn"]:
                    ops.attn_rope_bwd(q3, o, do.view(B, S, W), lse, H, hd, sv["scale"], sv["pos"], self.cos, self.sin,
                                      kv_len=sv["kv_len"], dqkv=d3)
                else:
                    ops.attn_bwd(q3[:, :, :W], q3[:, :, W:2 * W], q3[:, :, 2 * W:], o, do.view(B, S, W), lse, H, hd,
                                 sv["scale"], causal=True, kv_len=sv["kv_len"], dq=d3[:, :, :W], dk=d3[:, :, W:2 * W],
                                 dv=d3[:, :, 2 * W:])
                    ops.rope_(dqkv, 0, 2 * H, hd, sv["pos"], self.cos, self.sin, -1.0)
            elif sv["fused_attn"]:
                # o_proj dgrad + attention backward: the split-K slabs of dO are summed inside the attention kernel
                ops.gemm_attn_rope_bwd(dh2_b, L["woT"], q3, o, lse, H, hd, sv["scale"], sv["pos"], self.cos, self.sin,
                                       kv_len=sv["kv_len"], dqkv=d3)
            else:
                do = ops.gemm(dh2_b, L["woT"])                              # [M, W] bf16
                ops.attn_bwd(q3[:, :, :W], q3[:, :, W:2 * W], q3[:, :, 2 * W:], o, do.view(B, S, W), lse, H, hd,
                             sv["scale"], causal=True, kv_len=sv["kv_len"], dq=d3[:, :, :W], dk=d3[:, :, W:2 * W],
                             dv=d3[:, :, 2 * W:])
                ops.rope_(dqkv, 0, 2 * H, hd, sv["pos"], self.cos, self.sin, -1.0)
            if self.lora is None:
                dxn = ops.gemm(dqkv, L["wqkvT"], out_dtype=F32)
                dh, dh_b = ops.rmsnorm_bwd(dxn, h_in, L["ln1"], self.eps, dres=dh2, want_bf16=True)
            else:
                # [M, D+64] = base dgrad | d(s*t), the LoRA correction of d(xn) and the input norm's backward in one call: the
                # split-K slabs are summed inside the one kernel that does both (csrc/lora.hip)
                dh, dh_b = self.lora.backward_from_dqkv_norm(li, dqkv, L["wqkvT_ext"], lsave[0], lsave[1], lsave[2], h_in,
                                                             L["ln1"], self.eps, dh2, defer_wgrad=self.defer_lora_wgrad)
        self._saved = None
        if self.lora is not None:
            self.lora.run_deferred_wgrads()
            if not defer_lora_join:
                self.lora.join_wgrads()
        return dh.view(B, S, D)

    def _pos_ids(self, B: int, S: int) -> torch.Tensor:
        key = (B, S)
        if key not in self._pos_cache:
            self._pos_cache[key] = torch.arange(S, dtype=torch.int32).repeat(B).to(self.dev)
        return self._pos_cache[key]

    # ------------------------------------------------------------------ generation
    def _decode_block(self, h, B, S, caches, scale, pos, past=None, pos_dev=None, kvlen_dev=None, split_ws=None, live=None,
                      ragged=None, wide=False):
        """All decoder layers for a prefill chunk (host-known `past`: the chunk's rows go to cache rows past..past+S-1, `pos` holds
        their rotary positions, and causal masking is aligned to the bottom right) or for one decode token whose position lives
        in device memory (`pos_dev`/`kvlen_dev`), which makes the launch sequence replayable from a hipGraph.  `split_ws` (the
        partials buffer of ops.attn_decode_split_ws) makes the fused token step use the split-KV attention kernel.  `live` (int32
        [B] on the device, the slot engine's) makes it the rows kernel instead: every row appends at its own pos[b], idle rows
        are skipped; only the fused step has that form.  Both together: the split-KV kernel in its rows form
        (ops.attn_decode_rope_split_rows), at 1 to GEMV_WIDE_MAX_ROWS rows alike.
        `ragged` = (segment table on the device, its host copy) makes a prefill the packed one (_prefill_packed): B = 1, the S rows hold several requests, `caches` are the whole slot caches, and the
        three attention launches become one mh_attn_prefill_ragged (mh_attn_prefill_ragged_past for a table with a fourth column,
        the rows cached already).  `wide` (the slot engine above GEMV_MAX_ROWS slots) keeps the
        token step on the packed copies up to GEMV_WIDE_MAX_ROWS rows: the fused step's launch sequence with
        ops.gemv_packed_wide as the product and the two-launch forms of the norm / SiLU products, as at 3 to 16 rows.  Every
        other caller leaves it off and keeps the row-major GEMMs above GEMV_MAX_ROWS rows."""
        H, hd, W, D = self.H, self.hd, self.D, self.D
        M = B * S
        packed = self._packed["layers"] if pos_dev is not None and _packed_step(self, M, wide) else None
        wide = packed is not None and M > ops.GEMV_MAX_ROWS
        gemv = ops.gemv_packed_wide if wide else ops.gemv_packed
        if live is not None and not (packed is not None and self.decode_fused):
            raise ValueError("per-row decode state needs the fused packed token step")
        # the bordered LoRA product unless the packed qkv copy has the LoRA merged in (decode_merge_lora)
        lora = None if packed is not None and self._packed["qkv_key"] == "merged" else self.lora

        def lin(li, name, x, **kw):
            if packed is not None:
                return ops.gemv_packed(x, packed[li]["wqkv" if name.startswith("wqkv") else name], **kw)
            return ops.gemm(x, self.layers[li][name], **kw)

        # Single-token step on the packed copies: four launches per layer instead of nine -- the two RMSNorms
        # and the SiLU gate are rebuilt by every workgroup of the product that consumes them (mh_gemv_packed_rmsnorm /
        # _silu), rotary + KV append ride the attention launch (mh_attn_decode_rope); each fused form is bit-identical
        # to the launches it replaces (tests/test_kernels_gpu.py), MYRIAD_DECODE_FUSED=0 keeps the separate launches.
        # With LoRA attached the qkv product takes the bordered operand [xn | s A xn]: the norm and the LoRA down projection are
        # one launch (LoraQV.norm_border, <= 2 rows), the bordered packed weight the next -- five launches per layer become six.
        # With the LoRA merged into the packed qkv copy (decode_merge_lora) the step is the no-LoRA one.
        fused = packed is not None and self.decode_fused
        for li, (L, cache) in enumerate(zip(self.layers, caches)):
            if fused:
                P = packed[li]
                if lora is not None:
                    x_ext = lora.x_ext(li, M)
                    if not lora.norm_border(li, h, L["ln1"], self.eps, x_ext):
                        ops.rmsnorm_fwd(h, L["ln1"], self.eps, out=x_ext[:, :D])
                        lora.forward_border(li, x_ext, training=False)
                    qkv = gemv(x_ext, P["wqkv"])
                else:
                    qkv = None if wide else ops.gemv_packed_rmsnorm(h, L["ln1"], self.eps, P["wqkv"])
                    if qkv is None:
                        qkv = gemv(ops.rmsnorm_fwd(h, L["ln1"], self.eps), P["wqkv"])
                if live is not None and split_ws is not None:
                    o = ops.attn_decode_rope_split_rows(qkv, cache, pos, kvlen_dev, live, self.cos, self.sin, H, hd, scale, split_ws)
                elif live is not None:
                    o = ops.attn_decode_rope_rows(qkv, cache, pos, kvlen_dev, live, self.cos, self.sin, H, hd, scale)
                elif split_ws is not None:
                    o = ops.attn_decode_rope_split(qkv, cache, pos, pos_dev, kvlen_dev, self.cos, self.sin, H, hd, scale, split_ws)
                else:
                    o = ops.attn_decode_rope(qkv, cache, pos, pos_dev, kvlen_dev, self.cos, self.sin, H, hd, scale)
                h2 = gemv(o, P["wo"], residual=h, out_dtype=F32)
                gu = None if wide else ops.gemv_packed_rmsnorm(h2, L["ln2"], self.eps, P["wgu"])
                if gu is None:
                    gu = gemv(ops.rmsnorm_fwd(h2, L["ln2"], self.eps), P["wgu"])
                hn = None if wide else ops.gemv_packed_silu(gu, P["wd"], residual=h2, out_dtype=F32)
                h = hn if hn is not None else gemv(ops.silu_mul_fwd_blk(gu), P["wd"], residual=h2, out_dtype=F32)
                continue
            if lora is None:
                xn = ops.rmsnorm_fwd(h, L["ln1"], self.eps)
                qkv = lin(li, "wqkv", xn)
            else:
                x_ext = lora.x_ext(li, M)
                ops.rmsnorm_fwd(h, L["ln1"], self.eps, out=x_ext[:, :D])
                lora.forward_border(li, x_ext, training=False)
                qkv = lin(li, "wqkv_ext", x_ext)
            q3 = qkv.view(B, S, 3 * W)
            if ragged is not None:
                attn = ops.attn_prefill_ragged_past if ragged[1].shape[1] == 4 else ops.attn_prefill_ragged
                o = attn(qkv, pos, ragged[0], ragged[1], cache, self.cos, self.sin, H, hd, scale)
            elif pos_dev is None:
                ops.rope_(qkv, 0, 2 * H, hd, pos, self.cos, self.sin, 1.0)
                ops.copy3d_bf16(q3[:, :, W:], cache[:, past:past + S])       # append k|v (modeling_llama.py:190-195)
                kc = cache[:, :past + S]
                o, _ = ops.attn_fwd(q3[:, :, :W], kc[:, :, :W], kc[:, :, W:], H, hd, scale, causal=True, need_lse=False)
            else:
                ops.rope_kv_append(qkv, H, hd, pos, self.cos, self.sin, cache, pos_dev)   # rotary + append, one launch
                o, _ = ops.attn_fwd(q3[:, :, :W], cache[:, :, :W], cache[:, :, W:], H, hd, scale, causal=False,
                                    kv_len=kvlen_dev, need_lse=False)
            h2 = lin(li, "wo", o.view(M, W), residual=h, out_dtype=F32)
            xn2 = ops.rmsnorm_fwd(h2, L["ln2"], self.eps)
            act = ops.silu_mul_fwd_blk(lin(li, "wgu", xn2))
            h = lin(li, "wd", act, residual=h2, out_dtype=F32)
        return h

    def _decode_workspace(self, B: int, T_need: int, inv_temp: float, dev_sample: bool = False, penalty: bool = False,
                          num_beams: int = 1):
        """_decode_buffers (and, once captured, the hipGraph) of the single-token step for a batch size, kept across generate()
        calls -- an evaluation run calls generate() once per batch, and re-capturing ~290 launches each time cost ~9 ms per
        call.  The device sampler and the repetition penalty read their knobs and the seed from device memory, so the key holds
        only whether each is on; the arg-max kernel takes inv_temp as an argument, so it stays in the key there."""
        T_cap = ops.round_up(T_need + 2, 64)
        key = (B, T_cap, None if dev_sample else float(inv_temp), _decode_weights_id(self), bool(dev_sample), bool(penalty),
               int(num_beams))
        ws = self._decode_ws.get(key)
        if ws is None:
            if len(self._decode_ws) >= 3:                               # a few shapes at most: evict the oldest
                self._decode_ws.pop(next(iter(self._decode_ws)))
            ws = self._decode_ws[key] = _decode_buffers(self, B, T_cap, dev_sample or penalty, num_beams)
        return ws

    def _prefill(self, inputs_embeds: torch.Tensor, caches, past: int = 0) -> torch.Tensor:
        """The prefill (eager, host-known lengths) of positions past.. of [B, S0, D] f32 embeddings into `caches`, on top of the
        `past` rows cached already; returns the last position's f32 logits [B, V]."""
        B, S0, D = inputs_embeds.shape
        S = S0 - past
        pos = torch.arange(past, S0, dtype=torch.int32).repeat(B).to(self.dev)
        h = self._decode_block(inputs_embeds[:, past:].reshape(B * S, D).contiguous(), B, S, caches, 1.0 / math.sqrt(self.hd), pos,
                               past=past)
        last = h.view(B, S, D)[:, -1].contiguous()
        return ops.gemm(ops.rmsnorm_fwd(last, self.norm, self.eps), self.lm_head, out_dtype=F32)

    def _prefill_packed(self, embs, slots, caches, pasts=None) -> torch.Tensor:
        """The prefill of several requests in ONE pass over the decoder weights (the slot engine's prefill_batch > 1): `embs` is a
        list of [S_i, D] f32 embeddings, request i goes to positions 0 .. S_i - 1 of slot slots[i] of `caches` (the slot engine's
        [slots, T, 2D] caches, whole).  The rows are packed one request after the other, `pos` = each row's index within its
        request, and the row count is rounded up to a multiple of 64 with zero rows that belong to no segment (LoraQV.x_ext keeps
        a buffer per row count and the GEMM planner keys on it: a run meets a handful of shapes).  The layers are the prefill
        branch of _decode_block -- norms, GEMMs, the bordered LoRA, MLP -- with its three attention launches replaced by
        mh_attn_prefill_ragged; then the R last rows are gathered for the final norm and the lm-head.  Returns [R, V] f32 logits.
        A request's rows differ from its solo _prefill only through the GEMMs' row-count-dependent plans.

        `pasts` (SlotDecoder.run_turns): request i has its first pasts[i] rows in slot slots[i] already, so only embs[i][pasts[i]:]
        is packed, at positions pasts[i] .., and the attention launch is mh_attn_prefill_ragged_past -- the packed form of
        _prefill(emb, cache, past).  Without it the launches are the ones above."""
        if pasts is not None:
            pasts = [int(p) for p in pasts]
            if len(pasts) != len(embs) or any(not 0 <= p < int(e.shape[0]) for p, e in zip(pasts, embs)):
                raise ValueError("pasts: one per request, 0 <= past < its rows")
            embs = [e[p:] for e, p in zip(embs, pasts)]
        lens = [int(e.shape[0]) for e in embs]
        M, D = ops.round_up(sum(lens), 64), self.D
        x = torch.zeros((M, D), dtype=F32, device=self.dev)
        pos = torch.zeros((M,), dtype=torch.int32)
        seg, row = [], 0
        for i, (e, n, s) in enumerate(zip(embs, lens, slots)):
            x[row:row + n].copy_(e)
            if pasts is None:
                pos[row:row + n] = torch.arange(n, dtype=torch.int32)
                seg.append((row, n, int(s)))
            else:
                pos[row:row + n] = torch.arange(pasts[i], pasts[i] + n, dtype=torch.int32)
                seg.append((row, n, int(s), pasts[i]))
            row += n
        seg_host = torch.tensor(seg, dtype=torch.int32)
        last = torch.tensor([t[0] + t[1] - 1 for t in seg], dtype=torch.int32)
        h = self._decode_block(x, 1, M, caches, 1.0 / math.sqrt(self.hd), ops.h2d(pos, self.dev),
                               ragged=(ops.h2d(seg_host, self.dev), seg_host))
        hl = ops.gather_rows_f32(h, ops.h2d(last, self.dev))
        return ops.gemm(ops.rmsnorm_fwd(hl, self.norm, self.eps), self.lm_head, out_dtype=F32)

    def _step_logits(self, ws: dict) -> None:
        """The token step up to its logits: embed the fed ids ws["ids"], every decoder layer at the device-resident position,
        the final norm + lm-head into ws["logits"] -- one launch on the packed copy when the fused form fits, else the norm and
        the packed GEMV, or the GEMM above GEMV_MAX_ROWS rows (the wide packed GEMV there for a workspace marked `wide`: the
        slot engine's)."""
        ops.embed_gather(self.embed, ws["ids"], ws["x_in"])
        rows = ws["x_in"].shape[0]
        wide = bool(ws.get("wide"))
        h = self._decode_block(ws["x_in"], rows, 1, ws["caches"], 1.0 / math.sqrt(self.hd), ws["pos"], pos_dev=ws["pos"],
                               kvlen_dev=ws["kvlen"], split_ws=ws["split"], live=ws.get("live"), wide=wide)
        if _packed_step(self, rows) and self.decode_fused:
            if ops.gemv_packed_rmsnorm(h, self.norm, self.eps, self._packed["lm_head"], out=ws["logits"], out_dtype=F32) is not None:
                return
        hn = ops.rmsnorm_fwd(h, self.norm, self.eps)
        if _packed_step(self, rows):
            ops.gemv_packed(hn, self._packed["lm_head"], out=ws["logits"], out_dtype=F32)
        elif _packed_step(self, rows, wide):
            ops.gemv_packed_wide(hn, self._packed["lm_head"], out=ws["logits"], out_dtype=F32)
        else:
            ops.gemm(hn, self.lm_head, out=ws["logits"])

    @staticmethod
    def _launch_step(ws: dict, token_step, ban: int, use_graph: bool, stats: dict) -> None:
        """Enqueue one token step: a replay of ws's captured graph when there is one (counted in stats["graph_replays"]).  A step
        with a ban runs eagerly; an eager ban-free step after an earlier eager one captures the next (kernels are warm, buffers
        fixed)."""
        if ban == -1 and use_graph and ws["graph"] is not None:
            ws["graph"].replay()
            stats["graph_replays"] += 1
            return
        token_step(ban)
        if ban == -1 and use_graph and ws["warm"]:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                token_step(-1)
            ws["graph"] = g
        ws["warm"] = True

    @torch.no_grad()
    def greedy_generate(self, inputs_embeds: torch.Tensor, max_new_tokens: int = 90,
                        stop_ids=((835,), (2277, 29937)), eos_id: int = 2, min_length: int = 1,
                        return_margins: bool = False, use_graph: bool = True, do_sample: bool = False,
                        top_p: float = 1.0, temperature: float = 1.0, generator: Optional[torch.Generator] = None,
                        top_k: int = 50, repetition_penalty: float = 1.0):
        """Decode from [B,S0,D] f32 embeddings with a KV cache (prefill + 1-token steps).  Same contract
        as the oracle's greedy_generate: stop when ROW 0 ends with a stop sequence (conversation.py:102-107),
        EOS banned while fewer than `min_length` tokens were generated, finished rows padded with EOS.

        The single-token step (~290 launches) is captured into a hipGraph once per batch size, kept across generate() calls
        (an evaluation run calls generate() once per batch) and replayed; everything it needs lives on the device -- position /
        valid-length counters, and the token it just picked is fed back as the next input by the step itself
        (mh_decode_record), which packs the step's picks into one small record: between two steps the host makes ONE
        device->host copy.  (Measured and dropped: launching step t+1 before reading step t -- back-to-back launches of one
        executable graph cost more than the host's 0.07 ms per step; writing the record straight into pinned host memory --
        +0.2 ms per token.)

        `do_sample=True, top_p, temperature` are the eval script's arguments (evaluation_aqa_dataset.py:289-301).  HF's
        top-p warper keeps the smallest descending-probability set whose mass reaches top_p (at least one token), so a
        step whose p_max >= top_p IS the arg-max; the kernel reports p_max per row and only a row below the threshold is
        drawn on the host from that row's logits (a genuine sample: reproducible here through `generator`, never
        bit-comparable with another framework's RNG) and replaces the fed-back id.  `last_generate_stats` counts such steps.
        The host draw applies HF's default `top_k = 50` filter first, then top-p; the device test p_max >= top_p is taken over the
        full vocabulary, which is the conservative side: the top-k renormalisation only raises p_max, and a row whose
        renormalised p_max reaches top_p keeps exactly one token in the host draw -- the arg-max again.

        With `device_sampling` (MYRIAD_DEVICE_SAMPLING=1) and 1 <= top_k <= 1024 the whole chain runs inside the step instead
        (mh_sample_rows: temperature, top-k with ties kept, top-p, inverse-CDF draw from Philox4x32-10 keyed by one seed drawn from
        `generator` per call): every step is a draw, no row waits on the host, and runs are reproducible per seed but not
        bit-comparable with torch.multinomial.  A row whose tied top-k set passes 1024 candidates is still drawn on the host.
        `repetition_penalty` (HF RepetitionPenaltyLogitsProcessor over the generated ids; the prompt is embeddings only) is applied
        on the device to the step's logits before any pick, greedy, host or device draw."""
        return self._greedy_core(inputs_embeds, None, max_new_tokens=max_new_tokens, stop_ids=stop_ids, eos_id=eos_id,
                                 min_length=min_length, return_margins=return_margins, use_graph=use_graph, do_sample=do_sample,
                                 top_p=top_p, temperature=temperature, generator=generator, top_k=top_k,
                                 repetition_penalty=repetition_penalty)

    def _greedy_core(self, inputs_embeds: torch.Tensor, session, max_new_tokens: int = 90, stop_ids=((835,), (2277, 29937)),
                     eos_id: int = 2, min_length: int = 1, return_margins: bool = False, use_graph: bool = True,
                     do_sample: bool = False, top_p: float = 1.0, temperature: float = 1.0,
                     generator: Optional[torch.Generator] = None, top_k: int = 50, repetition_penalty: float = 1.0):
        """greedy_generate's body.  session=None: its workspace from the _decode_ws cache and a prefill from position 0; a
        DecodeSession instead lends its own buffers and graphs and names the cached prefix `past` that is not prefilled again."""
        B, S0, _ = inputs_embeds.shape
        if do_sample and not float(temperature) > 0:
            raise ValueError(f"temperature must be > 0 when sampling, got {temperature}")
        if not float(repetition_penalty) > 0:
            raise ValueError(f"repetition_penalty must be > 0, got {repetition_penalty}")
        out_ids, margins = [], []
        unfinished = torch.ones(B, dtype=torch.long)
        inv_temp = 1.0 / float(temperature) if do_sample else 1.0
        top_k = 0 if top_k is None else int(top_k)
        dev_sample = (self.device_sampling and do_sample and 1 <= top_k <= ops.SAMPLE_CAP and self.V <= 32768
                      and self.V % 4 == 0)
        penalty = float(repetition_penalty) != 1.0
        stats = dict(steps=0, sampled_rows=0, min_pmax=1.0, device_sampled_rows=0, host_sampled_rows=0, graph_replays=0)
        self.last_generate_stats = stats
        stats.update(self._prepare_decode_weights(B))
        if session is None:
            ws, past = self._decode_workspace(B, S0 + max_new_tokens, inv_temp, dev_sample, penalty), 0
        else:
            ws, past = session._begin_turn(B, S0, max_new_tokens, inv_temp, dev_sample, penalty)
        rec = ws["rec"][:4 if dev_sample else 3]                     # the sampler's kept counts are the fourth row
        if dev_sample or penalty:
            ws["prm"].copy_(torch.tensor([inv_temp, top_p, float(top_k), float(repetition_penalty)], dtype=F32))
            ws["seen"].zero_()                                       # generated ids only: the prompt is embeddings
        if dev_sample:
            ws["seed"].fill_(int(torch.randint(0, 2**63 - 1, (1,), generator=generator)))

        def sample_row(logits_row: torch.Tensor, ban: int) -> int:
            return _host_draw(logits_row, ban, inv_temp, top_k, top_p, generator)

        def record(nxt: torch.Tensor, mar: torch.Tensor, pm: torch.Tensor, ban: int, logits_of=None, kept=None):
            """Host bookkeeping of one step's picks.  Returns (done, redrawn): redrawn = a live row was re-drawn on the host
            (finished rows are fed their raw arg-max instead of EOS by the device: rows are independent and their outputs are
            overwritten with EOS here)."""
            nonlocal unfinished
            margins.append(mar)
            stats["steps"] += 1
            redrawn = False
            if do_sample:
                stats["min_pmax"] = min(stats["min_pmax"], float(pm[unfinished.bool()].min()) if int(unfinished.sum()) else 1.0)
                for row in range(B):
                    if not int(unfinished[row]):
                        continue
                    if float(pm[row]) < top_p:
                        stats["sampled_rows"] += 1
                    if dev_sample and int(kept[row]) >= 0:
                        stats["device_sampled_rows"] += 1            # drawn by the step itself
                    elif dev_sample or float(pm[row]) < top_p:
                        nxt[row] = sample_row(logits_of()[row], ban)
                        stats["host_sampled_rows"] += 1
                        redrawn = True
            nxt = nxt * unfinished + eos_id * (1 - unfinished)       # HF pads finished rows with pad(=eos)
            unfinished = unfinished * (nxt != eos_id).long()
            out_ids.append(nxt)
            row0 = [int(t[0]) for t in out_ids]
            if any(len(row0) >= len(st) and row0[-len(st):] == list(st) for st in stop_ids):
                return True, redrawn
            return int(unfinished.max()) == 0, redrawn

        logits0 = self._prefill(inputs_embeds, ws["caches"], past)
        ban0 = eos_id if 0 < min_length else -1
        if dev_sample:                                               # the prefill pick is Philox step t = 0
            ops.sample_rows(logits0, ws["nxt"], ws["mar"], ws["pmx"], ws["kept"], ws["prm"], ws["seed"], ban_id=ban0, t_add=0)
        else:
            ops.argmax_pmax_rows(logits0, ws["nxt"], ws["mar"], ws["pmx"], ban_id=ban0, inv_temp=inv_temp)
        done, _ = record(ws["nxt"].cpu(), ws["mar"].cpu(), ws["pmx"].cpu(), ban0, logits_of=lambda: logits0,
                         kept=ws["kept"].cpu() if dev_sample else None)

        # ---- single-token steps: everything the step reads is on the device
        ws["pos"].fill_(S0)                                          # position of the incoming token
        ws["kvlen"].fill_(S0 + 1)                                    # valid keys after the append
        ws["step"].zero_()

        def token_step(ban):
            self._step_logits(ws)
            if penalty:                                              # ws["ids"] = the token fed in: it joins the seen set first
                ops.repetition_penalty_rows(ws["logits"], ws["seen"], ws["ids"], ws["prm"][3:])
            if dev_sample:                                           # token s (= step + 1) draws Philox step t = s
                ops.sample_rows(ws["logits"], ws["nxt"], ws["mar"], ws["pmx"], ws["kept"], ws["prm"], ws["seed"], ban_id=ban,
                                step=ws["step"], t_add=1)
                ops.decode_advance_kept(ws["nxt"], ws["mar"], ws["pmx"], ws["kept"], rec, ws["ids"], ws["step"], ws["pos"],
                                        ws["kvlen"])
                return
            ops.argmax_pmax_rows(ws["logits"], ws["nxt"], ws["mar"], ws["pmx"], ban_id=ban, inv_temp=inv_temp)
            ops.decode_advance(ws["nxt"], ws["mar"], ws["pmx"], rec, ws["ids"], ws["step"], ws["pos"], ws["kvlen"])

        step = 1                                                     # tokens generated so far (= index of the next one)
        if not done and step < max_new_tokens:
            ws["ids"].copy_(out_ids[-1].to(self.dev))
        while not done and step < max_new_tokens:
            ban = eos_id if step < min_length else -1
            self._launch_step(ws, token_step, ban, use_graph, stats)
            r = rec.cpu()                                            # the one device->host copy of the step (it also waits for it)
            done, redrawn = record(r[0].long(), r[1].clone(), r[2].clone(), ban, logits_of=lambda: ws["logits"],
                                   kept=r[3] if dev_sample else None)
            if redrawn and not done:
                ws["ids"].copy_(out_ids[-1].to(self.dev))            # a host draw replaces the arg-max the step fed back to itself
            step += 1
        ids = torch.stack(out_ids, 1)
        if return_margins:
            return ids, torch.stack(margins, 1)
        return ids

    @torch.no_grad()
    def beam_generate(self, inputs_embeds: torch.Tensor, num_beams: int, max_new_tokens: int = 90, stop_ids=(), eos_id: int = 2,
                      min_length: int = 1, length_penalty: float = 1.0, early_stopping=False, num_return_sequences: int = 1,
                      use_graph: bool = True, return_scores: bool = False, pad_id: Optional[int] = None):
        """Beam search from [B,S0,D] f32 embeddings: HF GenerationMixin._beam_search (tests/beam_ref.py states the rules).
        Returns [B * num_return_sequences, L] int64 (CPU), generated ids only, the hypotheses of item b at rows
        b * nrs .. b * nrs + nrs - 1 best first, right-padded with pad_id (default EOS); with return_scores also their
        sequence scores (sum log-probs / len ** length_penalty), which last_generate_stats["sequences_scores"] holds either way.

        Stop rule: a hypothesis finishes when its own sequence ends with EOS or with one of `stop_ids` (per hypothesis, as
        transformers applies a criterion that returns one bool per row), or at max_new_tokens.  greedy_generate keeps the
        reference's rule instead (the batch stops when row 0 ends with a stop sequence).

        Device / host split.  The prefill runs at B rows, writing its keys / values into row b * nb of the B * nb row caches,
        and one mh_beam_reorder_kv broadcasts them over [0, S0) to the item's other beams.  The token step (captured into a
        hipGraph, like greedy's) is: reorder the generated positions [S0, pos) of every cache by the parent rows `src`, embed
        the fed tokens, the decoder layers at B * nb rows (packed GEMV up to GEMV_MAX_ROWS), lm-head, mh_beam_topk (log-softmax +
        running score + EOS ban, per item the top 2 * nb candidates), pos / kvlen += 1.  The host reads the [2, B, 2*nb]
        record (one device->host copy), keeps the hypotheses, and writes the next step's (ids, src, running scores) with one
        host->device copy."""
        B, S0, _ = inputs_embeds.shape
        nb, nrs = int(num_beams), int(num_return_sequences)
        if nb > ops.BEAM_MAX:
            raise NotImplementedError(f"num_beams={nb}: at most {ops.BEAM_MAX} beams on the HIP decode path")
        if nb < 1:
            raise ValueError(f"num_beams must be >= 1, got {nb}")
        if not 1 <= nrs <= nb:
            raise ValueError(f"num_return_sequences={nrs} must be between 1 and num_beams={nb}")
        if early_stopping not in (True, False, "never"):
            raise ValueError(f"early_stopping must be True, False or 'never', got {early_stopping!r}")
        if self.V < 2 * nb:
            raise ValueError(f"num_beams={nb} needs a vocabulary of at least {2 * nb} tokens")
        lp = float(length_penalty)
        pad = eos_id if pad_id is None else int(pad_id)
        stops = [tuple(int(t) for t in st) for st in stop_ids]
        R, K, V, NEG = B * nb, 2 * nb, self.V, np.float32(-1.0e9)
        stats = dict(steps=0, num_beams=nb, graph_replays=0, finished_hypotheses=0, sequences_scores=None, lengths=None)
        self.last_generate_stats = stats
        stats.update(self._prepare_decode_weights(R))
        ws = self._decode_workspace(R, S0 + max_new_tokens, 1.0, num_beams=nb)
        caches, T_cap, C = ws["caches"], ws["T"], 2 * self.D
        dev = self.dev

        # ---- host state of the search (HF's tensors, per item, as small numpy arrays / lists)
        run_seqs = [[()] * nb for _ in range(B)]
        fin_scores = np.full((B, nb), NEG, dtype=np.float32)
        fin_seqs = [[()] * nb for _ in range(B)]
        is_fin = np.zeros((B, nb), dtype=bool)
        unsat = np.ones((B,), dtype=bool)
        host = ws["bupd_host"]
        h_ids, h_src, h_sc = host[:2 * R].view(torch.long).numpy(), host[2 * R:3 * R].numpy(), host[3 * R:].view(F32).numpy()

        def select(top_s: np.ndarray, top_i: np.ndarray, gen_len: int) -> bool:
            """One step's bookkeeping from the record (top_s / top_i [B, K]); fills the upload; True = go on."""
            nonlocal unsat
            stats["steps"] += 1
            all_hit = True
            for b in range(B):
                par, tok = top_i[b] // V, top_i[b] % V
                cand = [run_seqs[b][int(par[k])] + (int(tok[k]),) for k in range(K)]
                hits = np.array([c[-1] == eos_id or gen_len >= max_new_tokens
                                 or any(len(c) >= len(st) and c[-len(st):] == st for st in stops) for c in cand])
                all_hit &= bool(hits.all())
                run_lp = top_s[b] + hits.astype(np.float32) * NEG
                nxt = np.argsort(-run_lp, kind="stable")[:nb]
                run_seqs[b] = [cand[k] for k in nxt]
                h_ids[b * nb:(b + 1) * nb] = tok[nxt]
                h_src[b * nb:(b + 1) * nb] = b * nb + par[nxt]
                h_sc[b * nb:(b + 1) * nb] = run_lp[nxt]
                did = hits.copy()
                did[nb:] = False                                     # only the top nb candidates may enter the pool
                sc = top_s[b] / np.float32(gen_len ** lp)
                if is_fin[b].all() and early_stopping is True:
                    sc = sc + NEG
                if not unsat[b]:
                    sc = sc + NEG
                sc = sc + (~did).astype(np.float32) * NEG
                merged = np.concatenate([fin_scores[b], sc])
                keep = np.argsort(-merged, kind="stable")[:nb]
                mseqs, mfin = fin_seqs[b] + cand, np.concatenate([is_fin[b], did])
                fin_scores[b], fin_seqs[b], is_fin[b] = merged[keep], [mseqs[k] for k in keep], mfin[keep]
                best_len = max_new_tokens if (early_stopping == "never" and lp > 0.0) else gen_len
                best_run = np.float32(h_sc[b * nb]) / np.float32(best_len ** lp)
                worst = fin_scores[b].min()
                unsat[b] = unsat[b] and bool(np.any(np.where(is_fin[b], best_run > worst, best_run > NEG)))
            return bool(unsat.any()) and not (bool(is_fin.all()) and early_stopping is True) and not all_hit

        def read_record():
            rec = ws["brec"].cpu()                                   # the one device->host copy of the step
            return rec[0].view(F32).numpy().reshape(B, K), rec[1].numpy().reshape(B, K).astype(np.int64)

        # ---- prefill at B rows into rows b * nb, then broadcast the prompt's keys / values to the other beams
        logits0 = self._prefill(inputs_embeds, [c[::nb] for c in caches])
        ws["bscore"].zero_()                                         # beam 0's running score; one row per item here
        ops.beam_topk(logits0, ws["bscore"], ws["part_s"], ws["part_i"], ws["brec"][0].view(F32), ws["brec"][1], B, nb,
                      ban_id=eos_id if 0 < min_length else -1)
        if self.layers:
            # a range of its own: ws["lo"] holds the previous call's S0 when the workspace is reused
            bsrc = torch.arange(B, dtype=torch.int32).repeat_interleave(nb).mul_(nb).to(dev)
            span = torch.tensor([0, S0], dtype=torch.int32).to(dev)
            ops.beam_reorder_kv(ws["table"], len(caches), B, nb, T_cap, C, bsrc, span[:1], span[1:])
        going = select(*read_record(), 1)

        # ---- token steps
        ws["pos"].fill_(S0)
        ws["kvlen"].fill_(S0 + 1)
        ws["lo"].fill_(S0)                                           # the prompt prefix is the same in every beam of an item

        def token_step(ban):
            ops.beam_reorder_kv(ws["table"], len(caches), B, nb, T_cap, C, ws["src"], ws["lo"], ws["pos"])
            self._step_logits(ws)
            ops.beam_topk(ws["logits"], ws["bscore"], ws["part_s"], ws["part_i"], ws["brec"][0].view(F32), ws["brec"][1], B, nb,
                          ban_id=ban, pos=ws["pos"], kvlen=ws["kvlen"])

        gen = 1                                                      # tokens generated so far
        while going and gen < max_new_tokens:
            ws["bupd"].copy_(ws["bupd_host"], non_blocking=True)    # ids | src | running scores: one host->device copy
            self._launch_step(ws, token_step, eos_id if gen < min_length else -1, use_graph, stats)
            gen += 1
            going = select(*read_record(), gen)

        seqs = [fin_seqs[b][i] for b in range(B) for i in range(nrs)]
        scores = torch.from_numpy(np.array([fin_scores[b, i] for b in range(B) for i in range(nrs)], dtype=np.float32))
        ids = torch.full((len(seqs), max(1, max(len(q) for q in seqs))), pad, dtype=torch.long)
        for r, q in enumerate(seqs):
            ids[r, :len(q)] = torch.tensor(q, dtype=torch.long)
        stats.update(sequences_scores=scores, finished_hypotheses=int(is_fin.sum()), lengths=[len(q) for q in seqs])
        return (ids, scores) if return_scores else ids

    def slot_decoder(self, slots: int, capacity: int, split_kv: Optional[bool] = False) -> "SlotDecoder":
        """A decode-slot engine over this model: `slots` rows of one captured token step, each decoding its own request of up to
        `capacity` positions (prompt + generated).  `split_kv`: the step's attention kernel (False: the single-workgroup rows
        kernel, True: the split-KV rows kernel, None: split_kv_rows_rule per call).  See SlotDecoder."""
        return SlotDecoder(self, slots, capacity, split_kv=split_kv)

    def embed_tokens_into(self, ids: torch.Tensor, out2d: torch.Tensor, dst_rows: Optional[torch.Tensor] = None):
        ops.embed_gather(self.embed, ids, out2d, dst_rows)


def _host_draw(logits_row: torch.Tensor, ban: int, inv_temp: float, top_k: int, top_p: float, generator) -> int:
    """HF TopKLogitsWarper + TopPLogitsWarper + multinomial on one row (host)."""
    lg = logits_row.float().cpu() * inv_temp
    if ban >= 0:
        lg[ban] = float("-inf")
    if top_k and 0 < top_k < lg.numel():                             # HF applies TopKLogitsWarper (default top_k = 50) before top-p
        lg = lg.masked_fill(lg < torch.topk(lg, top_k).values[-1], float("-inf"))
    srt, idx = torch.sort(lg, descending=False)
    cum = srt.softmax(-1).cumsum(-1)
    remove = cum <= (1.0 - top_p)
    remove[-1:] = False                                              # min_tokens_to_keep = 1
    srt = srt.masked_fill(remove, float("-inf"))
    probs = torch.zeros_like(lg).scatter(0, idx, srt.softmax(-1))
    return int(torch.multinomial(probs, 1, generator=generator))


# Decode helpers shared by LlamaHIP and DecodeSession.  They read only the model's fields, so the session needs no more of the
# model than those.
def _packed_step(lm: "LlamaHIP", rows: int, wide: bool = False) -> bool:
    """The token step at `rows` rows streams the packed copies (ops.gemv_packed takes at most GEMV_MAX_ROWS rows).  `wide`: the
    caller is the slot engine, which stays on them up to GEMV_WIDE_MAX_ROWS rows (ops.gemv_packed_wide); the other decode
    loops never pass it, so their routing above GEMV_MAX_ROWS rows is the row-major GEMM as before."""
    return lm._packed is not None and rows <= (ops.GEMV_WIDE_MAX_ROWS if wide else ops.GEMV_MAX_ROWS)


def _decode_weights_id(lm: "LlamaHIP") -> tuple:
    """What the token step multiplies by: the packed copies (which object, its kind, which qkv copy is live), the fused
    launches and the LoRA.  The workspace key holds it, so no graph captured on one set of weights is replayed on another."""
    P = lm._packed
    return id(P), None if P is None else (P["kind"], P["qkv_key"]), lm.decode_fused, lm.lora is not None


def _decode_buffers(lm: "LlamaHIP", B: int, T_cap: int, sampler: bool = False, num_beams: int = 1) -> dict:
    """Buffers of the single-token step at B rows: KV caches of T_cap positions, device-resident counters, id / logit /
    result buffers and the [4, B] per-step record (the arg-max step writes its first three rows); `graph` / `warm` hold the
    captured step once there is one (_launch_step), `split` the split-KV partials when the step uses them.  With `sampler`
    the device sampler's and the repetition penalty's buffers join: their knobs (`prm` = inv_temp, top_p, top_k, penalty),
    the seed, the kept counts and the seen-id bitmaps.  With num_beams > 1, B counts rows (items x beams) and the beam step's
    buffers join: `bupd` = the per-step upload (ids int64 | parent rows int32 | running scores f32) and its pinned host twin,
    the top-K scratch and record, and the device table of the per-layer cache pointers that mh_beam_reorder_kv walks."""
    dev, i32 = lm.dev, torch.int32
    ws = dict(T=T_cap, graph=None, warm=False, split=None,
              caches=[torch.zeros((B, T_cap, 2 * lm.D), dtype=BF16, device=dev) for _ in lm.layers],
              pos=torch.zeros((B,), dtype=i32, device=dev), kvlen=torch.zeros((B,), dtype=i32, device=dev),
              ids=torch.zeros((B,), dtype=torch.long, device=dev), x_in=torch.empty((B, lm.D), dtype=F32, device=dev),
              logits=torch.empty((B, lm.V), dtype=F32, device=dev),
              nxt=torch.empty((B,), dtype=torch.long, device=dev), mar=torch.empty((B,), dtype=F32, device=dev),
              pmx=torch.empty((B,), dtype=F32, device=dev), step=torch.zeros((1,), dtype=i32, device=dev),
              rec=torch.zeros((4, B), dtype=F32, device=dev))
    if sampler:
        ws.update(prm=torch.zeros((4,), dtype=F32, device=dev), seed=torch.zeros((1,), dtype=torch.long, device=dev),
                  kept=torch.zeros((B,), dtype=i32, device=dev),
                  seen=torch.zeros((B, (lm.V + 31) // 32), dtype=i32, device=dev))
    if num_beams > 1:
        nb, K = int(num_beams), 2 * int(num_beams)
        bupd = torch.zeros((4 * B,), dtype=i32, device=dev)
        ws.update(bupd=bupd, bupd_host=torch.zeros((4 * B,), dtype=i32).pin_memory(),
                  ids=bupd[:2 * B].view(torch.long), src=bupd[2 * B:3 * B], bscore=bupd[3 * B:].view(F32),
                  part_s=torch.empty((B * K,), dtype=F32, device=dev), part_i=torch.empty((B * K,), dtype=i32, device=dev),
                  brec=torch.zeros((2, B // nb * K), dtype=i32, device=dev), lo=torch.zeros((1,), dtype=i32, device=dev),
                  table=torch.tensor([c.data_ptr() for c in ws["caches"]], dtype=torch.long).to(dev))
    return ws


# The chat session's token step uses the split-KV attention kernel (mh_attn_decode_rope_split) when the single-workgroup kernel
# leaves most CUs idle and the cached context is long enough for the chunks to pay for the merge launch: B*H workgroups < 256 (the
# CU count) and at least SPLIT_KV_MIN_KEYS keys when the turn starts.  Measured at batch 1 on the full-size model
# (tools/chat_bench.py): ms per token split / single = 3.04 / 2.89 at 256 keys, 3.23 / 3.33 at 1,024,
# 3.39 / 3.86 at 2,048.  Each kernel has its own captured graph in the session; the choice is made per turn.
SPLIT_KV_MAX_ROWHEADS = 256
SPLIT_KV_MIN_KEYS = 1024


def split_kv_rule(B: int, H: int, kv_len: int) -> bool:
    return B * H < SPLIT_KV_MAX_ROWHEADS and kv_len >= SPLIT_KV_MIN_KEYS


# The slot engine's form of the rule (SlotDecoder(split_kv=None)): `live_rows` conversations decode in one call, the longest has
# `max_kv_len` keys when it is admitted.  It says yes only where the split rows kernel was measured faster than the single-workgroup
# rows kernel on the full-size model (tools/chat_bench.py --pool-split, DESIGN.md section 5, "Chat pool"; ms per token step,
# split_kv False / True, both pools interleaved in one process): N = 1: 3.390 / 3.218 at 1,136 keys, 3.961 / 3.463 at 2,160;
# N = 2: 3.688 / 3.578 and 4.235 / 3.875; N = 4: 3.982 / 3.987 and 4.562 / 4.619 -- at 128 row-heads the split kernel no longer
# wins.  So: at most 64 row-heads (the largest product at which split won) and at least 1,024 keys (the shortest context at which
# it won; the section 5 table says what was measured below that).
SPLIT_KV_ROWS_MAX_ROWHEADS = 64
SPLIT_KV_ROWS_MIN_KEYS = 1024


def split_kv_rows_rule(live_rows: int, H: int, max_kv_len: int) -> bool:
    return live_rows * H <= SPLIT_KV_ROWS_MAX_ROWHEADS and max_kv_len >= SPLIT_KV_ROWS_MIN_KEYS


def common_prefix(a, b) -> int:
    """Length of the longest common prefix of two key lists (the position keys of a context and of a cache)."""
    n = min(len(a), len(b))
    for i in range(n):
        if a[i] != b[i]:
            return i
    return n


class DecodeSession:
    """A decode KV cache that outlives one call: the multi-turn chat's (myriad_amd/chat.py).  It owns its buffers -- the per-layer
    caches, pos / kvlen / ids / records, the sampler's buffers, the split-KV partials -- and its captured token-step graphs, so no
    other generate() (whose workspaces live in the LlamaHIP._decode_ws LRU) can evict them.

    The session records one key per cached position (`keys[row][p]`): whatever the caller uses to name that position's input, a
    ("t", token id) for text and an image-slot / index pair for image rows.  A turn (`generate`) prefills only the rows past the
    longest common prefix of the new context's keys with the cached ones -- at their own positions, on top of the cached rows --
    then runs greedy_generate's token step on the session's buffers.  Afterwards the cache holds the context plus every token the
    step fed back (the last pick of a turn has no KV and is not counted; a row that finished early feeds ids the host does not
    know, recorded as a key that matches nothing).

    The whole cache is dropped (full prefill, `last_stats["full_reprefill_reason"]`) when the caller's weights version changes
    (optimiser update, state-dict load), when the decode weights change kind (bf16 / fp8 / fp4, LoRA on / off, the LoRA-merged qkv copy
    on / off or re-merged: "decode weights changed"), when the batch size changes, when the capacity (round_up(need + 2, 64), at
    most 8192) is exceeded, or when the caller says so (`reset_reason`: the chat's truncation window moved)."""

    def __init__(self, llama: "LlamaHIP", capacity: int, split: Optional[bool] = None):
        self.llama = llama
        self.capacity = min(8192, ops.round_up(int(capacity), 64))
        self.split_choice = split                                    # None: split_kv_rule per turn; True / False force it
        self.bufs = None
        self.B = None
        self.keys: List[list] = []
        self.stamp = None
        self.views = {}                                              # cfg -> workspace view of bufs, with its graph / warm flag
        self.graph_captures = 0
        self.split = False
        self.last_stats = {}
        self._turn = None

    def _begin_turn(self, B: int, S0: int, max_new_tokens: int, inv_temp: float, dev_sample: bool, penalty: bool):
        """Called by LlamaHIP._greedy_core once the decode weights are packed: invalidation, (re)allocation, the reused prefix.
        Returns (workspace, past)."""
        L = self.llama
        keys, version, reason = self._turn
        if S0 + max_new_tokens > L.cos.shape[0]:
            raise ValueError(f"context {S0} + max_new_tokens {max_new_tokens} passes the rotary table ({L.cos.shape[0]} positions)")
        if len(keys) != B or any(len(k) != S0 for k in keys):
            raise ValueError("one key per context position and batch row is required")
        # the merged qkv copy is rewritten in place by a re-merge: its merge id joins the stamp, so no KV row survives a change of
        # the weights the step multiplies by, whether or not the caller's weights_version saw it
        P = L._packed
        stamp = (version, _decode_weights_id(L), P["merge_id"] if P is not None and P["qkv_key"] == "merged" else None)
        need = S0 + max_new_tokens + 2
        if self.bufs is None:
            reason = reason or "empty cache"
        elif self.B != B:
            reason = "batch size"
        elif self.stamp[0] != version:
            reason = "weights changed"
        elif self.stamp[1:] != stamp[1:]:
            reason = "decode weights changed"
        elif need > self.bufs["T"]:
            reason = "capacity"
        if self.bufs is None or self.B != B or need > self.bufs["T"] or (self.stamp is not None and self.stamp[1:] != stamp[1:]):
            T_cap = max(self.capacity, ops.round_up(need, 64))
            if T_cap > 8192:
                raise ValueError(f"a chat session holds at most 8192 positions; this turn needs {need}")
            self.bufs, self.views = None, {}
            self.bufs, self.B = _decode_buffers(L, B, T_cap, sampler=True), B
        self.stamp = stamp
        if reason is not None:
            self.keys = [[] for _ in range(B)]
        past = min(common_prefix(keys[r], self.keys[r]) for r in range(B))
        past = min(past, S0 - 1)                                     # at least one row is prefilled: it gives the first logits
        fused = _packed_step(L, B) and L.decode_fused
        self.split = fused and (split_kv_rule(B, L.H, S0) if self.split_choice is None else bool(self.split_choice))
        if self.split and self.bufs["split"] is None:
            self.bufs["split"] = ops.attn_decode_split_ws(B, L.H, self.bufs["T"], L.dev)
        cfg = (None if dev_sample else float(inv_temp), bool(dev_sample), bool(penalty), self.split)
        ws = self.views.get(cfg)
        if ws is None:
            ws = self.views[cfg] = dict(self.bufs, split=self.bufs["split"] if self.split else None)
        self._ws, self._ws_graph = ws, ws["graph"]
        self.last_stats = dict(context_tokens=S0, reused_tokens=past, prefilled_tokens=S0 - past, split_kv=bool(self.split),
                               full_reprefill_reason=reason)
        return ws, past

    @torch.no_grad()
    def generate(self, inputs_embeds: torch.Tensor, keys, weights_version=None, reset_reason: Optional[str] = None, **kw):
        """One turn: greedy_generate's contract and arguments (`max_new_tokens`, `stop_ids`, `eos_id`, `min_length`, `do_sample`,
        `top_p`, `temperature`, `generator`, `top_k`, `repetition_penalty`, `return_margins`) on [B, S0, D] f32 embeddings whose
        positions are named by `keys` ([B][S0]).  `weights_version`: anything that changes when the weights do."""
        B, S0, _ = inputs_embeds.shape
        self._turn, self._ws = ([list(k) for k in keys], weights_version, reset_reason), None
        try:
            out = self.llama._greedy_core(inputs_embeds, self, use_graph=True, **kw)
        except BaseException:
            self.keys = [[] for _ in range(B)]                       # the cache may be half written
            raise
        finally:
            self._turn = None
            if self._ws is not None and self._ws["graph"] is not self._ws_graph:    # this turn captured its view's step
                self.graph_captures += 1
        ids = out[0] if isinstance(out, tuple) else out
        eos = int(kw.get("eos_id", 2))
        n = ids.shape[1]
        new_keys = []
        for r in range(B):
            row, fed, live = ids[r].tolist(), [], True
            for k in range(n - 1):                                   # token step k + 1 fed pick k at position S0 + k
                fed.append(("t", row[k]) if live else ("x",))
                live = live and row[k] != eos
            new_keys.append(list(keys[r]) + fed)
        self.keys = new_keys
        st = self.llama.last_generate_stats
        self.last_stats.update(steps=st["steps"], graph_replays=st["graph_replays"], graph_captures=self.graph_captures)
        return out


class SlotScheduler:
    """The bookkeeping of a decode-slot run, on plain Python values (no device in sight, so a scripted step can drive it): which
    free slot takes which request, each slot's own ids and margins, when a slot finishes -- EOS, a stop sequence at the end of
    ITS ids (kept in the output, as greedy_generate keeps row 0's), or max_new_tokens -- and the order results leave in.

    One round of a run: `admit` requests into `free()` slots until none is free or the requests run out (a request whose first
    pick already ends it never occupies a slot), then, while `live()`, one token step whose per-slot picks go to `step`.
    `pop()` hands out finished (index, ids, margins): in completion order, or with `ordered` in admission (= input) order, a
    result waiting for every earlier one."""

    def __init__(self, slots: int, max_new_tokens: int, stop_ids=(), eos_id: int = 2, ordered: bool = False):
        if slots < 1 or max_new_tokens < 1:
            raise ValueError(f"slots and max_new_tokens must be >= 1, got {slots} and {max_new_tokens}")
        self.slots, self.max_new_tokens, self.eos_id, self.ordered = int(slots), int(max_new_tokens), int(eos_id), bool(ordered)
        self.stops = [tuple(int(t) for t in st) for st in stop_ids]
        self.rows = [None] * self.slots                              # per slot: [index, ids, margins] while it decodes
        self.admitted = 0
        self._done, self._next_out = {}, 0
        self.steps = self.live_row_steps = 0

    def free(self) -> list:
        return [s for s in range(self.slots) if self.rows[s] is None]

    def live(self) -> list:
        return [s for s in range(self.slots) if self.rows[s] is not None]

    def _ended(self, ids: list) -> bool:
        return (ids[-1] == self.eos_id or len(ids) >= self.max_new_tokens
                or any(len(ids) >= len(st) and tuple(ids[-len(st):]) == st for st in self.stops))

    def _finish(self, row) -> None:
        self._done[row[0]] = (row[0], row[1], row[2])

    def admit(self, slot: int, first_id: int, margin: float) -> bool:
        """The next request (index = how many were admitted before it) with its prefill pick.  True: it decodes on in `slot`."""
        if self.rows[slot] is not None:
            raise ValueError(f"slot {slot} is busy")
        row = [self.admitted, [int(first_id)], [float(margin)]]
        self.admitted += 1
        if self._ended(row[1]):
            self._finish(row)
            return False
        self.rows[slot] = row
        return True

    def step(self, ids, margins) -> list:
        """One token step's picks, indexed by slot (idle slots' entries are ignored).  Returns the slots that finished."""
        live = self.live()
        self.steps += 1
        self.live_row_steps += len(live)
        finished = []
        for s in live:
            row = self.rows[s]
            row[1].append(int(ids[s]))
            row[2].append(float(margins[s]))
            if self._ended(row[1]):
                self._finish(row)
                self.rows[s] = None
                finished.append(s)
        return finished

    def pop(self) -> list:
        if not self.ordered:
            out = [self._done.pop(k) for k in list(self._done)]      # dicts keep insertion (= completion) order
        else:
            out = []
            while self._next_out in self._done:
                out.append(self._done.pop(self._next_out))
                self._next_out += 1
        return out

    @property
    def occupancy(self) -> float:
        return self.live_row_steps / (self.steps * self.slots) if self.steps else 0.0


class RefillPlanner:
    """Which waiting requests are prefilled together, and when: the host side of the slot engine's packed prefill, on plain Python
    values like SlotScheduler (whose free / live slots it reads), so a scripted run can drive it.

    `next_pass()` is asked at every refill point until it answers []: it hands out [(slot, request), ...] for ONE prefill pass --
    the next waiting requests in input order, one per free slot in ascending slot order, at most `prefill_batch` of them and as
    many as keep the pass's row count (the lengths' sum rounded up to 64) within `prefill_rows`; the first always goes, so a
    request too long to share a pass, or longer than the cap, gets a pass of its own.  `refill_min` = k holds a pass back while
    fewer than k slots are free, unless nothing is live or the requests have run out (the input ended and everything left is
    waiting already: the planner looks one request past the pass it could fill).  prefill_batch = 1, refill_min = 1 is the
    engine's one-request refill: the lowest free slot takes the next request, again if that one ended on its first pick."""

    def __init__(self, sched: "SlotScheduler", requests, prefill_batch: int = 1, prefill_rows: int = 2048, refill_min: int = 1,
                 length=len):
        if prefill_batch < 1 or refill_min < 1 or prefill_rows < 1:
            raise ValueError(f"prefill_batch, refill_min and prefill_rows must be >= 1, got {prefill_batch}, {refill_min} and "
                             f"{prefill_rows}")
        self.sched, self.it, self.more, self.waiting, self.length = sched, iter(requests), True, [], length
        self.prefill_batch, self.prefill_rows = int(prefill_batch), int(prefill_rows)
        self.refill_min = min(int(refill_min), sched.slots)
        self.passes = self.packed_rows = 0

    def next_pass(self) -> list:
        free = self.sched.free()
        if not free:
            return []
        want = min(self.prefill_batch, len(free))
        while self.more and len(self.waiting) < want + (self.refill_min > 1):    # refill_min = 1 never needs to look ahead
            try:
                self.waiting.append(next(self.it))
            except StopIteration:
                self.more = False
        if not self.waiting or (len(free) < self.refill_min and self.sched.live() and self.more):
            return []
        n, rows = 0, 0
        for req in self.waiting[:want]:
            if n and ops.round_up(rows + self.length(req), 64) > self.prefill_rows:
                break
            n, rows = n + 1, rows + self.length(req)
        group, self.waiting = self.waiting[:n], self.waiting[n:]
        self.passes += 1
        self.packed_rows += rows
        return list(zip(free, group))


class TurnPlanner:
    """RefillPlanner's place in SlotDecoder.run_turns: every turn has ITS session's slot, so the passes are fixed when the call
    starts -- the turns in list order, up to `prefill_batch` per pass and as many as keep the pass's NEW rows (rounded up to 64)
    within `prefill_rows`; the first of a pass always goes.  `items` = [(slot, request)], `length(request)` = its new rows."""

    def __init__(self, items, prefill_batch: int = 1, prefill_rows: int = 2048, length=len):
        if prefill_batch < 1 or prefill_rows < 1:
            raise ValueError(f"prefill_batch and prefill_rows must be >= 1, got {prefill_batch} and {prefill_rows}")
        self.groups, self.passes, self.packed_rows = [], 0, 0
        rows = 0
        for item in items:
            n = length(item[1])
            if not self.groups or len(self.groups[-1]) >= int(prefill_batch) or ops.round_up(rows + n, 64) > int(prefill_rows):
                self.groups.append([])
                rows = 0
            self.groups[-1].append(item)
            rows += n
        self._length = length

    def next_pass(self) -> list:
        if not self.groups:
            return []
        group = self.groups.pop(0)
        self.passes += 1
        self.packed_rows += sum(self._length(req) for _, req in group)
        return group


class SessionTable:
    """Which conversation lives in which decode slot, and what its slot's cache holds: the host side of SlotDecoder.run_turns, on
    plain Python values like SlotScheduler (no device in sight).

    At most `slots` sessions are open; a session (any object: hashable ones by value, others by identity, held until `close`)
    is pinned to one slot from its first turn until `close(session)` frees it.  Per session the table keeps one key per cached
    position, DecodeSession's convention: `begin(session, keys)` answers (slot, past, reason) with past =
    min(common_prefix(keys, cached), len(keys) - 1) -- at least one row is always prefilled, it gives the first logits -- and
    `end(session, keys, ids)` records the context's keys plus ("t", id) for ids[:-1]: the last pick of a turn has no KV, and a slot
    row goes idle the moment its turn ends, so no id the host does not know is ever fed (DecodeSession's ("x",) case does not
    arise).  Between `begin` and `end` the session's keys are dropped: a turn that fails or is abandoned midway leaves a cache
    nobody trusts.

    `sync(stamp)` is called with what the cached rows depend on -- (the caller's weights_version, _decode_weights_id, the merge
    id of a merged qkv copy) -- before the turns of a call: whenever it moves, every session's keys are dropped, with
    DecodeSession's reasons ("weights changed" / "decode weights changed").  `clear()` drops them all ("empty cache"): the
    caches were overwritten.  `reason` is None when the cached rows were usable, whatever `past` came out."""

    def __init__(self, slots: int):
        if slots < 1:
            raise ValueError(f"slots must be >= 1, got {slots}")
        self.slots = int(slots)
        self.stamp = None
        self._open = {}                                              # key -> [session, slot, keys, why the keys are empty]

    @staticmethod
    def _key(session):
        try:
            hash(session)
            return ("v", session)
        except TypeError:
            return ("id", id(session))                               # the entry holds the object, so the id stays its own

    def __len__(self) -> int:
        return len(self._open)

    def __contains__(self, session) -> bool:
        return self._key(session) in self._open

    def slot_of(self, session) -> int:
        return self._open[self._key(session)][1]

    def keys_of(self, session) -> list:
        return list(self._open[self._key(session)][2])

    def open(self, session) -> int:
        """The session's slot; a new session takes the lowest free one."""
        k = self._key(session)
        if k not in self._open:
            used = {e[1] for e in self._open.values()}
            if len(used) >= self.slots:
                raise ValueError(f"all {self.slots} slots hold an open session: close() one before opening another")
            self._open[k] = [session, min(set(range(self.slots)) - used), [], "empty cache"]
        return self._open[k][1]

    def close(self, session) -> None:
        self._open.pop(self._key(session), None)

    def drop(self, session, reason: str = "empty cache") -> None:
        e = self._open.get(self._key(session))
        if e is not None:
            e[2], e[3] = [], reason

    def clear(self, reason: str = "empty cache") -> None:
        for e in self._open.values():
            e[2], e[3] = [], reason

    def sync(self, stamp) -> None:
        if self.stamp is not None and stamp != self.stamp:
            self.clear("weights changed" if stamp[0] != self.stamp[0] else "decode weights changed")
        self.stamp = stamp

    def begin(self, session, keys, reset_reason: Optional[str] = None):
        slot = self.open(session)
        e = self._open[self._key(session)]
        if len(keys) < 1:
            raise ValueError("a turn needs at least one context position")
        reason = reset_reason if reset_reason is not None else (None if e[2] else e[3])
        cached = [] if reason is not None else e[2]
        past = min(common_prefix(keys, cached), len(keys) - 1)
        e[2], e[3] = [], "empty cache"                               # until end(): the slot is being written
        return slot, past, reason

    def end(self, session, keys, ids) -> None:
        e = self._open.get(self._key(session))
        if e is not None:
            e[2], e[3] = list(keys) + [("t", int(t)) for t in list(ids)[:-1]], None

    def plan(self, turns, stamp):
        """One run_turns call: `turns` = [(session, keys) or (session, keys, reset_reason)], at most one per session.  Syncs
        the stamp and begins every turn; returns [(slot, past, reason)] in the turns' order."""
        seen = set()
        for t in turns:
            k = self._key(t[0])
            if k in seen:
                raise ValueError("at most one turn per session in one call")
            seen.add(k)
        new = [k for k in seen if k not in self._open]
        if len(self._open) + len(new) > self.slots:
            raise ValueError(f"{len(self._open)} open sessions + {len(new)} new ones do not fit {self.slots} slots: close() some")
        self.sync(stamp)
        return [self.begin(t[0], t[1], t[2] if len(t) > 2 else None) for t in turns]


def seeded_requests(requests, generator: Optional[torch.Generator] = None, seeds=None):
    """Pairs every request with the seed of its own random stream: yields (request, seed) in input order.  The seed is drawn when
    the request is taken from the input -- torch.randint(0, 2**63 - 1, (1,), generator=generator), the draw greedy_generate makes
    once per call -- so request i gets the i-th draw however RefillPlanner groups or holds back the refills; `seeds` (an iterable
    of ints in [0, 2**63), one per request in input order) replaces the draws and leaves `generator` untouched.  No device in
    sight, like SlotScheduler and RefillPlanner."""
    given = None if seeds is None else iter(seeds)
    for req in requests:
        if given is None:
            seed = int(torch.randint(0, 2**63 - 1, (1,), generator=generator))
        else:
            seed = next(given, None)
            if seed is None:
                raise ValueError("seeds: fewer seeds than requests")
            seed = int(seed)
            if not 0 <= seed < 2**63:
                raise ValueError(f"seeds: {seed} is outside [0, 2**63)")
        yield req, seed


def _request_generator(seed: int, t: int) -> torch.Generator:
    """The host generator for token t of the request with `seed`: the rare row the device sampler hands back (kept = -1) is drawn
    from it, never from the run's shared generator, so it cannot shift another request's stream."""
    g = torch.Generator()
    g.manual_seed((int(seed) * 0x9E3779B1 + int(t)) % 2**63)
    return g


def replay_slot_run(lengths, ids, slots: int, max_new_tokens: int, stop_ids=(), eos_id: int = 2, prefill_batch: int = 1,
                    prefill_rows: int = 2048, refill_min: int = 1) -> dict:
    """The counters of a slot run whose picks are known: request i has a prompt of lengths[i] rows and generates ids[i] (which must
    end where the stop rule ends it).  SlotScheduler + RefillPlanner driven as SlotDecoder.run drives them, without a device."""
    sched = SlotScheduler(slots, max_new_tokens, stop_ids, eos_id)
    plan = RefillPlanner(sched, range(len(lengths)), prefill_batch, prefill_rows, refill_min, length=lambda i: lengths[i])
    owner, prefills = [None] * slots, 0
    while True:
        group = plan.next_pass()
        while group:
            for s, i in group:
                prefills += 1
                if sched.admit(s, ids[i][0], 0.0):
                    owner[s] = [i, 1]
            group = plan.next_pass()
        live = sched.live()
        if not live:
            break
        picks = [0] * slots
        for s in live:
            picks[s] = ids[owner[s][0]][owner[s][1]]
            owner[s][1] += 1
        sched.step(picks, [0.0] * slots)
    return dict(prefills=prefills, prefill_passes=plan.passes, packed_rows=plan.packed_rows, steps=sched.steps,
                live_row_steps=sched.live_row_steps, occupancy=sched.occupancy)


class SlotDecoder:
    """Streams requests through `slots` rows of ONE captured token step (LlamaHIP.slot_decoder).  Each slot holds one request with
    its own prompt length, position and stop rule; a slot whose request ends is refilled with the next one while the others go on
    decoding, so no row is computed and thrown away for long and no request is cut short by another's stop.

    1 to GEMV_WIDE_MAX_ROWS slots.  Above GEMV_MAX_ROWS slots the products are ops.gemv_packed_wide on the same packed copies, whose
    rows carry the 16-row kernel's bits: a request's ids and margins do not depend on the slot count.
    The step is greedy_generate's fused packed step (bf16 / FP8 / MXFP4 copies, merged or bordered LoRA alike) with two launches
    swapped: the attention is mh_attn_decode_rope_rows (row b appends at pos[b], idle rows skipped) and the bookkeeping is
    mh_decode_advance_rows (idle rows record id -1).  `split_kv` (opt-in) swaps the attention for the split-KV kernel's rows
    form, mh_attn_decode_rope_split_rows -- the solo chat session's kernel for long contexts, a live row has its bits: False
    (default) never, True always, None by split_kv_rows_rule once per run / run_turns call.  Each kernel has its own views and
    captured graphs, so toggling evicts nothing.  A refill is the existing B = 1 prefill into the slot's slice of every cache.
    Between two replays the host writes only a finished slot's live flag, a refilled slot's (id, pos, kvlen, live) and a host
    draw's id.  greedy_generate and its row-0 rule are untouched; this path is opt-in.

    Device sampling, repetition_penalty != 1 and min_length > 1 run the step's per-row tail instead: mh_repetition_penalty_rows_slots
    (with a penalty), mh_sample_rows_slots or -- greedy and host draw -- mh_argmax_pmax_rows_slots, then mh_decode_advance_kept_rows.
    Slot row r then also has gen[r] on the device, the count of tokens its request has generated, which decides its EOS ban
    (gen[r] < min_length) and, with device sampling, is the Philox step of its draw from its own seed[r]: every request draws from
    its own counter-based stream (seeded_requests), so its answer does not depend on its neighbours, the slot count or the refill
    settings.  The knobs (temperature, top_p, top_k, penalty, min_length, eos_id) are read from device memory: one graph per
    (device-sampled or not, penalty or not).  A refill there also writes the slot's seed and gen = 1 and clears its bitmap row.

    Packed prefill (opt-in, `run(prefill_batch=P > 1)` or `refill_min > 1`): at a refill point up to min(P, free slots) waiting
    requests are prefilled in ONE pass over the weights (LlamaHIP._prefill_packed, one mh_attn_prefill_ragged per layer writing
    each request's keys / values into its own slot), one arg-max launch and one device->host copy give all their first picks, and
    they are admitted in input order.  RefillPlanner decides which requests go together and when.

    Conversations (opt-in, `run_turns`; the chat pool's, myriad_amd/chat.py ChatPool): a session keeps ITS slot and the rows the
    slot caches from call to call (`sessions`, a SessionTable), a turn prefills only the rows past the prefix its new context
    shares with them -- solo with `past`, or several turns per pass through _prefill_packed(..., pasts), one
    mh_attn_prefill_ragged_past per layer -- and then decodes in the same captured step as `run`.  `run` itself starts every slot
    at row 0, so it drops what the sessions had cached."""

    def __init__(self, llama: "LlamaHIP", slots: int, capacity: int, split_kv: Optional[bool] = False):
        slots = int(slots)
        if slots < 1 or slots > ops.GEMV_WIDE_MAX_ROWS:
            raise ValueError(f"slots={slots}: the slot engine runs the packed token step, 1 to {ops.GEMV_WIDE_MAX_ROWS} rows")
        if split_kv is not None and not isinstance(split_kv, bool):
            raise ValueError(f"split_kv={split_kv!r}: False (the single-workgroup rows kernel), True (split-KV) or None (the rule)")
        self.split_kv = split_kv
        self.llama, self.slots = llama, slots
        self.T_cap = ops.round_up(int(capacity), 64)
        if not 0 < self.T_cap <= 8192:
            raise ValueError(f"capacity={capacity}: a slot holds at most 8192 positions")
        self.bufs = None                                             # the step's buffers, shared by every view
        self.views = {}                                              # inv_temp -> workspace view of bufs with its own graph
        self.ws = None                                               # the view of the current / last run
        self._weights = None
        self.graph_captures = 0
        self.last_stats = {}
        self.sessions = SessionTable(slots)                          # run_turns: which conversation each slot's cache holds

    def close(self, session) -> None:
        """Free the slot of a run_turns session."""
        self.sessions.close(session)

    @staticmethod
    def _view_key(inv_temp: float, rows_tail=None, split: bool = False):
        """The key of a view (one captured graph each).  Without split-KV it is what it was before the engine had the choice --
        inv_temp, or (inv_temp or None, device-sampled, penalty) for the per-row tail -- and a split view is ("split", that)."""
        key = float(inv_temp)
        if rows_tail is not None:
            key = (None if rows_tail[0] else key, bool(rows_tail[0]), bool(rows_tail[1]))
        return ("split", key) if split else key

    def _workspace(self, inv_temp: float, rows_tail=None, split: bool = False) -> dict:
        """The step's buffers, kept while the decode weights stay the ones the captured graphs read, and over them one view (its
        own graph / warm flag) per inv_temp: the arg-max kernel takes inv_temp as a launch argument, so a captured step is fixed
        to one value (LlamaHIP._decode_workspace keys its workspaces the same way).  `rows_tail` = (device-sampled, penalty) asks
        for the step with the per-row tail: its buffers join on first use (the knobs `prm`, per-slot `seed` / `gen` / `kept` /
        `seen`, and `seed0` / `gen0` for the refills' first picks), and a device-sampled view is keyed without inv_temp, which the
        sampler reads from `prm`.  `split`: the view's step runs the split-KV rows kernel; the partials buffer joins on first use,
        a split view holds it and a non-split view holds None, so each (key, split) has its own graph."""
        L = self.llama
        L._prepare_decode_weights(self.slots, wide=True)
        if not (_packed_step(L, self.slots, True) and L.decode_fused):
            raise ValueError("the slot engine needs the fused packed token step (MYRIAD_PACK_DECODE and MYRIAD_DECODE_FUSED on)")
        wid = _decode_weights_id(L)
        if self.bufs is None or self._weights != wid:
            self.bufs, self.views, self.ws = None, {}, None
            self.bufs = _decode_buffers(L, self.slots, self.T_cap)
            self.bufs["live"] = torch.zeros((self.slots,), dtype=torch.int32, device=L.dev)
            self.bufs["wide"] = True                                 # above GEMV_MAX_ROWS slots the step stays on the packed copies
            self._weights = wid
        key = self._view_key(inv_temp, rows_tail, split)
        if split and self.bufs["split"] is None:
            self.bufs["split"] = ops.attn_decode_split_ws(self.slots, L.H, self.T_cap, L.dev)
        if rows_tail is not None:
            if "prm" not in self.bufs:
                n, i32 = self.slots, torch.int32
                self.bufs.update(prm=torch.zeros((6,), dtype=F32, device=L.dev), seed=torch.zeros((n,), dtype=torch.long, device=L.dev),
                                 seed0=torch.zeros((n,), dtype=torch.long, device=L.dev), gen=torch.zeros((n,), dtype=i32, device=L.dev),
                                 gen0=torch.zeros((n,), dtype=i32, device=L.dev), kept=torch.zeros((n,), dtype=i32, device=L.dev),
                                 seen=torch.zeros((n, (L.V + 31) // 32), dtype=i32, device=L.dev))
        if key not in self.views:
            same = [k for k in self.views if (isinstance(k, tuple) and k[0] == "split") == bool(split)]
            if len(same) >= 4:                                       # a few temperatures at most per kernel: drop its oldest graph
                self.views.pop(same[0])
            self.views[key] = dict(self.bufs, graph=None, warm=False, split=self.bufs["split"] if split else None)
        self.ws = self.views[key]
        return self.ws

    @torch.no_grad()
    def run(self, requests, max_new_tokens: int = 90, stop_ids=((835,), (2277, 29937)), eos_id: int = 2, min_length: int = 1,
            do_sample: bool = False, top_p: float = 1.0, temperature: float = 1.0, top_k: int = 50,
            generator: Optional[torch.Generator] = None, ordered: bool = False, prefill_batch: int = 1, refill_min: int = 1,
            prefill_rows: int = 2048, repetition_penalty: float = 1.0, seeds=None):
        """Decode every request of `requests` (an iterable of [S0_i, D] f32 embeddings, lengths free) and yield
        (index, ids[L_i] int64 on the CPU, margins[L_i] f32) as each finishes -- or, with `ordered`, in input order.  The
        arguments are greedy_generate's; the stop rule is per request.  `last_stats` holds the run's counters: `prefills` counts
        requests, `prefill_passes` passes over the weights and `packed_rows` the request rows they held (padding not counted).
        `prefill_batch`, `refill_min`, `prefill_rows`: RefillPlanner's; at 1, 1 every refill is the one-request prefill.

        With `device_sampling` (and greedy_generate's conditions on top_k and the vocabulary) every pick is drawn on the device
        from the request's own stream: request i takes the i-th seed drawn from `generator`, or the i-th of `seeds`, and token t
        of it is Philox step t -- what greedy_generate draws for that request alone with that seed.  `device_sampled_rows`
        counts those picks; a row the sampler hands back (kept = -1) is drawn on the host from a generator derived from the
        request's seed and t (`host_sampled_rows`).  `repetition_penalty` != 1 needs the switch, as in generate(); `min_length`
        is a per-request EOS ban on every path.  A second run with other values of the knobs replays the same graph.
        `last_stats["split_kv"]`: the attention kernel of the call's token steps.  With the decoder's split_kv=None the rule sees
        `slots` live rows and a longest context of 0 -- the lengths are not known up front -- so None never splits here."""
        self.sessions.clear()                                        # the slots' caches are overwritten from row 0
        yield from self._run(requests, None, None, max_new_tokens, stop_ids, eos_id, min_length, do_sample, top_p, temperature,
                             top_k, generator, ordered, prefill_batch, refill_min, prefill_rows, repetition_penalty, seeds)

    def run_turns(self, turns, weights_version=None, **kw):
        """One turn each of several conversations, every one in ITS OWN slot on top of what that slot's cache holds of it
        (`sessions`, a SessionTable).  `turns` = [(session, emb [S0, D] f32, keys [S0])] or with a fourth item `reset_reason`; at
        most one turn per session per call (ValueError), at most `slots` open sessions (`close(session)` frees one).  `kw` are
        `run`'s arguments but `refill_min` (prefill_batch, prefill_rows, the sampling knobs, repetition_penalty, min_length,
        seeds: with device sampling the i-th turn of the call takes the i-th seed).  Only the rows past the prefix the slot
        shares with the new context are prefilled: with prefill_batch = 1 a solo _prefill(emb, slot cache, past) per turn,
        otherwise passes of up to prefill_batch turns / prefill_rows new rows through _prefill_packed(..., pasts).  Then `run`'s
        captured step (same graphs and views) runs until every turn has stopped under its own stop rule.  Yields (session, ids,
        margins) as `run` does, `ordered=True` in the list's order; `last_stats["turns"]` holds per turn `context_tokens`,
        `reused_tokens`, `prefilled_tokens` and `full_reprefill_reason`.  `weights_version`: anything that changes when the
        weights do; with it, a change of the decode weights or a `run()` on this decoder drops every session's cached rows.  The
        step's attention kernel is the decoder's `split_kv` choice, made once per call (`last_stats["split_kv"]`): with None,
        split_kv_rows_rule(turns in the call, heads, the longest context at admission)."""
        turns = [tuple(t) for t in turns]
        if "refill_min" in kw:
            raise ValueError("run_turns: refill_min does not apply, every turn has its own slot")
        for t in turns:
            if len(t) not in (3, 4) or t[1].dim() != 2 or len(t[2]) != t[1].shape[0]:
                raise ValueError("run_turns: a turn is (session, emb [S0, D], keys [S0]) or (session, emb, keys, reset_reason)")
        keys = [SessionTable._key(t[0]) for t in turns]
        if len(set(keys)) != len(keys):
            raise ValueError("run_turns: at most one turn per session in one call")
        return self._run(None, turns, weights_version, **kw)

    @torch.no_grad()
    def _run(self, requests, turns, weights_version, max_new_tokens: int = 90, stop_ids=((835,), (2277, 29937)), eos_id: int = 2,
             min_length: int = 1, do_sample: bool = False, top_p: float = 1.0, temperature: float = 1.0, top_k: int = 50,
             generator: Optional[torch.Generator] = None, ordered: bool = False, prefill_batch: int = 1, refill_min: int = 1,
             prefill_rows: int = 2048, repetition_penalty: float = 1.0, seeds=None):
        """`run` (requests) and `run_turns` (turns + weights_version): one engine, two admission rules."""
        L = self.llama
        if do_sample and not float(temperature) > 0:
            raise ValueError(f"temperature must be > 0 when sampling, got {temperature}")
        if not float(repetition_penalty) > 0:
            raise ValueError(f"repetition_penalty must be > 0, got {repetition_penalty}")
        penalty = float(repetition_penalty) != 1.0
        if penalty and not L.device_sampling:
            raise NotImplementedError(f"decode slots: repetition_penalty={repetition_penalty} needs the device sampling switch "
                                      "(MYRIAD_DEVICE_SAMPLING=1 or llama.device_sampling = True)")
        inv_temp = 1.0 / float(temperature) if do_sample else 1.0
        top_k = 0 if top_k is None else int(top_k)
        dev_sample = bool(L.device_sampling and do_sample and 1 <= top_k <= ops.SAMPLE_CAP and L.V <= 32768 and L.V % 4 == 0)
        if seeds is not None and not dev_sample:
            raise ValueError("seeds= names the device sampler's per-request streams: it needs do_sample with device_sampling on")
        rows_tail = dev_sample or penalty or min_length > 1          # else exactly the launches of the plain slot step
        # the attention kernel of every token step of this call, chosen once: `run` does not know its lengths up front
        if self.split_kv is None:
            split = split_kv_rows_rule(self.slots, L.H, 0) if turns is None else \
                split_kv_rows_rule(len(turns), L.H, max([int(t[1].shape[0]) for t in turns], default=0))
        else:
            split = self.split_kv
        ws = self._workspace(inv_temp, (dev_sample, penalty) if rows_tail else None, split)
        sched = SlotScheduler(self.slots, max_new_tokens, stop_ids, eos_id, ordered=ordered)
        stats = dict(steps=0, graph_replays=0, graph_captures=self.graph_captures, prefills=0, live_row_steps=0, occupancy=0.0,
                     host_sampled_rows=0, device_sampled_rows=0, prefill_passes=0, packed_rows=0, split_kv=bool(split))
        packed = int(prefill_batch) != 1 or int(refill_min) != 1
        # a request travels with the seed of its own stream (None unless the device draws)
        if turns is None:
            reqs = seeded_requests(requests, generator, seeds) if dev_sample else ((emb, None) for emb in requests)
            plan = RefillPlanner(sched, reqs, prefill_batch, prefill_rows, refill_min, length=lambda q: int(q[0].shape[0]))
        else:
            # the stamp of DecodeSession: no cached row survives a change of the weights the step multiplies by
            P = L._packed
            stamp = (weights_version, _decode_weights_id(L), P["merge_id"] if P["qkv_key"] == "merged" else None)
            begun = self.sessions.plan([(t[0], list(t[2])) + t[3:] for t in turns], stamp)
            seeds_ = [sd for _, sd in seeded_requests(turns, generator, seeds)] if dev_sample else [None] * len(turns)
            # a turn travels as (emb, seed, past) and is admitted in list order: its index is its place in `turns`
            plan = TurnPlanner([(slot, (t[1], sd, past)) for t, sd, (slot, past, _) in zip(turns, seeds_, begun)], prefill_batch,
                               prefill_rows, length=lambda q: int(q[0].shape[0]) - q[2])
            stats["turns"] = [dict(context_tokens=int(t[1].shape[0]), reused_tokens=past, prefilled_tokens=int(t[1].shape[0]) - past,
                                   full_reprefill_reason=reason) for t, (_, past, reason) in zip(turns, begun)]
        self.last_stats = stats
        ban0 = eos_id if 0 < min_length else -1
        rec = ws["rec"] if rows_tail else ws["rec"][:3]
        seed_of = {}                                                 # slot -> its request's seed
        ws["live"].zero_()                                           # an abandoned run may have left slots live
        ws["step"].zero_()
        if rows_tail:
            ws["prm"].copy_(torch.tensor([inv_temp, top_p, float(top_k), float(repetition_penalty), float(min_length), float(eos_id)],
                                         dtype=F32))

        def token_step(_ban):
            L._step_logits(ws)
            if not rows_tail:
                ops.argmax_pmax_rows(ws["logits"], ws["nxt"], ws["mar"], ws["pmx"], ban_id=-1, inv_temp=inv_temp)
                ops.decode_advance_rows(ws["nxt"], ws["mar"], ws["pmx"], rec, ws["ids"], ws["step"], ws["pos"], ws["kvlen"],
                                        ws["live"])
                return
            if penalty:                                              # ws["ids"] = the token fed in: it joins the seen set first
                ops.repetition_penalty_rows_slots(ws["logits"], ws["seen"], ws["ids"], ws["prm"][3:], ws["live"])
            if dev_sample:                                           # row r draws Philox step gen[r] of seed[r]
                ops.sample_rows_slots(ws["logits"], ws["nxt"], ws["mar"], ws["pmx"], ws["kept"], ws["prm"], ws["seed"], ws["gen"],
                                      ws["live"])
            else:
                ops.argmax_pmax_rows_slots(ws["logits"], ws["nxt"], ws["mar"], ws["pmx"], ws["prm"], ws["gen"], ws["live"])
            ops.decode_advance_kept_rows(ws["nxt"], ws["mar"], ws["pmx"], ws["kept"] if dev_sample else None, rec, ws["ids"],
                                         ws["step"], ws["pos"], ws["kvlen"], ws["gen"], ws["live"])

        def results():
            for index, ids, mar in sched.pop():
                if turns is not None:                                # the slot now holds the context and every id but the last
                    self.sessions.end(turns[index][0], turns[index][2], ids)
                    index = turns[index][0]
                yield index, torch.tensor(ids, dtype=torch.long), torch.tensor(mar, dtype=F32)

        def fits(emb: torch.Tensor) -> int:
            S0 = emb.shape[0] if emb.dim() == 2 else 0
            if S0 < 1 or S0 + max_new_tokens > min(self.T_cap, L.cos.shape[0]):
                raise ValueError(f"request of shape {tuple(emb.shape)} + max_new_tokens {max_new_tokens} does not fit a slot of "
                                 f"{min(self.T_cap, L.cos.shape[0])} positions")
            return S0

        def go_live(s: int, first: int, S0: int, seed) -> None:
            sl = slice(s, s + 1)
            ws["ids"][sl].fill_(first)
            ws["pos"][sl].fill_(S0)                                  # position of the incoming token
            ws["kvlen"][sl].fill_(S0 + 1)                            # valid keys after the append
            if rows_tail:
                ws["gen"][sl].fill_(1)                               # the prefill pick was token 0
                if dev_sample:
                    ws["seed"][sl].fill_(seed)
                    seed_of[s] = seed
                if penalty:
                    ws["seen"][sl].zero_()                           # generated ids only, and the last request's are gone
            ws["live"][sl].fill_(1)

        def first_picks(logits0: torch.Tensor, sl: slice, seeds_) -> list:
            """The first pick of each prefilled request (rows of logits0) in one launch into the step's result buffers at `sl` and
            one device->host copy: rows of [id, margin, p_max, kept].  The per-row tail's pick is its step kernel at gen = 0."""
            out = [ws["nxt"][sl], ws["mar"][sl], ws["pmx"][sl]]
            R = logits0.shape[0]
            if dev_sample:
                ws["seed0"][:R].copy_(torch.tensor(seeds_, dtype=torch.long))
                ops.sample_rows_slots(logits0, *out, ws["kept"][sl], ws["prm"], ws["seed0"][:R], ws["gen0"][:R])
                out.append(ws["kept"][sl])
            elif rows_tail:
                ops.argmax_pmax_rows_slots(logits0, *out, ws["prm"], ws["gen0"][:R])
            else:
                ops.argmax_pmax_rows(logits0, *out, ban_id=ban0, inv_temp=inv_temp)
            return torch.stack([o.to(torch.float64) for o in out], 1).tolist()

        def first_id(pick, logits_row: torch.Tensor, seed) -> int:
            """The request's first token from its pick: the device's draw, or the host's where the rules hand the row to it."""
            first = int(pick[0])
            if dev_sample and pick[3] >= 0:
                stats["device_sampled_rows"] += 1
            elif dev_sample:
                first = _host_draw(logits_row, ban0, inv_temp, top_k, top_p, _request_generator(seed, 0))
                stats["host_sampled_rows"] += 1
            elif do_sample and pick[2] < top_p:
                first = _host_draw(logits_row, ban0, inv_temp, top_k, top_p, generator)
                stats["host_sampled_rows"] += 1
            return first

        def refill_packed(group) -> None:
            """Prefill the group's requests in one packed pass, each into its slot; one pick launch and one device->host copy
            for all first picks; admission in input order."""
            R, lens = len(group), [fits(req[0]) for _, req in group]
            pasts = None if turns is None else [req[2] for _, req in group]
            logits0 = L._prefill_packed([req[0] for _, req in group], [s for s, _ in group], ws["caches"], pasts)
            stats["prefills"] += R
            picks = first_picks(logits0, slice(0, R), [req[1] for _, req in group])
            for i, (s, req) in enumerate(group):
                seed = req[1]
                first = first_id(picks[i], logits0[i], seed)
                if sched.admit(s, first, picks[i][1]):
                    go_live(s, first, lens[i], seed)

        def refill(s: int, req) -> None:
            """Prefill one request alone into slot s and take its first pick; the slot goes live if the request goes on."""
            emb, seed = req[0], req[1]
            S0 = fits(emb)
            logits0 = L._prefill(emb[None].to(L.dev), [c[s:s + 1] for c in ws["caches"]], req[2] if turns is not None else 0)
            stats["prefills"] += 1
            pick = first_picks(logits0, slice(s, s + 1), [seed])[0]
            first = first_id(pick, logits0[0], seed)
            if sched.admit(s, first, pick[1]):
                go_live(s, first, S0, seed)

        try:
            while True:
                group = plan.next_pass()
                while group:
                    if packed:
                        refill_packed(group)
                    else:
                        refill(*group[0])
                    group = plan.next_pass()
                yield from results()
                live = sched.live()
                if not live:
                    break
                before = ws["graph"]
                L._launch_step(ws, token_step, -1, True, stats)
                if ws["graph"] is not before:
                    self.graph_captures += 1
                r = rec.cpu()                                        # the one device->host copy of the step (it also waits for it)
                ids = r[0].long().tolist()
                if dev_sample:
                    for s in live:
                        if float(r[3][s]) >= 0:
                            stats["device_sampled_rows"] += 1        # drawn by the step itself
                            continue
                        t = len(sched.rows[s][1])                    # the row's gen when the step ran
                        ids[s] = _host_draw(ws["logits"][s], eos_id if t < min_length else -1, inv_temp, top_k, top_p,
                                            _request_generator(seed_of[s], t))
                        stats["host_sampled_rows"] += 1
                elif do_sample:
                    for s in live:
                        if float(r[2][s]) < top_p:                   # greedy_generate's rule per row: below top_p the host draws
                            ban = eos_id if len(sched.rows[s][1]) < min_length else -1
                            ids[s] = _host_draw(ws["logits"][s], ban, inv_temp, top_k, top_p, generator)
                            stats["host_sampled_rows"] += 1
                finished = sched.step(ids, r[1].tolist())
                for s in live:
                    if s in finished:
                        ws["live"][s:s + 1].zero_()
                    elif ids[s] != int(r[0][s]):
                        ws["ids"][s:s + 1].fill_(ids[s])             # a host draw replaces the arg-max the step fed back
                yield from results()
        finally:
            stats.update(steps=sched.steps, live_row_steps=sched.live_row_steps, occupancy=sched.occupancy,
                         graph_captures=self.graph_captures, prefill_passes=plan.passes, packed_rows=plan.packed_rows)
