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

import torch

from . import _lib, ops
from .decode import DecodeSession, LlamaDecode, SlotDecoder, _decode_buffers, _packed_step  # noqa: F401  (re-exported)
from .decode_host import (SPLIT_KV_MAX_ROWHEADS, SPLIT_KV_MIN_KEYS, SPLIT_KV_ROWS_MAX_ROWHEADS,  # noqa: F401  (re-exported)
                          SPLIT_KV_ROWS_MIN_KEYS, RefillPlanner, SessionTable, SlotScheduler, TurnPlanner, common_prefix,
                          replay_slot_run, seeded_requests, split_kv_rows_rule, split_kv_rule)

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


class LlamaHIP(LlamaDecode):
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
        # num_beams > 1 with do_sample (HF's beam-search multinomial sampling) or a repetition penalty: the beam step selects with
        # mh_beam_sample_topk and carries the seen-id bitmaps (mh_beam_seen_update); off, generate() refuses both as before
        self.beam_sampling = os.environ.get("MYRIAD_BEAM_SAMPLING", "0") != "0"
        # beam search in the decode slots, one request per group of num_beams rows (SlotDecoder.run(num_beams > 1)); off by default.
        # With beam_sampling on as well the groups take do_sample and the penalty (mh_beam_sample_topk_items)
        self.slot_beams = os.environ.get("MYRIAD_SLOT_BEAMS", "0") != "0"
        # draft-and-verify decoding in the decode slots (SlotDecoder.run(draft=...), generate_stream(draft=...), eval_aqa.py --slots
        # N --draft-k K); off by default: those entries refuse `draft` as before
        self.slot_draft = os.environ.get("MYRIAD_SLOT_DRAFT", "0") != "0"
        # draft decoding under device sampling, the repetition penalty, min_length and the token scores (off by default)
        self.draft_sampling = os.environ.get("MYRIAD_DRAFT_SAMPLING", "0") != "0"
        # draft decoding on the split-KV view (mh_attn_decode_rope_split_draft: the chat session's long turns, a decoder built with
        # split_kv) and in SlotDecoder.run_turns / ChatPool; off by default: the split view decodes with plain steps and run_turns
        # refuses `draft` as before
        self.draft_split = os.environ.get("MYRIAD_DRAFT_SPLIT", "0") != "0"
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

    def _prepare_decode_weights(self, rows: int, row_limit: int = ops.GEMV_MAX_ROWS) -> dict:
        """Before a decode call at `rows` rows: the LoRA's bordered weights refreshed, the packed copies (re)built when the step
        can stream them (MYRIAD_PACK_DECODE=0 drops them: the step streams the row-major matrices).  Returns last_generate_stats'
        decode_weights ("fp8" / "fp4" / "bf16": what the token step streams) and decode_weight_bytes (the weight bytes of one token
        step: the packed copies, fp8 row scales / fp4 scale bytes included, up to `row_limit` rows -- GEMV_MAX_ROWS, or
        GEMV_WIDE_MAX_ROWS in the slot engine's call; the row-major bf16 matrices above), lora_merged (the
        step streams the LoRA-merged qkv copy) and lora_merges (whole-model merges this model has made so far)."""
        self._decode_kind()                                             # both kinds on: an error whatever this call streams
        if self.lora is not None:
            self.lora.refresh(self.layers)
        if self.pack_decode and rows <= row_limit:
            self._pack_for_decode()                                     # GEMV_WIDE_MAX_ROWS: the slot engine's route to the copies above 16 rows
        elif not self.pack_decode:
            self._packed, self._packs = None, {}
        if _packed_step(self, rows, row_limit):
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

    def embed_tokens_into(self, ids: torch.Tensor, out2d: torch.Tensor, dst_rows: Optional[torch.Tensor] = None):
        ops.embed_gather(self.embed, ids, out2d, dst_rows)

