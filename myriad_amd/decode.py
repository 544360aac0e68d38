"""KV-cache decode on the HIP kernels: the prefills and the single-token step of the LLaMA decoder, the greedy and beam loops
(LlamaDecode, the mixin LlamaHIP inherits), the multi-turn chat's DecodeSession and the decode-slot engine SlotDecoder.  The
weights, their packed decode copies and the training path are myriad_amd/llama.py's; what never sees a device is
myriad_amd/decode_host.py's."""
from __future__ import annotations

import gc
import math
from typing import List, Optional

import numpy as np
import torch

from . import ops
from .decode_host import (BeamItem, BeamSlotScheduler, DraftLoop, RefillPlanner, ScorePlan, SessionTable, SlotScheduler, TurnPlanner, _host_draw,
                          _request_generator, beam_batch_going, beam_sample_select, common_prefix, run_draft_loop, f32_at_least, seeded_requests,
                          slot_guesses, split_kv_rows_rule, split_kv_rule)

BF16, F32 = torch.bfloat16, torch.float32


# Decode helpers shared by LlamaHIP and DecodeSession.  They read only the model's fields, so the session needs no more of the
# model than those.
def _packed_step(lm: "LlamaHIP", rows: int, row_limit: int = ops.GEMV_MAX_ROWS) -> bool:
    """The token step at `rows` rows streams the packed copies.  `row_limit` is the caller's: GEMV_MAX_ROWS (what ops.gemv_packed
    takes) for every decode loop, so their routing above it is the row-major GEMM; GEMV_WIDE_MAX_ROWS for the slot engine, which
    stays on the copies up to there (ops.gemv_packed_wide)."""
    return lm._packed is not None and rows <= row_limit


def _wide_step(lm: "LlamaHIP", rows: int, row_limit: int) -> bool:
    """The packed token step above GEMV_MAX_ROWS rows (the slot engine's, whose row limit lets it be): the fused step's launch
    sequence with ops.gemv_packed_wide as the product and the two-launch forms of the norm / SiLU products, as at 3 to 16 rows."""
    return _packed_step(lm, rows, row_limit) and rows > ops.GEMV_MAX_ROWS


def _decode_weights_id(lm: "LlamaHIP") -> tuple:
    """What the token step multiplies by: the packed copies (which object, its kind, which qkv copy is live), the fused
    launches and the LoRA.  The workspace key holds it, so no graph captured on one set of weights is replayed on another."""
    P = lm._packed
    return id(P), None if P is None else (P["kind"], P["qkv_key"]), lm.decode_fused, lm.lora is not None


def _decode_buffers(lm: "LlamaHIP", B: int, T_cap: int, sampler: bool = False, num_beams: int = 1,
                    row_limit: int = ops.GEMV_MAX_ROWS, scores: bool = False) -> dict:
    """Buffers of the single-token step at B rows: KV caches of T_cap positions, device-resident counters, id / logit /
    result buffers and the [4, B] per-step record (the arg-max step writes its first three rows); `graph` / `warm` hold the
    captured step once there is one (_launch_step), `split` the split-KV partials when the step uses them, `row_limit` the rows
    up to which the step stays on the packed copies (_packed_step).  With `sampler`
    the device sampler's and the repetition penalty's buffers join: their knobs (`prm` = inv_temp, top_p, top_k, penalty),
    the seed, the kept counts and the seen-id bitmaps.  With num_beams > 1, B counts rows (items x beams) and the beam step's
    buffers join (_beam_buffers, and `lo`, where the generated positions start).  With
    `scores` the record is the one with the token scores' rows behind its four (_score_buffers)."""
    dev, i32 = lm.dev, torch.int32
    # `ids` is the head of `ids_k`, which the K-row verify step of draft decoding reads whole: ids_k[0] is the fed token of both
    ids_k = torch.zeros((max(B, ops.DRAFT_MAX_K),), dtype=torch.long, device=dev)
    ws = dict(T=T_cap, graph=None, warm=False, split=None, row_limit=row_limit, ids_k=ids_k,
              caches=[torch.zeros((B, T_cap, 2 * lm.D), dtype=BF16, device=dev) for _ in lm.layers],
              pos=torch.zeros((B,), dtype=i32, device=dev), kvlen=torch.zeros((B,), dtype=i32, device=dev),
              ids=ids_k[:B], x_in=torch.empty((B, lm.D), dtype=F32, device=dev),
              logits=torch.empty((B, lm.V), dtype=F32, device=dev),
              nxt=torch.empty((B,), dtype=torch.long, device=dev), mar=torch.empty((B,), dtype=F32, device=dev),
              pmx=torch.empty((B,), dtype=F32, device=dev), step=torch.zeros((1,), dtype=i32, device=dev),
              rec=torch.zeros((4, B), dtype=F32, device=dev))
    if sampler:
        ws.update(prm=torch.zeros((4,), dtype=F32, device=dev), seed=torch.zeros((1,), dtype=torch.long, device=dev),
                  kept=torch.zeros((B,), dtype=i32, device=dev),
                  seen=torch.zeros((B, (lm.V + 31) // 32), dtype=i32, device=dev))
    if num_beams > 1:
        ws.update(_beam_buffers(lm, ws["caches"], B, int(num_beams)), lo=torch.zeros((1,), dtype=i32, device=dev))
    if scores:
        ws["rec"] = _score_buffers(lm, ws)["srec"]
    return ws


def _beam_buffers(lm: "LlamaHIP", caches, R: int, nb: int) -> dict:
    """The beam step's buffers for R rows in groups of nb: `bupd` = the per-step upload (ids int64 | parent rows int32 | running
    scores f32) with its pinned host twin and the views of it the captured step reads, the top-K scratch, the [2, G * K] record
    and the device table of the per-layer cache pointers that the KV reorder walks."""
    dev, i32, K = lm.dev, torch.int32, 2 * nb
    bupd = torch.zeros((4 * R,), dtype=i32, device=dev)
    return dict(bupd=bupd, bupd_host=torch.zeros((4 * R,), dtype=i32).pin_memory(),
                ids=bupd[:2 * R].view(torch.long), src=bupd[2 * R:3 * R], bscore=bupd[3 * R:].view(F32),
                part_s=torch.empty((R * K,), dtype=F32, device=dev), part_i=torch.empty((R * K,), dtype=i32, device=dev),
                brec=torch.zeros((2, R // nb * K), dtype=i32, device=dev),
                table=torch.tensor([c.data_ptr() for c in caches], dtype=torch.long).to(dev))


def _beam_upload(host: torch.Tensor):
    """The pinned upload's three parts as numpy views: (ids int64 [R], parent rows int32 [R], running scores f32 [R])."""
    R = host.shape[0] // 4
    return host[:2 * R].view(torch.long).numpy(), host[2 * R:3 * R].numpy(), host[3 * R:].view(F32).numpy()


def _beam_record(rec: torch.Tensor, G: int):
    """A [2, G * K] int32 record as (top_s [G, K] f32, top_i [G, K] int64): a beam step's one device->host copy (it waits for it)."""
    rec = rec.cpu()
    return rec[0].view(F32).numpy().reshape(G, -1), rec[1].numpy().reshape(G, -1).astype(np.int64)


def _beam_sample_record(rec: torch.Tensor, G: int, K: int):
    """A sampled beam step's (acc [G * K] f32 | flat [G * K] | overflow flag [G]) int32 record as (top_s [G, K] f32, top_i [G, K]
    int64, flags [G]): the step's one device->host copy (it waits for it).  top_s is a copy: a host redo writes into it."""
    rec = rec.cpu()
    return (rec[:G * K].view(F32).numpy().reshape(G, K).copy(), rec[G * K:2 * G * K].numpy().reshape(G, K).astype(np.int64),
            rec[2 * G * K:2 * G * K + G].numpy())


def _pad_ids(seqs, pad: int) -> torch.Tensor:
    """Id tuples right-padded with `pad` to a [n, max(1, Lmax)] int64 tensor."""
    ids = torch.full((len(seqs), max(1, max(len(q) for q in seqs))), pad, dtype=torch.long)
    for r, q in enumerate(seqs):
        ids[r, :len(q)] = torch.tensor(q, dtype=torch.long)
    return ids


def _beam_checks(nb: int, V: int) -> None:
    """The beam paths' checks of num_beams that need no request (BeamItem checks the rest of the search's arguments)."""
    if nb > ops.BEAM_MAX:
        raise NotImplementedError(f"num_beams={nb}: at most {ops.BEAM_MAX} beams on the HIP decode path")
    if nb < 1:
        raise ValueError(f"num_beams must be >= 1, got {nb}")
    if V < 2 * nb:
        raise ValueError(f"num_beams={nb} needs a vocabulary of at least {2 * nb} tokens")


def _score_buffers(lm: "LlamaHIP", bufs: dict) -> dict:
    """The token scores' buffers, joined to a buffer set on first use: `srec`, a step record of 4 + SCORE_ROWS rows whose last
    SCORE_ROWS mh_token_scores_rows writes (lse, the pick's log-prob, one row per watch slot), so a step with scores is still ONE
    device->host copy; `watch`, the watched ids on the device (-1: unused), which the kernel reads from memory."""
    if "srec" not in bufs:
        B = bufs["ids"].shape[0]
        bufs.update(srec=torch.zeros((4 + ops.SCORE_ROWS, B), dtype=F32, device=lm.dev),
                    watch=torch.full((ops.SCORE_WATCH_MAX,), -1, dtype=torch.int32, device=lm.dev))
    return bufs


def _cache_stamp(lm: "LlamaHIP", weights_version) -> tuple:
    """What cached KV rows depend on: the caller's weights version and the weights the step multiplies by.  The merged qkv copy is
    rewritten in place by a re-merge: its merge id joins the stamp, so no KV row survives a change of the weights the step
    multiplies by, whether or not the caller's weights_version saw it."""
    P = lm._packed
    return weights_version, _decode_weights_id(lm), P["merge_id"] if P is not None and P["qkv_key"] == "merged" else None


def _sampling_args(lm: "LlamaHIP", do_sample: bool = False, temperature: float = 1.0, top_k=50, repetition_penalty: float = 1.0,
                   **_others):
    """The decode loops' checks of their sampling arguments (greedy_generate's, with its defaults; its other arguments pass
    through unread) and what they derive from them: (inv_temp, top_k, dev_sample -- the device draws inside the token step --,
    penalty -- the repetition penalty is on)."""
    if do_sample and not float(temperature) > 0:
        raise ValueError(f"temperature must be > 0 when sampling, got {temperature}")
    if not float(repetition_penalty) > 0:
        raise ValueError(f"repetition_penalty must be > 0, got {repetition_penalty}")
    top_k = 0 if top_k is None else int(top_k)
    dev_sample = bool(do_sample and lm.device_sampling and 1 <= top_k <= ops.SAMPLE_CAP and lm.V <= 32768 and lm.V % 4 == 0)
    return 1.0 / float(temperature) if do_sample else 1.0, top_k, dev_sample, float(repetition_penalty) != 1.0


def _buffer_view(lm: "LlamaHIP", bufs: dict, split: bool, scores: bool = False) -> dict:
    """A workspace view of a buffer set: the buffers with a graph / warm flag of its own.  `split`: the view's step runs a split-KV
    attention kernel; the partials buffer joins the set on first use, a split view holds it and a non-split view holds None.
    `scores`: the view's step also writes the token scores; its record is the set's `srec` (_score_buffers)."""
    if split and bufs["split"] is None:
        bufs["split"] = ops.attn_decode_split_ws(bufs["ids"].shape[0], lm.H, bufs["T"], lm.dev)
    view = dict(bufs, graph=None, warm=False, split=bufs["split"] if split else None)
    if scores:
        view.update(rec=_score_buffers(lm, bufs)["srec"], watch=bufs["watch"])
    return view


def _draft_view(lm: "LlamaHIP", bufs: dict, K: int, inv_temp: float, tail=None, split: bool = False) -> dict:
    """The K-row verify step's view of a B = 1 buffer set (draft decoding): the caches, `pos`, `kvlen`, `step` and the fed token
    ids_k[0] are the set's, shared with its plain one-row step, so the host switches between the two from step to step; the K-row
    ids / activations / logits / picks, the 3K + 1 float record `drec`, the device float `top_p` and the always-live flag are the
    view's own, and so is its graph.  Kept in the set (one per K and inv_temp, which the arg-max launch bakes in).

    `tail` = (device-sampled, penalty, scores), behind `draft_sampling`: the view of the verify step that runs the decode slots'
    per-row tail at G = 1 (draft_sample.hip), keyed (K, inv_temp) + tail.  It adds `kept` [K], the one-group state `full` = [K]
    (nrow: every row holds a token, fillers included), `ngs` = [K - 1] and, in the set, the token counter `gen` [1]; its record
    `drec` is flat -- the 4K + 1 floats of mh_draft_accept_sampled_rows (`arec`), then with scores SCORE_ROWS rows of K (`sc`).
    With the device sampler the set also gains `prm6` (the slot form's six knobs) and `plain_rows`, the view of the call's plain
    step in the slot form: the solo step counts launches in `step`, the slot form tokens in `gen`, which both steps advance.

    `split` (behind `draft_split`, for a split-KV `bufs`): the view's attention is ops.attn_decode_rope_split_draft and it holds
    that launch's partials `split_draft`; keyed ("split",) + the above, beside the plain split step it switches with."""
    if bufs["ids"].shape[0] != 1:
        raise NotImplementedError("draft decoding runs one sequence (batch 1)")
    views = bufs.setdefault("draft_views", {})
    key = (("split",) if split else ()) + (int(K), float(inv_temp)) + (() if tail is None else tuple(bool(t) for t in tail))
    if tail is not None and "gen" not in bufs:
        bufs["gen"] = torch.zeros((1,), dtype=torch.int32, device=lm.dev)
    if tail is not None and tail[0] and "prm6" not in bufs:
        bufs["prm6"] = torch.zeros((6,), dtype=F32, device=lm.dev)
    if tail is not None and tail[0] and ("plain_rows", bool(tail[1]), bool(tail[2])) not in views:
        views["plain_rows", bool(tail[1]), bool(tail[2])] = dict(bufs, graph=None, warm=False,
                                                                 live1=torch.ones((1,), dtype=torch.int32, device=lm.dev))
    if key not in views:
        dev = lm.dev
        views[key] = dict(bufs, graph=None, warm=False, split=None, draft_k=int(K), ids=bufs["ids_k"][:K],
                          split_draft=ops.attn_decode_split_draft_ws(1, int(K), lm.H, bufs["T"], dev) if split else None,
                          x_in=torch.empty((K, lm.D), dtype=F32, device=dev), logits=torch.empty((K, lm.V), dtype=F32, device=dev),
                          nxt=torch.empty((K,), dtype=torch.long, device=dev), mar=torch.empty((K,), dtype=F32, device=dev),
                          pmx=torch.empty((K,), dtype=F32, device=dev), drec=torch.zeros((3 * K + 1,), dtype=F32, device=dev),
                          top_p=torch.zeros((1,), dtype=F32, device=dev), live1=torch.ones((1,), dtype=torch.int32, device=dev))
        if tail is not None:
            drec = torch.zeros((4 * K + 1 + (ops.SCORE_ROWS * K if tail[2] else 0),), dtype=F32, device=dev)
            views[key].update(kept=torch.zeros((K,), dtype=torch.int32, device=dev), drec=drec, arec=drec[:4 * K + 1],
                              sc=drec[4 * K + 1:].view(ops.SCORE_ROWS, K) if tail[2] else None,
                              full=torch.full((1,), K, dtype=torch.int32, device=dev),
                              ngs=torch.full((1,), K - 1, dtype=torch.int32, device=dev))
    return views[key]


def _draft_refusals(B: int, dev_sample: bool, penalty: bool, return_scores: bool, draft_k, tail: bool = False) -> int:
    """The arguments draft decoding does not take; returns K.  `tail`: the caller's `draft_sampling` switch, behind which the
    verify step runs the sampler, the penalty and the scores per row (_draft_core)."""
    K = int(draft_k)
    if not 1 <= K <= ops.DRAFT_MAX_K:
        raise ValueError(f"draft_k={draft_k}: 1 to {ops.DRAFT_MAX_K} rows per verify step")
    for on, what in ((B != 1, f"batch size {B} (one sequence only)"), (dev_sample and not tail, "device sampling"),
                     (penalty and not tail, "repetition_penalty != 1"), (return_scores and not tail, "return_scores")):
        if on:
            raise NotImplementedError(f"draft decoding with {what} is not implemented")
    return K


class LlamaDecode:
    """The decode methods of LlamaHIP (myriad_amd/llama.py), which holds the weights and their packed copies they read."""

    # ------------------------------------------------------------------ generation
    def _gemm_lin(self, li: int, name: str, x, **kw):
        return ops.gemm(x, self.layers[li][name], **kw)

    def _lora_operand(self, lora, li: int, h, fused: bool):
        """The bordered operand [xn | s A xn] of layer li's qkv product with LoRA attached.  `fused`: the norm and the LoRA down
        projection are one launch where that form exists (LoraQV.norm_border, <= 2 rows)."""
        L, x_ext = self.layers[li], lora.x_ext(li, h.shape[0])
        if not (fused and lora.norm_border(li, h, L["ln1"], self.eps, x_ext)):
            ops.rmsnorm_fwd(h, L["ln1"], self.eps, out=x_ext[:, :self.D])
            lora.forward_border(li, x_ext, training=False)
        return x_ext

    def _decode_layers(self, h, lin, attention, lora):
        """All decoder layers on [M, D] f32 rows, every launch of its own: norm, qkv product (the bordered one with `lora`),
        `attention(li, qkv)` -> [.., D] bf16, o_proj with the residual, norm, gate|up, SiLU, down.  `lin(li, name, x, **kw)` is the
        caller's product with layer li's matrix `name`.  The prefills and the unfused token step are this with their own attention."""
        M = h.shape[0]
        for li, L in enumerate(self.layers):
            if lora is None:
                qkv = lin(li, "wqkv", ops.rmsnorm_fwd(h, L["ln1"], self.eps))
            else:
                qkv = lin(li, "wqkv_ext", self._lora_operand(lora, li, h, False))
            o = attention(li, qkv)
            h2 = lin(li, "wo", o.view(M, self.D), residual=h, out_dtype=F32)
            xn2 = ops.rmsnorm_fwd(h2, L["ln2"], self.eps)
            act = ops.silu_mul_fwd_blk(lin(li, "wgu", xn2))
            h = lin(li, "wd", act, residual=h2, out_dtype=F32)
        return h

    def _last_rows_logits(self, last, out=None):
        """The final norm and the row-major lm-head product of [R, D] f32 rows: f32 logits [R, V]."""
        return ops.gemm(ops.rmsnorm_fwd(last, self.norm, self.eps), self.lm_head, out=out, out_dtype=F32)

    def _decode_workspace(self, B: int, T_need: int, inv_temp: float, dev_sample: bool = False, penalty: bool = False,
                          num_beams: int = 1, scores: bool = False):
        """_decode_buffers (and, once captured, the hipGraph) of the single-token step for a batch size, kept across generate()
        calls -- an evaluation run calls generate() once per batch, and re-capturing ~290 launches each time cost ~9 ms per
        call.  The device sampler and the repetition penalty read their knobs and the seed from device memory, so the key holds
        only whether each is on; the arg-max kernel takes inv_temp as an argument, so it stays in the key there.  A step that also
        writes the token scores (`scores`) is another launch sequence and a larger record: its key carries one more item, so a call
        without scores finds the workspace, the graph and the launches it had."""
        T_cap = ops.round_up(T_need + 2, 64)
        key = (B, T_cap, None if dev_sample else float(inv_temp), _decode_weights_id(self), bool(dev_sample), bool(penalty),
               int(num_beams)) + (("scores",) if scores else ())
        ws = self._decode_ws.get(key)
        if ws is None:
            if len(self._decode_ws) >= 3:                               # a few shapes at most: evict the oldest
                self._decode_ws.pop(next(iter(self._decode_ws)))
            ws = self._decode_ws[key] = _decode_buffers(self, B, T_cap, dev_sample or penalty, num_beams, scores=scores)
        return ws

    def _prefill(self, inputs_embeds: torch.Tensor, caches, past: int = 0) -> torch.Tensor:
        """The prefill (eager, host-known lengths) of positions past.. of [B, S0, D] f32 embeddings into `caches`, on top of the
        `past` rows cached already; returns the last position's f32 logits [B, V].  The chunk's rows go to cache rows
        past..S0-1, `pos` holds their rotary positions, and causal masking is aligned to the bottom right."""
        B, S0, D = inputs_embeds.shape
        S, H, hd, W = S0 - past, self.H, self.hd, self.D
        scale = 1.0 / math.sqrt(hd)
        pos = torch.arange(past, S0, dtype=torch.int32).repeat(B).to(self.dev)

        def attention(li, qkv):
            q3, cache = qkv.view(B, S, 3 * W), caches[li]
            ops.rope_(qkv, 0, 2 * H, hd, pos, self.cos, self.sin, 1.0)
            ops.copy3d_bf16(q3[:, :, W:], cache[:, past:S0])             # append k|v (modeling_llama.py:190-195)
            kc = cache[:, :S0]
            return ops.attn_fwd(q3[:, :, :W], kc[:, :, :W], kc[:, :, W:], H, hd, scale, causal=True, need_lse=False)[0]

        h = self._decode_layers(inputs_embeds[:, past:].reshape(B * S, D).contiguous(), self._gemm_lin, attention, self.lora)
        return self._last_rows_logits(h.view(B, S, D)[:, -1].contiguous())

    def _prefill_packed(self, embs, slots, caches, pasts=None) -> torch.Tensor:
        """The prefill of several requests in ONE pass over the decoder weights (the slot engine's prefill_batch > 1): `embs` is a
        list of [S_i, D] f32 embeddings, request i goes to positions 0 .. S_i - 1 of slot slots[i] of `caches` (the slot engine's
        [slots, T, 2D] caches, whole).  The rows are packed one request after the other, `pos` = each row's index within its
        request, and the row count is rounded up to a multiple of 64 with zero rows that belong to no segment (LoraQV.x_ext keeps
        a buffer per row count and the GEMM planner keys on it: a run meets a handful of shapes).  The layers are _prefill's
        (_decode_layers) -- norms, GEMMs, the bordered LoRA, MLP -- with its three attention launches replaced by
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
            past = 0 if pasts is None else pasts[i]
            pos[row:row + n] = torch.arange(past, past + n, dtype=torch.int32)
            seg.append((row, n, int(s)) if pasts is None else (row, n, int(s), past))
            row += n
        seg_host = torch.tensor(seg, dtype=torch.int32)
        last = torch.tensor([t[0] + t[1] - 1 for t in seg], dtype=torch.int32)
        pos, seg_dev, scale = ops.h2d(pos, self.dev), ops.h2d(seg_host, self.dev), 1.0 / math.sqrt(self.hd)

        def attention(li, qkv):                                          # a table with a fourth column: the rows cached already
            attn = ops.attn_prefill_ragged if pasts is None else ops.attn_prefill_ragged_past
            return attn(qkv, pos, seg_dev, seg_host, caches[li], self.cos, self.sin, self.H, self.hd, scale)

        h = self._decode_layers(x, self._gemm_lin, attention, self.lora)
        return self._last_rows_logits(ops.gather_rows_f32(h, ops.h2d(last, self.dev)))

    def _token_logprobs(self, logits: torch.Tensor, targets) -> torch.Tensor:
        """The log-softmax at temperature 1 of each f32 logits row at its target id, on the device (mh_token_scores_rows with no
        watch id): f32 [R]."""
        R = logits.shape[0]
        out = torch.empty((ops.SCORE_ROWS, R), dtype=F32, device=self.dev)
        watch = ops.h2d(torch.full((ops.SCORE_WATCH_MAX,), -1, dtype=torch.int32), self.dev)
        ops.token_scores_rows(logits, ops.h2d(torch.tensor(targets, dtype=torch.long), self.dev), watch, out)
        return out[1]

    def score_continuations(self, prompt_embs, continuations, max_prompts: int = 8, max_rows: int = 2048,
                            return_logits: bool = False):
        """The teacher-forced token log-probs of candidate continuations of prompts, nothing decoded: `prompt_embs` is a list of
        [S_i, D] f32 embeddings, `continuations` per prompt a list of 1-D integer id tensors (or lists).  Returns, per prompt, a
        list of f32 [n] CPU tensors: entry j is log p(t_j | prompt, t_<j), the log-softmax at temperature 1 of the f32 logits at
        t_j (mh_token_scores_rows; the host never recomputes a softmax).  Two passes over the decoder weights per group of at most
        `max_prompts` prompts (decode_host.ScorePlan; more when the candidates' rows exceed `max_rows`):

          1. _prefill_packed of the prompts, as it is, into the caches of _decode_workspace; its [P, V] last-row logits give every
             candidate's first token;
          2. the candidates' rows t_0 .. t_{n-2} of all prompts packed into one zero-padded frame of a multiple of 64 rows, the
             prefill's own layers (_decode_layers: the bordered LoRA, norms, GEMMs, MLP) with mh_attn_prefill_ragged_shared as the
             attention -- every candidate of a prompt continues that prompt's cached rows, attends causally to its own rows only
             and writes no cache row -- then the final norm and the lm-head on all segment rows.

        The caches must hold past + len rows for the attention entry to take a segment, so their T covers max S_i plus the longest
        candidate; cache rows >= S_i are neither read nor written.  A decode call after this one prefills anew, as always.
        A candidate's log-probs do not depend on its neighbours as long as the GEMMs' plans are the same: the frame's padded row
        count and, for the lm-head, the count of scored rows (_prefill_packed's docstring).
        This path runs on the bf16 prefill weights: MYRIAD_DECODE_FP8 / _FP4 / _MERGE_LORA concern the token step and do not
        change it.  LoRA dropout is off, as in every decode path.  Sets `last_score_stats` (passes, packed_rows, segments,
        prompts, candidates).  `return_logits` (debug): also returns, per prompt and candidate, the f32 [n, V] logits rows on the
        CPU each log-prob was read from."""
        embs = list(prompt_embs)
        cands = [[[int(t) for t in (c.tolist() if hasattr(c, "tolist") else c)] for c in cs] for cs in continuations]
        plan = ScorePlan([int(e.shape[0]) for e in embs], cands, self.V, self.cos.shape[0], max_prompts, max_rows)
        if self.lora is not None:
            self.lora.refresh(self.layers)
        scale = 1.0 / math.sqrt(self.hd)
        out = [[torch.zeros((len(c),), dtype=F32) for c in cs] for cs in cands]
        rows_of = [[torch.zeros((len(c), self.V), dtype=F32) for c in cs] for cs in cands] if return_logits else None

        def scatter(lp: torch.Tensor, logits: torch.Tensor, where) -> None:
            """Rows r of `lp` (and of `logits`) to their (prompt, candidate, token index) = where[r], a candidate's run at once."""
            lp = lp.cpu()
            logits = logits.cpu() if return_logits else None
            r = 0
            while r < len(where):
                i, c, j = where[r]
                e = r + 1
                while e < len(where) and where[e][:2] == (i, c):
                    e += 1
                out[i][c][j:j + e - r] = lp[r:e]
                if return_logits:
                    rows_of[i][c][j:j + e - r] = logits[r:e]
                r = e

        for g in plan.groups:
            members = g["prompts"]
            T_need = max(plan.prompt_lens[i] + max(len(c) for c in cands[i]) - 1 for i in members)
            caches = self._decode_workspace(len(members), T_need, 1.0)["caches"]
            logits0 = self._prefill_packed([embs[i] for i in members], g["slots"], caches)
            first = ops.gather_rows_f32(logits0, ops.h2d(torch.tensor(g["first_rows"], dtype=torch.int32), self.dev))
            scatter(self._token_logprobs(first, g["first_targets"]), first, g["first_map"])
            for ps in g["passes"]:
                n = len(ps["ids"])
                x = torch.zeros((ps["M"], self.D), dtype=F32, device=self.dev)
                self.embed_tokens_into(ops.h2d(torch.tensor(ps["ids"], dtype=torch.long), self.dev), x)
                pos = torch.zeros((ps["M"],), dtype=torch.int32)
                pos[:n] = torch.tensor(ps["pos"], dtype=torch.int32)
                seg_host = torch.tensor(ps["seg"], dtype=torch.int32)
                pos_dev, seg_dev = ops.h2d(pos, self.dev), ops.h2d(seg_host, self.dev)

                def attention(li, qkv):
                    return ops.attn_prefill_ragged_shared(qkv, pos_dev, seg_dev, seg_host, caches[li], self.cos, self.sin, self.H,
                                                          self.hd, scale)

                h = self._decode_layers(x, self._gemm_lin, attention, self.lora)
                rows = ops.gather_rows_f32(h, ops.h2d(torch.arange(n, dtype=torch.int32), self.dev))
                logits = self._last_rows_logits(rows)
                scatter(self._token_logprobs(logits, ps["targets"]), logits, ps["map"])
        self.last_score_stats = dict(passes=plan.passes, packed_rows=plan.packed_rows, segments=plan.segments,
                                     prompts=len(embs), candidates=sum(len(cs) for cs in cands))
        return (out, rows_of) if return_logits else out

    def _step_layers(self, ws: dict) -> torch.Tensor:
        """All decoder layers for one decode token per row of ws["x_in"], whose position lives in device memory (ws["pos"] /
        ws["kvlen"]), which makes the launch sequence replayable from a hipGraph: the fused packed step when the workspace's rows
        stream the packed copies and decode_fused is on, else every launch of its own (_decode_layers)."""
        rows = ws["x_in"].shape[0]
        packed = self._packed["layers"] if _packed_step(self, rows, ws["row_limit"]) else None
        # the bordered LoRA product unless the packed qkv copy has the LoRA merged in (decode_merge_lora)
        lora = None if packed is not None and self._packed["qkv_key"] == "merged" else self.lora
        if packed is not None and self.decode_fused:
            return self._fused_step_layers(ws, packed, lora)
        if ws.get("live") is not None:
            raise ValueError("per-row decode state needs the fused packed token step")
        if ws.get("draft_k"):
            raise ValueError("draft decoding needs the fused packed token step")
        H, hd, W, pos, scale = self.H, self.hd, self.D, ws["pos"], 1.0 / math.sqrt(self.hd)

        def lin(li, name, x, **kw):
            return ops.gemv_packed(x, packed[li]["wqkv" if name.startswith("wqkv") else name], **kw)

        def attention(li, qkv):
            q3, cache = qkv.view(rows, 1, 3 * W), ws["caches"][li]
            ops.rope_kv_append(qkv, H, hd, pos, self.cos, self.sin, cache, pos)       # rotary + append, one launch
            return ops.attn_fwd(q3[:, :, :W], cache[:, :, :W], cache[:, :, W:], H, hd, scale, causal=False, kv_len=ws["kvlen"],
                                need_lse=False)[0]

        return self._decode_layers(ws["x_in"], self._gemm_lin if packed is None else lin, attention, lora)

    def _fused_step_layers(self, ws: dict, packed, lora) -> torch.Tensor:
        """Single-token step on the packed copies: four launches per layer instead of nine -- the two RMSNorms
        and the SiLU gate are rebuilt by every workgroup of the product that consumes them (mh_gemv_packed_rmsnorm /
        _silu), rotary + KV append ride the attention launch (mh_attn_decode_rope); each fused form is bit-identical
        to the launches it replaces (tests/test_kernels_gpu.py), MYRIAD_DECODE_FUSED=0 keeps the separate launches.
        With LoRA attached the qkv product takes the bordered operand [xn | s A xn]: the norm and the LoRA down projection are
        one launch (LoraQV.norm_border, <= 2 rows), the bordered packed weight the next -- five launches per layer become six.
        With the LoRA merged into the packed qkv copy (decode_merge_lora) the step is the no-LoRA one.

        The attention kernel is chosen once, from what the workspace holds.  ws["split"] (the partials buffer of
        ops.attn_decode_split_ws) makes it the split-KV kernel.  ws["live"] (int32 [rows] on the device, the slot engine's) makes
        it the rows kernel instead: every row appends at its own pos[b], idle rows are skipped; only the fused step has that
        form.  Both together: the split-KV kernel in its rows form (ops.attn_decode_rope_split_rows), at 1 to GEMV_WIDE_MAX_ROWS
        rows alike.  Above GEMV_MAX_ROWS rows (_wide_step) the products are ops.gemv_packed_wide and the norm / SiLU products take
        their two-launch forms.  ws["draft_k"] = K (_draft_view, draft decoding's verify step): the rows are K consecutive tokens
        of one sequence and the attention is ops.attn_decode_rope_draft, row j at position pos + j; with ws["nrow"] beside it (the
        slot engine's verify view) the rows are K per slot and the attention is ops.attn_decode_rope_draft_rows on (pos, live, nrow).
        ws["split_draft"] (the partials of ops.attn_decode_split_draft_ws, a verify view of the split-KV step) swaps those two for
        ops.attn_decode_rope_split_draft[_rows], whose rows carry the split-KV kernel's bits."""
        H, hd, scale, cos, sin = self.H, self.hd, 1.0 / math.sqrt(self.hd), self.cos, self.sin
        pos, kvlen, live, split = ws["pos"], ws["kvlen"], ws.get("live"), ws["split"]
        wide = _wide_step(self, ws["x_in"].shape[0], ws["row_limit"])
        if live is not None:                                             # per-row state: (pos, kvlen, live)
            attention, state = ops.attn_decode_rope_rows if split is None else ops.attn_decode_rope_split_rows, (pos, kvlen, live)
        else:                                                            # one position for all rows: (pos, pos_dev, kvlen)
            attention, state = ops.attn_decode_rope if split is None else ops.attn_decode_rope_split, (pos, pos, kvlen)
        partials = () if split is None else (split,)
        if ws.get("draft_k") and ws.get("nrow") is not None:             # the slots' verify step: K rows per slot, (pos, live, nrow)
            attention, state, partials = ops.attn_decode_rope_draft_rows, (pos, live, ws["nrow"]), (ws["draft_k"],)
        elif ws.get("draft_k"):                                          # K consecutive rows of one sequence: (pos, live), K behind
            attention, state, partials = ops.attn_decode_rope_draft, (pos, ws["live1"]), (ws["draft_k"],)
        if ws.get("draft_k") and ws.get("split_draft") is not None:      # the same two on the split-KV view: K, then the partials
            attention = ops.attn_decode_rope_split_draft if ws.get("nrow") is None else ops.attn_decode_rope_split_draft_rows
            partials = (ws["draft_k"], ws["split_draft"])

        def gemv(x, w, **kw):
            return (ops.gemv_packed_wide if wide else ops.gemv_packed)(x, w, **kw)

        def norm_gemv(x, norm_w, w):                                     # one launch where the fused form fits, else two
            y = None if wide else ops.gemv_packed_rmsnorm(x, norm_w, self.eps, w)
            return y if y is not None else gemv(ops.rmsnorm_fwd(x, norm_w, self.eps), w)

        h = ws["x_in"]
        for li, (L, P, cache) in enumerate(zip(self.layers, packed, ws["caches"])):
            qkv = norm_gemv(h, L["ln1"], P["wqkv"]) if lora is None else gemv(self._lora_operand(lora, li, h, True), P["wqkv"])
            o = attention(qkv, cache, *state, cos, sin, H, hd, scale, *partials)
            h2 = gemv(o, P["wo"], residual=h, out_dtype=F32)
            gu = norm_gemv(h2, L["ln2"], P["wgu"])
            hn = None if wide else ops.gemv_packed_silu(gu, P["wd"], residual=h2, out_dtype=F32)
            h = hn if hn is not None else gemv(ops.silu_mul_fwd_blk(gu), P["wd"], residual=h2, out_dtype=F32)
        return h

    def _step_logits(self, ws: dict) -> None:
        """The token step up to its logits: embed the fed ids ws["ids"], every decoder layer at the device-resident position,
        the final norm + lm-head into ws["logits"] -- one launch on the packed copy when the fused form fits, else the norm and
        the packed GEMV, or the GEMM above the workspace's row limit (the wide packed GEMV above GEMV_MAX_ROWS rows within it:
        the slot engine's)."""
        ops.embed_gather(self.embed, ws["ids"], ws["x_in"])
        rows = ws["x_in"].shape[0]
        h = self._step_layers(ws)
        if not _packed_step(self, rows, ws["row_limit"]):
            self._last_rows_logits(h, out=ws["logits"])
            return
        wide, lm_head = _wide_step(self, rows, ws["row_limit"]), self._packed["lm_head"]
        if not wide and self.decode_fused and \
                ops.gemv_packed_rmsnorm(h, self.norm, self.eps, lm_head, out=ws["logits"], out_dtype=F32) is not None:
            return
        hn = ops.rmsnorm_fwd(h, self.norm, self.eps)
        (ops.gemv_packed_wide if wide else ops.gemv_packed)(hn, lm_head, out=ws["logits"], out_dtype=F32)

    @staticmethod
    def _launch_step(ws: dict, token_step, ban: int, use_graph: bool, stats: dict) -> bool:
        """Enqueue one token step: a replay of ws's captured graph when there is one (counted in stats["graph_replays"]).  A step
        with a ban runs eagerly; an eager ban-free step after an earlier eager one captures the next (kernels are warm, buffers
        fixed).  Returns whether this call captured."""
        if ban == -1 and use_graph and ws["graph"] is not None:
            ws["graph"].replay()
            stats["graph_replays"] += 1
            return False
        token_step(ban)
        captured = ban == -1 and use_graph and ws["warm"]
        if captured:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            # torch.cuda.graph does not collect garbage on entry, so the cyclic collector may run in mid-capture and finalise a
            # dead cycle that still holds an earlier loop's graph and its memory pool -- the process aborted there.  Collect
            # before the capture begins and keep the collector off until it has ended.
            gc_was_on = gc.isenabled()
            gc.collect()
            gc.disable()
            try:
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    token_step(-1)
            finally:
                if gc_was_on:
                    gc.enable()
            ws["graph"] = g
        ws["warm"] = True
        return captured

    @torch.no_grad()
    def greedy_generate(self, inputs_embeds: torch.Tensor, max_new_tokens: int = 90,
                        stop_ids=((835,), (2277, 29937)), eos_id: int = 2, min_length: int = 1,
                        return_margins: bool = False, use_graph: bool = True, do_sample: bool = False,
                        top_p: float = 1.0, temperature: float = 1.0, generator: Optional[torch.Generator] = None,
                        top_k: int = 50, repetition_penalty: float = 1.0, return_scores: bool = False, watch_ids=(), draft=None,
                        draft_k: int = 4):
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
        on the device to the step's logits before any pick, greedy, host or device draw.

        `return_scores` (opt-in; a workspace and a captured step of its own) appends a dict to the return: `token_logprobs` [B, L]
        f32, the log-probability of every returned id, and `watch_logprobs` [B, L, W], that of each of the W <= 8 `watch_ids` at
        the same step.  Both are the log-softmax at temperature 1 of the logits the pick was made from -- after the repetition
        penalty when it is on; temperature, top-k, top-p and the EOS ban do not enter -- computed inside the step
        (mh_token_scores_rows, after the pick and before the advance) into rows of the step's record, so a step is still one
        device->host copy.  Positions padded after a row finished are 0.0.  A row the host re-draws takes its log-prob from the
        logits row the host reads for the draw and the recorded normaliser.

        `draft` (opt-in, B = 1; a drafter with `propose` / `observe`, decode_host.NgramDrafter) with `draft_k` = K rows: draft-and-
        verify decoding (_draft_core).  Steps past `min_length` feed the last token and K - 1 guessed tokens as K rows of one token
        step and keep the guesses the arg-max confirms plus the one token the step produces anyway.  Every row of that step has the
        bits of the one-row step at its position, so ids and margins are those of the call without `draft`, whatever the drafter
        proposes; it only decides how many passes over the weights the answer takes.  NotImplementedError with B > 1, and -- unless
        `draft_sampling` (MYRIAD_DRAFT_SAMPLING=1, off by default) is on -- with device sampling, `repetition_penalty` != 1 or
        `return_scores`.  With it on the verify step draws, penalises and scores every row as the plain step would at that row's
        token index (_draft_core), so the sampled, penalised or scored answer is again that of the call without `draft`."""
        B, S0, _ = inputs_embeds.shape
        inv_temp, _, dev_sample, penalty = _sampling_args(self, do_sample, temperature, top_k, repetition_penalty)
        ops.score_watch_ids(watch_ids if return_scores else (), self.V)
        K = 0 if draft is None else _draft_refusals(B, dev_sample, penalty, bool(return_scores), draft_k, self.draft_sampling)
        if K and S0 + max_new_tokens + K > self.cos.shape[0]:        # a verify step rotates K rows past the last fed position
            raise ValueError(f"context {S0} + max_new_tokens {max_new_tokens} + draft_k {K} passes the rotary table "
                             f"({self.cos.shape[0]} positions)")
        weight_stats = self._prepare_decode_weights(B)
        ws = self._decode_workspace(B, S0 + max_new_tokens + K, inv_temp, dev_sample, penalty, scores=bool(return_scores))
        return self._greedy_core(inputs_embeds, ws, 0, weight_stats, max_new_tokens, stop_ids, eos_id, min_length, return_margins,
                                 use_graph, do_sample, top_p, temperature, generator, top_k, repetition_penalty, return_scores,
                                 watch_ids, draft, draft_k)

    def _greedy_core(self, inputs_embeds: torch.Tensor, ws: dict, past: int, weight_stats: dict, max_new_tokens: int = 90,
                     stop_ids=((835,), (2277, 29937)), eos_id: int = 2, min_length: int = 1, return_margins: bool = False,
                     use_graph: bool = True, do_sample: bool = False, top_p: float = 1.0, temperature: float = 1.0,
                     generator: Optional[torch.Generator] = None, top_k: int = 50, repetition_penalty: float = 1.0,
                     return_scores: bool = False, watch_ids=(), draft=None, draft_k: int = 4):
        """greedy_generate's body on the caller's workspace `ws` (greedy_generate's from the _decode_ws cache, a DecodeSession's
        own buffers and graphs), on top of the cached prefix `past` that is not prefilled again; `weight_stats` is what
        _prepare_decode_weights answered for this call.  The other arguments are greedy_generate's, in its order."""
        B, S0, _ = inputs_embeds.shape
        inv_temp, top_k, dev_sample, penalty = _sampling_args(self, do_sample, temperature, top_k, repetition_penalty)
        if draft is not None:
            K = _draft_refusals(B, dev_sample, penalty, bool(return_scores), draft_k, self.draft_sampling)
            return self._draft_core(inputs_embeds, ws, past, weight_stats, draft, K, max_new_tokens, stop_ids, eos_id, min_length,
                                    return_margins, use_graph, do_sample, top_p, inv_temp, top_k, generator, dev_sample,
                                    repetition_penalty if penalty else None, watch_ids if return_scores else None)
        out_ids, margins = [], []
        unfinished = torch.ones(B, dtype=torch.long)
        stats = dict(steps=0, sampled_rows=0, min_pmax=1.0, device_sampled_rows=0, host_sampled_rows=0, graph_replays=0, **weight_stats)
        self.last_generate_stats = stats
        scores = bool(return_scores)
        if scores:                                                   # ws is a scores workspace / view: its record has the rows
            watch = ops.score_watch_table(watch_ids, self.V)
            if ws["rec"].shape[0] != 4 + ops.SCORE_ROWS:
                raise ValueError("return_scores needs a workspace whose record holds the score rows")
            ws["watch"].copy_(watch)
            W, srec, tok_lp, watch_lp = int((watch >= 0).sum()), ws["rec"][4:], [], []
        rec = ws["rec"] if scores else ws["rec"][:4 if dev_sample else 3]      # the sampler's kept counts are the fourth row
        if dev_sample or penalty:
            ws["prm"].copy_(torch.tensor([inv_temp, top_p, float(top_k), float(repetition_penalty)], dtype=F32))
            ws["seen"].zero_()                                       # generated ids only: the prompt is embeddings
        if dev_sample:
            ws["seed"].fill_(int(torch.randint(0, 2**63 - 1, (1,), generator=generator)))

        def record(nxt: torch.Tensor, mar: torch.Tensor, pm: torch.Tensor, ban: int, logits_of=None, kept=None, sc=None):
            """Host bookkeeping of one step's picks.  Returns (done, redrawn): redrawn = a live row was re-drawn on the host
            (finished rows are fed their raw arg-max instead of EOS by the device: rows are independent and their outputs are
            overwritten with EOS here).  `sc` = the step's score rows [SCORE_ROWS, B] on the host, with scores on."""
            nonlocal unfinished
            margins.append(mar)
            stats["steps"] += 1
            redrawn = False
            alive = unfinished.bool()                                # rows whose pick of this step is part of their answer
            lp = sc[1].clone() if scores else None
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
                        nxt[row] = _host_draw(logits_of()[row], ban, inv_temp, top_k, top_p, generator)
                        stats["host_sampled_rows"] += 1
                        redrawn = True
                        if scores:                                   # x[id] - lse in f32, from the row the draw read
                            lp[row] = logits_of()[row, int(nxt[row])].cpu() - sc[0, row]
            if scores:
                tok_lp.append(torch.where(alive, lp, torch.zeros_like(lp)))
                wl = sc[2:2 + W].t()
                watch_lp.append(torch.where(alive[:, None], wl, torch.zeros_like(wl)))
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
        if scores:
            ops.token_scores_rows(logits0, ws["nxt"], ws["watch"], srec)
        done, _ = record(ws["nxt"].cpu(), ws["mar"].cpu(), ws["pmx"].cpu(), ban0, logits_of=lambda: logits0,
                         kept=ws["kept"].cpu() if dev_sample else None, sc=srec.cpu() if scores else None)

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
                if scores:
                    ops.token_scores_rows(ws["logits"], ws["nxt"], ws["watch"], srec)
                ops.decode_advance_kept(ws["nxt"], ws["mar"], ws["pmx"], ws["kept"], rec, ws["ids"], ws["step"], ws["pos"],
                                        ws["kvlen"])
                return
            ops.argmax_pmax_rows(ws["logits"], ws["nxt"], ws["mar"], ws["pmx"], ban_id=ban, inv_temp=inv_temp)
            if scores:
                ops.token_scores_rows(ws["logits"], ws["nxt"], ws["watch"], srec)
            ops.decode_advance(ws["nxt"], ws["mar"], ws["pmx"], rec, ws["ids"], ws["step"], ws["pos"], ws["kvlen"])

        step = 1                                                     # tokens generated so far (= index of the next one)
        if not done and step < max_new_tokens:
            ws["ids"].copy_(out_ids[-1].to(self.dev))
        while not done and step < max_new_tokens:
            ban = eos_id if step < min_length else -1
            self._launch_step(ws, token_step, ban, use_graph, stats)
            r = rec.cpu()                                            # the one device->host copy of the step (it also waits for it)
            done, redrawn = record(r[0].long(), r[1].clone(), r[2].clone(), ban, logits_of=lambda: ws["logits"],
                                   kept=r[3] if dev_sample else None, sc=r[4:] if scores else None)
            if redrawn and not done:
                ws["ids"].copy_(out_ids[-1].to(self.dev))            # a host draw replaces the arg-max the step fed back to itself
            step += 1
        ids = torch.stack(out_ids, 1)
        out = (ids, torch.stack(margins, 1)) if return_margins else (ids,)
        if scores:
            out += (dict(token_logprobs=torch.stack(tok_lp, 1), watch_logprobs=torch.stack(watch_lp, 1)),)
        return out if len(out) > 1 else ids

    def _draft_core(self, inputs_embeds: torch.Tensor, ws: dict, past: int, weight_stats: dict, draft, K: int, max_new_tokens: int,
                    stop_ids, eos_id: int, min_length: int, return_margins: bool, use_graph: bool, do_sample: bool, top_p: float,
                    inv_temp: float, top_k: int, generator, dev_sample: bool = False, repetition_penalty=None, watch_ids=None):
        """_greedy_core for one sequence with draft-and-verify steps (greedy_generate(draft=...)).  The prefill and its first pick
        are _greedy_core's.  Then decode_host.DraftLoop chooses each step: while the EOS ban is on, or when the drafter proposes
        nothing, the plain one-row step of `ws`; otherwise the host writes the K - 1 guesses (id 0 as filler) behind the fed token
        and replays the K-row verify step of _draft_view -- embed, the fused packed layers at K rows with
        mh_attn_decode_rope_draft, final norm and lm-head at K rows, mh_argmax_pmax_rows, mh_draft_accept, which records the K
        picks and how many of them stand, feeds the last of those back and moves pos / kvlen past them.  Both steps read and
        advance the same caches, pos, kvlen, ids_k[0] and step, each from a graph of its own; a row of the verify step has the bits
        of the plain step at its position, so switching is free and the answer is the plain loop's.  Per step the host makes one
        device->host copy (the record) and at most one small host->device copy (the guesses, with a host-drawn id in front).

        `dev_sample`, `repetition_penalty` (None: off) and `watch_ids` (None: no scores), behind `draft_sampling`: the verify step
        runs the decode slots' per-row tail at G = 1 instead (draft_sample.hip) -- mh_repetition_penalty_draft_rows,
        mh_sample_rows_draft with the device sampler (else mh_argmax_pmax_rows: the loop drafts only past min_length),
        mh_token_scores_rows over the K rows, mh_draft_accept_sampled_rows -- and the plain step is _greedy_core's, except with the
        device sampler: _greedy_core's sampled step counts launches in `step`, so both steps of this call take the slot form and
        count tokens in `gen` (mh_sample_rows_slots at one row, Philox counter (t, 0, 0, 0): the draw of the solo step for token
        t).  Row j of the verify step draws token gen + j itself, so a guess stands iff it equals the draw and the answer is the
        sampled answer of the call without `draft`.

        The verify step is off for the whole call, and last_generate_stats["draft_off"] says why, when `ws` runs the split-KV
        attention with `draft_split` off ("split_kv") or the verify step's attention launch -- mh_attn_decode_rope_draft, on the
        split-KV view mh_attn_decode_rope_split_draft -- does not take the shape ("unsupported").  Stats: verify_steps,
        plain_steps, draft_proposed, draft_accepted (DraftLoop), verify_graph_replays and plain_graph_replays beside graph_replays."""
        _, S0, _ = inputs_embeds.shape
        if not (_packed_step(self, K, ws["row_limit"]) and self.decode_fused):
            raise ValueError("draft decoding needs the fused packed token step (MYRIAD_PACK_DECODE and MYRIAD_DECODE_FUSED on)")
        if ws["T"] < S0 + max_new_tokens + K:
            raise ValueError(f"draft decoding needs a cache of {S0 + max_new_tokens + K} positions, the workspace holds {ws['T']}")
        stats = dict(steps=0, sampled_rows=0, min_pmax=1.0, device_sampled_rows=0, host_sampled_rows=0, graph_replays=0,
                     verify_graph_replays=0, plain_graph_replays=0, draft_k=K, draft_off=None, **weight_stats)
        self.last_generate_stats = stats
        penalty, scores = repetition_penalty is not None, watch_ids is not None
        tail = (dev_sample, penalty, scores) if dev_sample or penalty or scores else None
        loop = DraftLoop(draft, K, max_new_tokens, stop_ids, eos_id, min_length, do_sample, top_p, stats)
        split = ws["split"] is not None
        if split and not getattr(self, "draft_split", False):
            stats["draft_off"] = "split_kv"
        elif not (ops.attn_decode_split_draft_supported(self.H, self.hd, K, ws["T"]) if split else
                  ops.attn_decode_draft_supported(self.H, self.hd, K, ws["T"])):
            stats["draft_off"] = "unsupported"
        loop.use_draft = stats["draft_off"] is None
        dv = _draft_view(self, ws, K, inv_temp, tail, split and loop.use_draft) if loop.use_draft or dev_sample else None
        pv = dv["draft_views"]["plain_rows", penalty, scores] if dev_sample else ws      # the view of the call's plain step
        rec = ws["rec"] if scores else ws["rec"][:4 if dev_sample else 3]
        ids_k, fresh, sc_rows = ws["ids_k"], [True], []
        if scores:
            watch = ops.score_watch_table(watch_ids, self.V)
            if ws["rec"].shape[0] != 4 + ops.SCORE_ROWS:
                raise ValueError("return_scores needs a workspace whose record holds the score rows")
            ws["watch"].copy_(watch)
            W = int((watch >= 0).sum())
        if dev_sample or penalty:                                    # _greedy_core's: the knobs, an empty seen set, one seed per call
            ws["prm"].copy_(torch.tensor([inv_temp, top_p, float(top_k), float(repetition_penalty or 1.0)], dtype=F32))
            ws["seen"].zero_()
        if dev_sample:
            ws["seed"].fill_(int(torch.randint(0, 2**63 - 1, (1,), generator=generator)))
            ws["prm6"].copy_(torch.tensor([inv_temp, top_p, float(top_k), float(repetition_penalty or 1.0), float(min_length),
                                           float(eos_id)], dtype=F32))

        def draw_from(logits, ban):
            return lambda j: _host_draw(logits()[j], ban, inv_temp, top_k, top_p, generator)

        def take(record, logits, first=False):
            """A step's record (ids, margins, pmax, n_out, draw, kept, score rows) into the loop; with scores every token the loop
            emitted takes its entries -- a token the host drew instead x[id] - lse from the row the draw read, as _greedy_core."""
            n0, sc = len(loop.ids), record[6]
            loop.take(*record[:5], first=first, kept=record[5])
            for j, tok in enumerate(loop.ids[n0:] if scores else ()):
                lp = sc[1][j] if tok == record[0][j] else float(logits()[j, tok].cpu() - torch.tensor(sc[0][j], dtype=F32))
                sc_rows.append([lp] + [sc[2 + w][j] for w in range(W)])

        logits0 = self._prefill(inputs_embeds, ws["caches"], past)
        ban0 = eos_id if 0 < min_length else -1
        if dev_sample:                                               # the prefill pick is Philox step t = 0
            ops.sample_rows(logits0, ws["nxt"], ws["mar"], ws["pmx"], ws["kept"], ws["prm"], ws["seed"], ban_id=ban0, t_add=0)
        else:
            ops.argmax_pmax_rows(logits0, ws["nxt"], ws["mar"], ws["pmx"], ban_id=ban0, inv_temp=inv_temp)
        if scores:
            ops.token_scores_rows(logits0, ws["nxt"], ws["watch"], ws["rec"][4:])
        first = (ws["nxt"].cpu().tolist(), ws["mar"].cpu().tolist(), ws["pmx"].cpu().tolist(), 1, draw_from(lambda: logits0, ban0),
                 ws["kept"].cpu().tolist() if dev_sample else None, ws["rec"][4:].cpu().tolist() if scores else None)
        ws["pos"].fill_(S0)                                          # position of the incoming token
        ws["kvlen"].fill_(S0 + 1)                                    # valid keys after the append
        ws["step"].zero_()
        if tail is not None:
            ws["gen"].fill_(1)                                       # the prefill pick was token 0
        if dv is not None:
            dv["top_p"].fill_(float(top_p) if do_sample else 0.0)    # <= 0: no row needs a draw

        def feed(fed, guesses=()):
            """The step's host->device copy: the guesses, behind the fed token when the host chose it (the prefill's pick, a draw)."""
            lead = fresh[0] or fed is not None
            fresh[0] = False
            vals = ([loop.ids[-1]] if lead else []) + list(guesses)
            if vals:
                lo = 0 if lead else 1
                ids_k[lo:lo + len(vals)].copy_(torch.tensor(vals, dtype=torch.long))

        def launch(view, token_step, ban, counter):
            before = stats["graph_replays"]
            self._launch_step(view, token_step, ban, use_graph, stats)
            stats[counter] += stats["graph_replays"] - before

        def plain_token_step(ban):
            self._step_logits(ws)
            if penalty:                                              # ws["ids"] = the token fed in: it joins the seen set first
                ops.repetition_penalty_rows(ws["logits"], ws["seen"], ws["ids"], ws["prm"][3:])
            if dev_sample:                                           # the slot form at one row: token gen draws Philox step gen, and
                ops.sample_rows_slots(ws["logits"], ws["nxt"], ws["mar"], ws["pmx"], ws["kept"], ws["prm6"], ws["seed"], ws["gen"])
            else:                                                    # the ban is gen < min_length (the launch's `ban` is unused)
                ops.argmax_pmax_rows(ws["logits"], ws["nxt"], ws["mar"], ws["pmx"], ban_id=ban, inv_temp=inv_temp)
            if scores:
                ops.token_scores_rows(ws["logits"], ws["nxt"], ws["watch"], ws["rec"][4:])
            if dev_sample:
                ops.decode_advance_kept_rows(ws["nxt"], ws["mar"], ws["pmx"], ws["kept"], rec, ws["ids"], ws["step"], ws["pos"],
                                             ws["kvlen"], ws["gen"], pv["live1"])
            else:
                ops.decode_advance(ws["nxt"], ws["mar"], ws["pmx"], rec, ws["ids"], ws["step"], ws["pos"], ws["kvlen"])

        def verify_token_step(_ban):
            self._step_logits(dv)
            if tail is None:
                ops.argmax_pmax_rows(dv["logits"], dv["nxt"], dv["mar"], dv["pmx"], ban_id=-1, inv_temp=inv_temp)
                ops.draft_accept(dv["nxt"], dv["mar"], dv["pmx"], dv["ids"], dv["top_p"], dv["drec"], ws["pos"], ws["kvlen"], ws["step"], K)
                return
            if penalty:                                              # row j: the seen set plus the ids fed in rows 0 .. j
                ops.repetition_penalty_draft_rows(dv["logits"], ws["seen"], dv["ids"], dv["full"], dv["live1"], ws["prm"][3:], K)
            if dev_sample:                                           # row j draws Philox step gen + j
                ops.sample_rows_draft(dv["logits"], dv["nxt"], dv["mar"], dv["pmx"], dv["kept"], ws["prm6"], ws["seed"], ws["gen"],
                                      dv["full"], dv["live1"], K, True)
            else:
                ops.argmax_pmax_rows(dv["logits"], dv["nxt"], dv["mar"], dv["pmx"], ban_id=-1, inv_temp=inv_temp)
            if scores:
                ops.token_scores_rows(dv["logits"], dv["nxt"], ws["watch"], dv["sc"])
            ops.draft_accept_sampled_rows(dv["nxt"], dv["mar"], dv["pmx"], dv["kept"] if dev_sample else None, dv["ids"], ws["ids"],
                                          dv["ngs"], dv["live1"], dv["top_p"], ws["seen"] if penalty else None, dv["arec"], ws["pos"],
                                          ws["kvlen"], ws["gen"], ws["step"], K, self.V)

        def plain_step(ban, fed):
            feed(fed)
            launch(pv, plain_token_step, -1 if dev_sample else ban, "plain_graph_replays")
            r = rec.cpu()                                            # the one device->host copy of the step (it also waits for it)
            return (r[0].long().tolist(), r[1].tolist(), r[2].tolist(), 1, draw_from(lambda: ws["logits"], ban),
                    r[3].tolist() if dev_sample else None, r[4:].tolist() if scores else None), lambda: ws["logits"]

        def verify_step(guesses, fed):
            feed(fed, guesses)
            launch(dv, verify_token_step, -1, "verify_graph_replays")
            r = dv["drec"].cpu()
            out = (r[:K].long().tolist(), r[K:2 * K].tolist(), r[2 * K:3 * K].tolist())
            if tail is None:
                return out + (int(r[3 * K]), draw_from(lambda: dv["logits"], -1), None, None), lambda: dv["logits"]
            return out + (int(r[4 * K]), draw_from(lambda: dv["logits"], -1), r[3 * K:4 * K].tolist() if dev_sample else None,
                          r[4 * K + 1:].view(ops.SCORE_ROWS, K).tolist() if scores else None), lambda: dv["logits"]

        take(first, lambda: logits0, first=True)
        while not loop.done:
            g = loop.guesses()
            take(*(verify_step(g, loop.fed) if g else plain_step(loop.ban(), loop.fed)))
        ids = torch.tensor([loop.ids], dtype=torch.long)
        out = (ids, torch.tensor([loop.margins], dtype=F32)) if return_margins else (ids,)
        if scores:
            sc = torch.tensor(sc_rows, dtype=torch.float64).to(F32).view(1, len(loop.ids), 1 + W)
            out += (dict(token_logprobs=sc[:, :, 0].contiguous(), watch_logprobs=sc[:, :, 1:].contiguous()),)
        return out if len(out) > 1 else ids

    @torch.no_grad()
    def beam_generate(self, inputs_embeds: torch.Tensor, num_beams: int, max_new_tokens: int = 90, stop_ids=(), eos_id: int = 2,
                      min_length: int = 1, length_penalty: float = 1.0, early_stopping=False, num_return_sequences: int = 1,
                      use_graph: bool = True, return_scores: bool = False, pad_id: Optional[int] = None, do_sample: bool = False,
                      temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0, repetition_penalty: float = 1.0,
                      generator: Optional[torch.Generator] = None):
        """Beam search from [B,S0,D] f32 embeddings, HF GenerationMixin._beam_search: the host rule (per-hypothesis stops, where
        greedy_generate keeps the reference's row-0 rule; running beams, finished pool, `early_stopping`) is decode_host.BeamItem's,
        one per batch item, and the batch goes on by decode_host.beam_batch_going.  Returns [B * num_return_sequences, L] int64
        (CPU), generated ids only, the hypotheses of item b at rows b * nrs .. b * nrs + nrs - 1 best first, right-padded with
        pad_id (default EOS); with return_scores also their sequence scores (sum log-probs / len ** length_penalty), which
        last_generate_stats["sequences_scores"] holds either way.

        Device / host split.  The prefill runs at B rows, writing its keys / values into row b * nb of the B * nb row caches,
        and one mh_beam_reorder_kv broadcasts them over [0, S0) to the item's other beams.  The token step (captured into a
        hipGraph, like greedy's) is: reorder the generated positions [S0, pos) of every cache by the parent rows `src`, embed
        the fed tokens, the decoder layers at B * nb rows (packed GEMV up to GEMV_MAX_ROWS), lm-head, mh_beam_topk (log-softmax +
        running score + EOS ban, per item the top 2 * nb candidates), pos / kvlen += 1.  The host reads the [2, B, 2*nb]
        record (one device->host copy), selects every item, and writes the next step's (ids, src, running scores) with one
        host->device copy.

        `do_sample` / `repetition_penalty != 1` (behind `beam_sampling`, MYRIAD_BEAM_SAMPLING=1; NotImplementedError without it)
        are HF's beam-search multinomial sampling and its penalty under beams (tests/beam_sample_ref.py states the rule): per row
        log_softmax, the penalty on the log-probs of the ids the hypothesis generated, the EOS ban, temperature, top-k
        (max(top_k, 2), ties kept), top-p (the best two always stay), + the running score, and the item's 2 * nb candidates are
        drawn without replacement as the top 2 * nb of acc + Gumbel noise, one Philox4x32-10 stream per candidate keyed by one seed
        drawn from `generator` per call.  The step selects with mh_beam_sample_topk in place of mh_beam_topk, and
        mh_beam_seen_update carries the seen-id bitmaps to their hypotheses after the KV reorder; the workspace and the captured
        step are this path's own, and the knobs, the seed and the step counter sit in device memory.  The items select as
        before: the record is what HF's multinomial hands on.  do_sample=False with a penalty is the same step without
        temperature, cuts and noise.  An item whose tied top-k set passed the device's 1024 candidates is redone on the host for
        that step (decode_host.beam_sample_select, counted in last_generate_stats["beam_host_steps"]); with sampling, top_k
        outside 1 .. 1024 is refused (there is no host draw path under beams)."""
        B, S0, _ = inputs_embeds.shape
        nb, V = int(num_beams), self.V
        _beam_checks(nb, V)
        items = [BeamItem(nb, V, max_new_tokens, stop_ids, eos_id, length_penalty, early_stopping, num_return_sequences)
                 for _ in range(B)]                                  # their argument checks, before any launch
        pad = eos_id if pad_id is None else int(pad_id)
        R, K, NEG = B * nb, 2 * nb, BeamItem.NEG
        draw, pen = bool(do_sample), float(repetition_penalty)
        sampled = draw or pen != 1.0                                 # the step selects with mh_beam_sample_topk
        if sampled:
            if not self.beam_sampling:
                raise NotImplementedError(f"num_beams={nb} with do_sample or repetition_penalty != 1 needs the beam sampling "
                                          "switch (MYRIAD_BEAM_SAMPLING=1 or llama.beam_sampling = True)")
            inv_temp, top_k, _, _ = _sampling_args(self, draw, temperature, top_k, pen)
            if draw and not 1 <= top_k <= ops.SAMPLE_CAP:
                raise NotImplementedError(f"num_beams={nb}, do_sample=True: top_k={top_k} is outside 1..{ops.SAMPLE_CAP} "
                                          "(beam sampling draws on the device only)")
            if V < 3:
                raise ValueError(f"beam sampling needs a vocabulary of at least 3 tokens, got {V}")
            if V > 32768 or V % 4:
                raise NotImplementedError(f"beam sampling takes a vocabulary of at most 32768 tokens, a multiple of 4, got {V}")
        stats = dict(steps=0, num_beams=nb, graph_replays=0, finished_hypotheses=0, sequences_scores=None, lengths=None)
        if sampled:
            stats.update(beam_sampled_steps=0, beam_host_steps=0)
        self.last_generate_stats = stats
        stats.update(self._prepare_decode_weights(R))
        # the sampled step is another launch sequence (and `draw` is baked into it): a workspace and a graph of its own
        ws = self._decode_workspace(R, S0 + max_new_tokens, 1.0, dev_sample=sampled and draw, penalty=sampled and not draw, num_beams=nb)
        caches, T_cap, C = ws["caches"], ws["T"], 2 * self.D
        dev = self.dev

        h_ids, h_src, h_sc = _beam_upload(ws["bupd_host"])

        def feed(top_s: np.ndarray, top_i: np.ndarray) -> bool:
            """One step's record (top_s / top_i [B, K]) to every item, whose answer fills its rows of the upload; True = go on."""
            stats["steps"] += 1
            for b, item in enumerate(items):
                rows = slice(b * nb, (b + 1) * nb)
                ids, src, run, _ = item.select(top_s[b], top_i[b])
                h_ids[rows], h_src[rows], h_sc[rows] = ids, b * nb + src, run
            return beam_batch_going(items)

        if sampled:
            if "bsrec" not in ws:                                    # the record: acc [B, K] f32 | flat [B, K] | overflow flag [B]
                ws.update(bsrec=torch.zeros((2 * B * K + B,), dtype=torch.int32, device=dev),
                          part_k=torch.empty((R * K,), dtype=F32, device=dev), part_f=torch.zeros((R,), dtype=torch.int32, device=dev))
            bsrec = ws["bsrec"]
            rec_s, rec_i, rec_f = bsrec[:B * K].view(F32), bsrec[B * K:2 * B * K], bsrec[2 * B * K:]
            ws["prm"].copy_(torch.tensor([inv_temp, float(top_p), float(top_k), pen], dtype=F32))
            ws["seen"].zero_()                                       # generated ids only: the prompt is embeddings
            seed = int(torch.randint(0, 2**63 - 1, (1,), generator=generator)) if draw else 0
            ws["seed"].fill_(seed)
            ws["step"].zero_()

            def sample_topk(logits, ban, t_add, step=None, **adv):
                ops.beam_sample_topk(logits, ws["bscore"], ws["part_k"], ws["part_s"], ws["part_i"], ws["part_f"], rec_s, rec_i, rec_f,
                                     B, nb, ban_id=ban, draw=draw, params=ws["prm"], seed=ws["seed"], seen=ws["seen"], step=step,
                                     t_add=t_add, **adv)

            def read_sampled(logits_of, ban):                        # the sampled step's record, the items' flags behind it
                rec = bsrec.cpu()
                top_s, top_i = rec[:B * K].view(F32).numpy().reshape(B, K).copy(), rec[B * K:2 * B * K].numpy().reshape(B, K).astype(np.int64)
                stats["beam_sampled_steps"] += 1
                for b in np.nonzero(rec[2 * B * K:].numpy())[0]:     # a tied top-k set past the device's cap: the host's rule
                    t = stats["steps"]                               # tokens generated so far = the index of this one
                    acc, flat, _ = beam_sample_select(logits_of()[b * nb:(b + 1) * nb].cpu().numpy(), h_sc[b * nb:(b + 1) * nb],
                                                      items[b].run_seqs, ban, inv_temp, top_k, float(top_p), pen, seed, t, int(b), draw)
                    top_s[b], top_i[b] = acc, flat
                    stats["beam_host_steps"] += 1
                return top_s, top_i

        # ---- prefill at B rows into rows b * nb, then broadcast the prompt's keys / values to the other beams
        logits0 = self._prefill(inputs_embeds, [c[::nb] for c in caches])
        ban0 = eos_id if 0 < min_length else -1
        if sampled:                                                  # the prompt's row nb times, HF's initial scores (0, -1e9, ...)
            logits0 = logits0.repeat_interleave(nb, 0)
            h_sc[:] = NEG
            h_sc[::nb] = 0.0
            ws["bscore"].copy_(torch.from_numpy(h_sc))
            sample_topk(logits0, ban0, 0)
        else:
            ws["bscore"].zero_()                                     # beam 0's running score; one row per item here
            ops.beam_topk(logits0, ws["bscore"], ws["part_s"], ws["part_i"], ws["brec"][0].view(F32), ws["brec"][1], B, nb,
                          ban_id=ban0)
        if self.layers:
            # a range of its own: ws["lo"] holds the previous call's S0 when the workspace is reused
            bsrc = torch.arange(B, dtype=torch.int32).repeat_interleave(nb).mul_(nb).to(dev)
            span = torch.tensor([0, S0], dtype=torch.int32).to(dev)
            ops.beam_reorder_kv(ws["table"], len(caches), B, nb, T_cap, C, bsrc, span[:1], span[1:])
        going = feed(*(read_sampled(lambda: logits0, ban0) if sampled else _beam_record(ws["brec"], B)))

        # ---- token steps
        ws["pos"].fill_(S0)
        ws["kvlen"].fill_(S0 + 1)
        ws["lo"].fill_(S0)                                           # the prompt prefix is the same in every beam of an item

        def token_step(ban):
            ops.beam_reorder_kv(ws["table"], len(caches), B, nb, T_cap, C, ws["src"], ws["lo"], ws["pos"])
            if sampled:                                              # the bitmaps follow their hypotheses; the fed token joins
                ops.beam_seen_update(ws["seen"], ws["src"], ws["ids"], B, nb, V)
                self._step_logits(ws)
                sample_topk(ws["logits"], ban, 1, step=ws["step"], pos=ws["pos"], kvlen=ws["kvlen"])   # token s draws Philox step s
                return
            self._step_logits(ws)
            ops.beam_topk(ws["logits"], ws["bscore"], ws["part_s"], ws["part_i"], ws["brec"][0].view(F32), ws["brec"][1], B, nb,
                          ban_id=ban, pos=ws["pos"], kvlen=ws["kvlen"])

        gen = 1                                                      # tokens generated so far
        while going:
            ws["bupd"].copy_(ws["bupd_host"], non_blocking=True)    # ids | src | running scores: one host->device copy
            ban = eos_id if gen < min_length else -1
            self._launch_step(ws, token_step, ban, use_graph, stats)
            gen += 1
            going = feed(*(read_sampled(lambda: ws["logits"], ban) if sampled else _beam_record(ws["brec"], B)))

        results = [item.result() for item in items]
        seqs = [q for qs, _ in results for q in qs]
        scores = torch.from_numpy(np.concatenate([sc for _, sc in results]))
        stats.update(sequences_scores=scores, finished_hypotheses=sum(item.finished for item in items), lengths=[len(q) for q in seqs])
        ids = _pad_ids(seqs, pad)
        return (ids, scores) if return_scores else ids

    def slot_decoder(self, slots: int, capacity: int, split_kv: Optional[bool] = False) -> "SlotDecoder":
        """A decode-slot engine over this model: `slots` rows of one captured token step, each decoding its own request of up to
        `capacity` positions (prompt + generated).  `split_kv`: the step's attention kernel (False: the single-workgroup rows
        kernel, True: the split-KV rows kernel, None: split_kv_rows_rule per call).  See SlotDecoder."""
        return SlotDecoder(self, slots, capacity, split_kv=split_kv)


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
        self.bufs = self.B = self.stamp = None
        self.keys: List[list] = []
        self.views = {}                                              # cfg -> workspace view of bufs, with its graph / warm flag
        self.graph_captures = 0
        self.split = False
        self.last_stats = {}

    def _begin_turn(self, keys, version, reason, B: int, S0: int, max_new_tokens: int, inv_temp: float, dev_sample: bool,
                    penalty: bool, scores: bool = False, draft_k: int = 0):
        """A turn's setup, once the decode weights are packed: invalidation, (re)allocation, the reused prefix.  `draft_k`: the
        rows of a draft turn's verify step, which the capacity and the rotary table must hold past the last fed position.
        Returns (workspace, past).  `scores`: the turn's step writes the token scores -- a view (and graph) of its own, whose key
        carries one more item, so the views of turns without scores are the ones they were."""
        L = self.llama
        if S0 + max_new_tokens + draft_k > L.cos.shape[0]:
            raise ValueError(f"context {S0} + max_new_tokens {max_new_tokens}{f' + draft_k {draft_k}' if draft_k else ''} passes the "
                             f"rotary table ({L.cos.shape[0]} positions)")
        if len(keys) != B or any(len(k) != S0 for k in keys):
            raise ValueError("one key per context position and batch row is required")
        stamp = _cache_stamp(L, version)
        need = S0 + max_new_tokens + 2 + draft_k
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
        cfg = (None if dev_sample else float(inv_temp), bool(dev_sample), bool(penalty), self.split) + (("scores",) if scores else ())
        if cfg not in self.views:
            self.views[cfg] = _buffer_view(L, self.bufs, self.split, scores)
        self.last_stats = dict(context_tokens=S0, reused_tokens=past, prefilled_tokens=S0 - past, split_kv=bool(self.split),
                               full_reprefill_reason=reason)
        return self.views[cfg], past

    @torch.no_grad()
    def generate(self, inputs_embeds: torch.Tensor, keys, weights_version=None, reset_reason: Optional[str] = None,
                 max_new_tokens: int = 90, **kw):
        """One turn: greedy_generate's contract and arguments (`max_new_tokens`, `stop_ids`, `eos_id`, `min_length`, `do_sample`,
        `top_p`, `temperature`, `generator`, `top_k`, `repetition_penalty`, `return_margins`, `return_scores`, `watch_ids`, `draft`, `draft_k`) on
        [B, S0, D] f32 embeddings whose
        positions are named by `keys` ([B][S0]).  `weights_version`: anything that changes when the weights do."""
        L = self.llama
        B, S0, _ = inputs_embeds.shape
        ws = None
        try:
            inv_temp, _, dev_sample, penalty = _sampling_args(L, **kw)
            scores = bool(kw.get("return_scores", False))
            ops.score_watch_ids(kw.get("watch_ids", ()) if scores else (), L.V)
            draft_k = 0 if kw.get("draft") is None else _draft_refusals(B, dev_sample, penalty, scores, kw.get("draft_k", 4),
                                                                                L.draft_sampling)
            weight_stats = L._prepare_decode_weights(B)              # packed before the stamp, which names the packed copies
            ws, past = self._begin_turn([list(k) for k in keys], weights_version, reset_reason, B, S0, max_new_tokens, inv_temp,
                                        dev_sample, penalty, scores, draft_k)
            graph = ws["graph"]
            out = L._greedy_core(inputs_embeds, ws, past, weight_stats, max_new_tokens=max_new_tokens, use_graph=True, **kw)
        except BaseException:
            self.keys = [[] for _ in range(B)]                       # the cache may be half written
            raise
        finally:
            if ws is not None and ws["graph"] is not graph:          # this turn captured its view's step
                self.graph_captures += 1
        ids = out[0] if isinstance(out, tuple) else out
        eos = int(kw.get("eos_id", 2))
        new_keys = []
        for r in range(B):
            row, fed, live = ids[r].tolist(), [], True
            for k in range(len(row) - 1):                                  # token step k + 1 fed pick k at position S0 + k
                fed.append(("t", row[k]) if live else ("x",))
                live = live and row[k] != eos
            new_keys.append(list(keys[r]) + fed)
        self.keys = new_keys
        st = self.llama.last_generate_stats
        self.last_stats.update(steps=st["steps"], graph_replays=st["graph_replays"], graph_captures=self.graph_captures)
        if "draft_k" in st:                                          # a draft turn: a split-KV view decodes with plain steps
            self.last_stats.update({k: st[k] for k in ("draft_k", "draft_off", "verify_steps", "plain_steps", "draft_proposed",
                                                       "draft_accepted")})
        return out


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
    at row 0, so it drops what the sessions had cached.

    Beam search (opt-in, `run(num_beams=nb > 1)` behind `LlamaHIP.slot_beams`, MYRIAD_SLOT_BEAMS=1): the slots form G = slots / nb
    groups of nb rows and a group holds one request's search (decode_host.BeamItem, beam_generate's rule per request), refilled
    as soon as that request ends.  The captured step is beam_generate's with per-group state: mh_beam_reorder_kv_items over each
    group's [lo, pos), the slot step's layers and lm-head under a per-row live mask, mh_beam_topk_items (each group's EOS ban
    from its own gen).  One view and one graph per nb, in `beam_views`: no key of `views` changes.  With `LlamaHIP.beam_sampling`
    on as well, `do_sample` / `repetition_penalty` != 1 run beam_generate's sampled step per group -- mh_beam_seen_update_items
    and mh_beam_sample_topk_items, every group with its own seed and Philox step in device memory -- in a view and a graph of
    its own beside the deterministic one.  See _run_beams.

    Draft-and-verify decoding (opt-in, `run(draft=drafter, draft_k=K)` behind `LlamaHIP.slot_draft`, MYRIAD_SLOT_DRAFT=1; slots *
    K <= GEMV_WIDE_MAX_ROWS): a verify view of the
    buffers in `draft_views` (_draft_workspace, its own graph) runs the token step at slots * K rows, K consecutive tokens per
    slot -- mh_attn_decode_rope_draft_rows, mh_argmax_pmax_rows, mh_draft_accept_rows -- whenever a live slot has a guess, and
    the plain step otherwise; a request's ids and margins are exactly those of the run without `draft`.  No key of `views`
    changes.  Behind `LlamaHIP.draft_sampling` (MYRIAD_DRAFT_SAMPLING=1) the verify step also runs the per-row tail and the
    token scores (mh_repetition_penalty_draft_rows, mh_sample_rows_draft, mh_token_scores_rows, mh_draft_accept_sampled_rows)
    on `seen`, `gen` and `seed` shared with the plain step.  See `run`."""

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
        self.beam_views = {}                                         # (num_beams, split[, draw]) -> the beam step's view (_beam_workspace)
        self.draft_views = {}                                        # (draft_k, inv_temp) -> the verify step's view (_draft_workspace)
        self.ws = None                                               # the view of the current / last run
        self._weights = None
        self.graph_captures = 0
        self.last_stats = {}
        self.sessions = SessionTable(slots)                          # run_turns: which conversation each slot's cache holds

    def close(self, session) -> None:
        """Free the slot of a run_turns session."""
        self.sessions.close(session)

    @staticmethod
    def _view_key(inv_temp: float, rows_tail=None, split: bool = False, scores: bool = False):
        """The key of a view (one captured graph each).  Without split-KV it is what it was before the engine had the choice --
        inv_temp, or (inv_temp or None, device-sampled, penalty) for the per-row tail -- and a split view is ("split", that).  A
        view whose step writes the token scores wraps the first of those in ("scores", ...): every other key is what it was."""
        key = float(inv_temp)
        if rows_tail is not None:
            key = (None if rows_tail[0] else key, bool(rows_tail[0]), bool(rows_tail[1]))
        if scores:
            key = ("scores", key)
        return ("split", key) if split else key

    def _base_buffers(self) -> dict:
        """The step's buffers, shared by every view and kept while the decode weights stay the ones the captured graphs read."""
        L = self.llama
        L._prepare_decode_weights(self.slots, ops.GEMV_WIDE_MAX_ROWS)
        if not (_packed_step(L, self.slots, ops.GEMV_WIDE_MAX_ROWS) and L.decode_fused):
            raise ValueError("the slot engine needs the fused packed token step (MYRIAD_PACK_DECODE and MYRIAD_DECODE_FUSED on)")
        wid = _decode_weights_id(L)
        if self.bufs is None or self._weights != wid:
            self.bufs, self.views, self.beam_views, self.draft_views, self.ws = None, {}, {}, {}, None
            # its row limit: above GEMV_MAX_ROWS slots the step stays on the packed copies
            self.bufs = _decode_buffers(L, self.slots, self.T_cap, row_limit=ops.GEMV_WIDE_MAX_ROWS)
            self.bufs["live"] = torch.zeros((self.slots,), dtype=torch.int32, device=L.dev)
            self._weights = wid
        return self.bufs

    def _beam_workspace(self, nb: int, split: bool, draw: Optional[bool] = None) -> dict:
        """The beam step's view of the buffers for groups of nb rows, with its own graph: the beam step's buffers (_beam_buffers)
        and the per-group state mh_beam_topk_items / mh_beam_reorder_kv_items read -- `lo`, `hi`, `gen`, `glive` [G] and `bprm` =
        (min_length, eos_id) -- next to the per-row `pos` / `kvlen` / `live` every view shares.  `rec0` and `zero` serve the
        refills' first selection, `bsrc` (every row's group's first row) the prompt broadcast.

        `draw` = True / False asks for the sampled beam step's view (mh_beam_sample_topk_items with or without the draw, which is
        baked into the launch), keyed (nb, split, draw) beside the deterministic step's (nb, split): on top of the above it holds
        the seen-id bitmaps `bseen` [slots, ceil(V / 32)], the groups' seeds `bseed` [G], the knobs `bsprm` (inv_temp, top_p,
        top_k, penalty), the (acc | flat | flag) record `bsrec`, the scratch `part_k` / `part_f`, and for the refills' first
        selection `rec0s`, `seed0`, `gen0` (zeros), `live1` (ones) and `score0` (HF's initial scores 0, -1e9, ... per group)."""
        L, bufs = self.llama, self._base_buffers()
        key = (int(nb), bool(split)) if draw is None else (int(nb), bool(split), bool(draw))
        if key not in self.beam_views:
            dev, i32, G, K = L.dev, torch.int32, self.slots // nb, 2 * nb
            view = _buffer_view(L, bufs, split)
            view.update(_beam_buffers(L, bufs["caches"], self.slots, nb), rec0=torch.zeros((2, G * K), dtype=i32, device=dev),
                        zero=torch.zeros((G,), dtype=F32, device=dev), bprm=torch.zeros((2,), dtype=i32, device=dev),
                        bsrc=torch.arange(G, dtype=i32).repeat_interleave(nb).mul_(nb).to(dev),
                        **{k: torch.zeros((G,), dtype=i32, device=dev) for k in ("lo", "hi", "gen", "glive")})
            if draw is not None:
                score0 = torch.full((G, nb), float(BeamItem.NEG), dtype=F32)
                score0[:, 0] = 0.0
                view.update(bseen=torch.zeros((self.slots, (L.V + 31) // 32), dtype=i32, device=dev),
                            bseed=torch.zeros((G,), dtype=torch.long, device=dev), seed0=torch.zeros((G,), dtype=torch.long, device=dev),
                            bsprm=torch.zeros((4,), dtype=F32, device=dev), bsrec=torch.zeros((2 * G * K + G,), dtype=i32, device=dev),
                            rec0s=torch.zeros((2 * G * K + G,), dtype=i32, device=dev),
                            part_k=torch.empty((self.slots * K,), dtype=F32, device=dev),
                            part_f=torch.zeros((self.slots,), dtype=i32, device=dev), gen0=torch.zeros((G,), dtype=i32, device=dev),
                            live1=torch.ones((G,), dtype=i32, device=dev), score0=score0.reshape(-1).to(dev))
            self.beam_views[key] = view
        self.ws = self.beam_views[key]
        return self.ws

    def _workspace(self, inv_temp: float, rows_tail=None, split: bool = False, scores: bool = False) -> dict:
        """The step's buffers, kept while the decode weights stay the ones the captured graphs read, and over them one view (its
        own graph / warm flag) per inv_temp: the arg-max kernel takes inv_temp as a launch argument, so a captured step is fixed
        to one value (LlamaHIP._decode_workspace keys its workspaces the same way).  `rows_tail` = (device-sampled, penalty) asks
        for the step with the per-row tail: its buffers join on first use (the knobs `prm`, per-slot `seed` / `gen` / `kept` /
        `seen`, and `seed0` / `gen0` for the refills' first picks), and a device-sampled view is keyed without inv_temp, which the
        sampler reads from `prm`.  `split`: the view's step runs the split-KV rows kernel; the partials buffer joins on first use,
        a split view holds it and a non-split view holds None, so each (key, split) has its own graph.  `scores`: the view's step
        also writes the token scores into a record of its own (_score_buffers; `sc0` takes the refills' first picks' scores)."""
        L = self.llama
        self._base_buffers()
        if rows_tail is not None and "prm" not in self.bufs:
            n, i32 = self.slots, torch.int32
            self.bufs.update(prm=torch.zeros((6,), dtype=F32, device=L.dev), seed=torch.zeros((n,), dtype=torch.long, device=L.dev),
                             seed0=torch.zeros((n,), dtype=torch.long, device=L.dev), gen=torch.zeros((n,), dtype=i32, device=L.dev),
                             gen0=torch.zeros((n,), dtype=i32, device=L.dev), kept=torch.zeros((n,), dtype=i32, device=L.dev),
                             seen=torch.zeros((n, (L.V + 31) // 32), dtype=i32, device=L.dev))
        if scores and "sc0" not in self.bufs:
            self.bufs["sc0"] = torch.zeros((ops.SCORE_ROWS, self.slots), dtype=F32, device=L.dev)
        key = self._view_key(inv_temp, rows_tail, split, scores)
        if key not in self.views:
            same = [k for k in self.views if (isinstance(k, tuple) and k[0] == "split") == bool(split)]
            if len(same) >= 4:                                       # a few temperatures at most per kernel: drop its oldest graph
                self.views.pop(same[0])
            self.views[key] = _buffer_view(L, self.bufs, split, scores)
        self.ws = self.views[key]
        return self.ws

    def _draft_workspace(self, K: int, inv_temp: float, tail=None, split: bool = False) -> dict:
        """The verify step's view of the buffers (run(draft=...)): slots x K rows, K consecutive tokens per slot, with a graph of
        its own, one per (K, inv_temp) -- the arg-max launch bakes inv_temp in.  It shares the caches, `pos`, `kvlen`, `live`,
        `step` and the plain step's fed ids (`next_ids`, what mh_draft_accept_rows also writes its kept pick to) with the plain
        views, so the host switches between the two steps from one launch to the next.  Its own: the fed ids `ids` [slots * K]
        (per slot the last token, its real guesses, id 0 as filler), `x_in`, `logits`, `nxt` / `mar` / `pmx`, the counts `cnt`
        [2, slots] = (`nguess`, `nrow`), the [slots, 3K + 1] record `drec` and the device float `top_p`.  No key of `views`
        changes.

        `tail` = (device-sampled, penalty, rows_tail, scores), behind `draft_sampling`: the view of the verify step with the
        per-row tail (_SlotRun.verify_token_step), keyed (K, inv_temp) + tail beside the plain verify view's (K, inv_temp).  It
        reads the `prm`, `seed`, `gen`, `seen` and `watch` the call's plain view already put into the set (without the per-row
        tail `gen` is a counter nobody reads), holds `kept` [slots * K], and its record `drec` is one flat buffer -- slots x (4K
        + 1) floats of mh_draft_accept_sampled_rows (`arec`), then with scores SCORE_ROWS rows of slots * K floats (`sc`) -- so
        the step still makes one device->host copy.

        `split` (behind `draft_split`, for a call on the split-KV view): the verify step's attention is
        ops.attn_decode_rope_split_draft_rows and the view holds its partials `split_draft`; keyed ("split",) + the above."""
        L, bufs = self.llama, self._base_buffers()
        key = (("split",) if split else ()) + (int(K), float(inv_temp)) + (() if tail is None else tuple(bool(t) for t in tail))
        if key not in self.draft_views:
            if len(self.draft_views) >= 4:                           # a few (K, temperature) pairs at most: drop the oldest graph
                self.draft_views.pop(next(iter(self.draft_views)))
            dev, R = L.dev, self.slots * int(K)
            cnt = torch.zeros((2, self.slots), dtype=torch.int32, device=dev)
            view = _buffer_view(L, bufs, False)
            view.update(draft_k=int(K), next_ids=bufs["ids"], ids=torch.zeros((R,), dtype=torch.long, device=dev),
                        x_in=torch.empty((R, L.D), dtype=F32, device=dev), logits=torch.empty((R, L.V), dtype=F32, device=dev),
                        nxt=torch.empty((R,), dtype=torch.long, device=dev), mar=torch.empty((R,), dtype=F32, device=dev),
                        pmx=torch.empty((R,), dtype=F32, device=dev), cnt=cnt, nguess=cnt[0], nrow=cnt[1],
                        drec=torch.zeros((self.slots, 3 * int(K) + 1), dtype=F32, device=dev),
                        top_p=torch.zeros((1,), dtype=F32, device=dev),
                        split_draft=ops.attn_decode_split_draft_ws(self.slots, int(K), L.H, bufs["T"], dev) if split else None)
            if tail is not None:
                n_acc = self.slots * (4 * int(K) + 1)
                drec = torch.zeros((n_acc + (ops.SCORE_ROWS * R if tail[3] else 0),), dtype=F32, device=dev)
                view.update(kept=torch.zeros((R,), dtype=torch.int32, device=dev), drec=drec, arec=drec[:n_acc],
                            sc=drec[n_acc:].view(ops.SCORE_ROWS, R) if tail[3] else None)
                if not tail[2]:
                    view["gen"] = torch.zeros((self.slots,), dtype=torch.int32, device=dev)
            self.draft_views[key] = view
        return self.draft_views[key]

    @torch.no_grad()
    def run(self, requests, max_new_tokens: int = 90, stop_ids=((835,), (2277, 29937)), eos_id: int = 2, min_length: int = 1,
            do_sample: bool = False, top_p: float = 1.0, temperature: float = 1.0, top_k: int = 50,
            generator: Optional[torch.Generator] = None, ordered: bool = False, prefill_batch: int = 1, refill_min: int = 1,
            prefill_rows: int = 2048, repetition_penalty: float = 1.0, seeds=None, return_scores: bool = False, watch_ids=(),
            num_beams: int = 1, length_penalty: float = 1.0, early_stopping=False, num_return_sequences: int = 1,
            pad_id: Optional[int] = None, draft=None, draft_k: int = 4):
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
        `slots` live rows and a longest context of 0 -- the lengths are not known up front -- so None never splits here.

        `return_scores`, `watch_ids` (greedy_generate's; a view and a graph of their own): every yielded tuple gains a fourth
        item, dict(token_logprobs [L_i] f32, watch_logprobs [L_i, W] f32) of that request -- what greedy_generate returns for it
        alone.

        `num_beams` = nb > 1 (behind `slot_beams`; with `length_penalty`, `early_stopping`, `num_return_sequences`, `pad_id`,
        beam_generate's): beam search, one request per group of nb slots (_run_beams).  The run then yields (index, ids [nrs, Lmax]
        right-padded with pad_id, sequence scores [nrs] f32, lengths [nrs]) per request -- what beam_generate returns for it
        alone -- and `last_stats` gains `num_beams`, `groups`, `finished_hypotheses`; `occupancy` counts groups.  With
        `beam_sampling` on as well, `do_sample` (with `temperature`, `top_k` in 1..1024, `top_p`) and `repetition_penalty` != 1 are
        beam_generate's beam sampling and penalty per request: request i draws from the i-th seed of `generator` or `seeds`, what
        beam_generate draws for it alone with that seed (`beam_sampled_steps`, `beam_host_steps` join `last_stats`).

        `draft` (behind `slot_draft`, MYRIAD_SLOT_DRAFT=1, off by default: NotImplementedError without it; a drafter with
        `propose`, decode_host.NgramDrafter) with `draft_k` = K rows per slot, slots * K <=
        GEMV_WIDE_MAX_ROWS: draft-and-verify decoding in the slots.  Before every step each live slot gets up to K - 1 guesses
        (decode_host.slot_guesses: never past the last token the request can still emit); the step is the VERIFY step iff at least
        one live slot has a real guess, else the plain one-row-per-slot step.  The verify step (_draft_workspace, a graph of its
        own) is the token step at slots * K rows with mh_attn_decode_rope_draft_rows (slot g's rows at pos[g] .. pos[g] + nrow[g] -
        1), mh_argmax_pmax_rows and mh_draft_accept_rows, which keeps per slot the guesses the picks confirm plus the one token the
        last of them produces, feeds that one to both steps and moves pos / kvlen.  Every row has the bits of the plain step at its
        position, so a request's ids and margins are exactly those of the run without `draft`, whatever the drafter proposes.  Per
        verify step the host makes two small host->device copies (the fed ids and guesses; the counts) and one device->host copy
        (the record); a plain step after it needs none.  Under do_sample a row with p_max < top_p ends its window on the device
        and is drawn on the host from its row of the verify logits.  K = 1 runs plain steps only; so does a call on the split-KV
        view (unless `draft_split`, MYRIAD_DRAFT_SPLIT=1, is on: then its verify step runs mh_attn_decode_rope_split_draft_rows) or
        with a shape the verify step's attention launch refuses, and `last_stats["draft_off"]` says "split_kv" / "unsupported".
        `last_stats` gains draft_k, draft_off, verify_steps, plain_steps, draft_proposed, draft_accepted, emitted,
        verify_graph_replays and plain_graph_replays.  The caller teaches the drafter.  NotImplementedError with num_beams > 1
        and -- unless `draft_sampling` (MYRIAD_DRAFT_SAMPLING=1, off by default) is on -- with device sampling, repetition_penalty
        != 1, min_length > 1 and return_scores; ValueError for K outside 1 .. DRAFT_MAX_K or slots * K above GEMV_WIDE_MAX_ROWS.

        With `draft_sampling` on, those four run in the verify step too (a view and a graph of their own; a call without them
        replays the graphs it always did): after the layers, mh_repetition_penalty_draft_rows (row j of slot g is penalised on
        seen[g] plus the ids fed in its rows 0 .. j), mh_sample_rows_draft (row j draws Philox step gen[g] + j of seed[g] and bans
        EOS iff gen[g] + j < min_length; without the device sampler the same launch picks the arg-max), mh_token_scores_rows over
        the slots * K rows into the step's record, and mh_draft_accept_sampled_rows, which ends a window at a row the host must
        draw (kept < 0, or p_max < top_p on the host-draw path), adds the tokens that stood to seen[g] and moves gen[g].  A draw
        depends on (logits row, seed, token index) only, so a guess stands iff it equals the draw: ids, margins, sampled-row
        counts and scores are bit for bit those of the run without `draft`.  Both graphs share seen, gen, seed, the caches and
        the counters; a row the host must draw is drawn as the plain step draws that token of that request."""
        self.sessions.clear()                                        # the slots' caches are overwritten from row 0
        if draft is not None and int(num_beams) != 1:
            raise NotImplementedError(f"decode slots: draft decoding with num_beams={num_beams} is not implemented")
        if int(num_beams) != 1:
            yield from self._run_beams(requests, int(num_beams), max_new_tokens, stop_ids, eos_id, min_length, ordered, prefill_batch,
                                       refill_min, prefill_rows, length_penalty, early_stopping, num_return_sequences, pad_id,
                                       refused=dict(do_sample=bool(do_sample), repetition_penalty=float(repetition_penalty) != 1.0,
                                                    return_scores=bool(return_scores), seeds=seeds is not None),
                                       sampling=dict(do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p,
                                                     repetition_penalty=repetition_penalty, generator=generator, seeds=seeds))
            return
        yield from self._run(requests, None, None, max_new_tokens, stop_ids, eos_id, min_length, do_sample, top_p, temperature,
                             top_k, generator, ordered, prefill_batch, refill_min, prefill_rows, repetition_penalty, seeds,
                             return_scores, watch_ids, draft, draft_k)

    def run_turns(self, turns, weights_version=None, **kw):
        """One turn each of several conversations, every one in ITS OWN slot on top of what that slot's cache holds of it
        (`sessions`, a SessionTable).  `turns` = [(session, emb [S0, D] f32, keys [S0])] or with a fourth item `reset_reason`; at
        most one turn per session per call (ValueError), at most `slots` open sessions (`close(session)` frees one).  `kw` are
        `run`'s arguments but `refill_min` (prefill_batch, prefill_rows, the sampling knobs, repetition_penalty, min_length,
        seeds: with device sampling the i-th turn of the call takes the i-th seed; return_scores, watch_ids: the yielded tuples
        gain the scores dict).  Only the rows past the prefix the slot shares with the new context are prefilled: with
        prefill_batch = 1 a solo _prefill(emb, slot cache, past) per turn,
        otherwise passes of up to prefill_batch turns / prefill_rows new rows through _prefill_packed(..., pasts).  Then `run`'s
        captured step (same graphs and views) runs until every turn has stopped under its own stop rule.  Yields (session, ids,
        margins) as `run` does, `ordered=True` in the list's order; `last_stats["turns"]` holds per turn `context_tokens`,
        `reused_tokens`, `prefilled_tokens` and `full_reprefill_reason`.  `weights_version`: anything that changes when the
        weights do; with it, a change of the decode weights or a `run()` on this decoder drops every session's cached rows.  The
        step's attention kernel is the decoder's `split_kv` choice, made once per call (`last_stats["split_kv"]`): with None,
        split_kv_rows_rule(turns in the call, heads, the longest context at admission).
        `draft` / `draft_k` (behind `slot_draft` and `draft_split`; NotImplementedError without them): `run`'s draft-and-verify
        loop on the turns.  A window is clamped so that no row is fed past context + max_new_tokens - 1 (slot_guesses), and a
        session records the context plus the ids that stood: the cache rows of rejected guesses lie past the recorded keys, where
        the next turn's prefill or verify step overwrites them."""
        turns = [tuple(t) for t in turns]
        if "refill_min" in kw:
            raise ValueError("run_turns: refill_min does not apply, every turn has its own slot")
        if kw.get("draft") is not None and not getattr(self.llama, "draft_split", False):
            raise NotImplementedError("run_turns: draft decoding with run_turns / ChatPool is not implemented (it runs in `run`) "
                                      "without its switch (MYRIAD_DRAFT_SPLIT=1 or llama.draft_split = True)")
        if kw.get("draft") is None:
            kw.pop("draft", None), kw.pop("draft_k", None)
        if int(kw.pop("num_beams", 1) or 1) != 1:
            raise NotImplementedError("run_turns: beam search runs in `run` only (a conversation would have to carry the winning "
                                      "hypothesis's cache rows into its next turn)")
        for t in turns:
            if len(t) not in (3, 4) or t[1].dim() != 2 or len(t[2]) != t[1].shape[0]:
                raise ValueError("run_turns: a turn is (session, emb [S0, D], keys [S0]) or (session, emb, keys, reset_reason)")
        keys = [SessionTable._key(t[0]) for t in turns]
        if len(set(keys)) != len(keys):
            raise ValueError("run_turns: at most one turn per session in one call")
        return self._run(None, turns, weights_version, **kw)

    def beam_args(self, nb: int, refused=None) -> int:
        """The checks of run(num_beams = nb > 1) that need no request; returns the group count.  `refused`: the arguments in use
        that the beam groups do not take; with the beam sampling switch on, do_sample, repetition_penalty and seeds leave it
        (_beam_sampling_args checks them)."""
        L = self.llama
        _beam_checks(nb, L.V)
        if not getattr(L, "slot_beams", False):
            raise NotImplementedError(f"decode slots: num_beams={nb} needs the slot beams switch (MYRIAD_SLOT_BEAMS=1 or "
                                      "llama.slot_beams = True)")
        if self.slots % nb:
            raise ValueError(f"slots={self.slots} do not divide into groups of num_beams={nb} rows")
        if getattr(L, "beam_sampling", False):
            refused = {k: v for k, v in (refused or {}).items() if k not in ("do_sample", "repetition_penalty", "seeds")}
        for name, on in (refused or {}).items():
            if on:
                raise NotImplementedError(f"decode slots: num_beams={nb} with {name} is not implemented (beam sampling, the penalty "
                                          "and token scores under beams are beam_generate's)")
        return self.slots // nb

    def _beam_sampling_args(self, nb: int, sampling):
        """run(num_beams = nb > 1)'s sampling arguments, checked as beam_generate checks them (beam_args has refused them with the
        beam sampling switch off): ((inv_temp, top_k, top_p, penalty) when the step is the sampled one -- do_sample or a penalty --
        else None, draw)."""
        L, a = self.llama, sampling or {}
        draw, pen = bool(a.get("do_sample", False)), float(a.get("repetition_penalty", 1.0))
        if not getattr(L, "beam_sampling", False):
            return None, False
        inv_temp, top_k, _, _ = _sampling_args(L, draw, a.get("temperature", 1.0), a.get("top_k", 50), pen)
        if a.get("seeds") is not None and not draw:
            raise ValueError("seeds= names the beam groups' per-request streams: it needs do_sample")
        if not draw and pen == 1.0:
            return None, False
        if draw and not 1 <= top_k <= ops.SAMPLE_CAP:
            raise NotImplementedError(f"decode slots: num_beams={nb}, do_sample=True: top_k={top_k} is outside 1..{ops.SAMPLE_CAP} "
                                      "(beam sampling draws on the device only)")
        if L.V < 3:
            raise ValueError(f"beam sampling needs a vocabulary of at least 3 tokens, got {L.V}")
        if L.V > 32768 or L.V % 4:
            raise NotImplementedError(f"beam sampling takes a vocabulary of at most 32768 tokens, a multiple of 4, got {L.V}")
        return (inv_temp, top_k, float(a.get("top_p", 1.0)), pen), draw

    @torch.no_grad()
    def _run_beams(self, requests, nb, max_new_tokens, stop_ids, eos_id, min_length, ordered, prefill_batch, refill_min, prefill_rows,
                   length_penalty, early_stopping, num_return_sequences, pad_id, refused=None, sampling=None):
        """run(num_beams = nb > 1): the slot loop over G groups of nb rows (BeamSlotScheduler, driven by RefillPlanner unchanged).

        The captured step: hi = pos of each group's first row (one strided copy), mh_beam_reorder_kv_items over [lo, hi) by the
        parent rows, the slot view's _step_logits under the per-row live mask (nb equal entries per group), mh_beam_topk_items.
        Between two replays the host reads the [2, G, K] record with one copy and uploads (ids, src, running scores) of all rows
        with one copy, as beam_generate does; beside that it writes a finished group's live flags and a refilled group's state.
        min_length and eos_id sit in device memory, length_penalty / early_stopping / num_return_sequences on the host: a run
        with other values replays the same graph.

        A refill -- solo into cache row g * nb, or packed through _prefill_packed -- is: the prefill, ONE eager mh_beam_topk at
        rpi = 1 over the refilled prompts' logits, BeamItem's first selection, one eager mh_beam_reorder_kv_items that broadcasts
        the prompts' rows [0, S0_g) to the groups' sibling rows, then pos = S0, kvlen = S0 + 1, lo = S0, gen = 1, live = 1.

        `sampling` (run's do_sample, temperature, top_k, top_p, repetition_penalty, generator, seeds) with do_sample or a penalty
        and the beam sampling switch on: beam_generate's sampled step per group, in a view and a graph of its own.  The captured
        step is then hi, mh_beam_reorder_kv_items, mh_beam_seen_update_items (the bitmaps follow their hypotheses, the fed token
        joins them), _step_logits, mh_beam_sample_topk_items with t_add = 0 -- gen[g] is the index of the token being picked, so
        group g draws Philox step gen[g] of its own seed[g] with the counter's item field 0: what beam_generate draws for the
        request alone.  A refill's first selection is ONE eager mh_beam_sample_topk_items over the prompts' rows repeated nb
        times under HF's initial scores (0, -1e9, ...) with gen = 0, every request's own seed and no advance; going live also
        clears the group's bitmap rows and writes seed[g].  Seeds travel with the requests (seeded_requests).  A group whose
        overflow flag is set (a tied top-k set past the device's 1024 candidates) is redone on the host for that selection
        (decode_host.beam_sample_select with the group's seed, its t and item = 0), counted in last_stats["beam_host_steps"];
        "beam_sampled_steps" counts the sampled token steps.  The knobs sit in device memory: one graph per (nb, split, draw)."""
        L = self.llama
        G = self.beam_args(nb, refused)
        V, i32 = L.V, torch.int32
        sampled, draw = self._beam_sampling_args(nb, sampling)
        pad = int(eos_id) if pad_id is None else int(pad_id)

        def make_item():
            return BeamItem(nb, V, max_new_tokens, stop_ids, eos_id, length_penalty, early_stopping, num_return_sequences)

        make_item()                                                  # its argument checks, before any launch
        split = self.split_kv
        if split is None:
            split = split_kv_rows_rule(self.slots, L.H, 0)
        ws = self._beam_workspace(nb, split, draw if sampled else None)
        sched = BeamSlotScheduler(G, make_item, ordered=ordered)
        # a request travels with the seed of its own stream (None unless the groups draw)
        reqs = seeded_requests(requests, sampling["generator"], sampling["seeds"]) if draw else ((emb, None) for emb in requests)
        plan = RefillPlanner(sched, reqs, prefill_batch, prefill_rows, refill_min, length=lambda q: int(q[0].shape[0]))
        packed = int(prefill_batch) != 1 or int(refill_min) != 1
        stats = dict(steps=0, graph_replays=0, graph_captures=self.graph_captures, prefills=0, live_row_steps=0, occupancy=0.0,
                     prefill_passes=0, packed_rows=0, split_kv=bool(split), num_beams=nb, groups=G, finished_hypotheses=0)
        if sampled:
            stats.update(beam_sampled_steps=0, beam_host_steps=0)
        self.last_stats = stats
        caches, nl, T_cap, C, R = ws["caches"], len(ws["caches"]), self.T_cap, 2 * L.D, self.slots
        h_ids, h_src, h_sc = _beam_upload(ws["bupd_host"])
        h_ids[:], h_src[:], h_sc[:] = 0, np.arange(R), 0.0           # idle rows: themselves as parents
        ws["live"].zero_()                                           # an abandoned run may have left rows live
        ws["glive"].zero_()
        ws["bprm"].copy_(torch.tensor([int(min_length), int(eos_id)], dtype=i32))
        ban0 = int(eos_id) if 0 < min_length else -1
        room = min(T_cap, L.cos.shape[0])
        if sampled:
            K = 2 * nb
            inv_temp, top_k, top_p, pen = sampled
            ws["bsprm"].copy_(torch.tensor([inv_temp, top_p, float(top_k), pen], dtype=F32))
            rec_of = {name: (ws[name][:G * K].view(F32), ws[name][G * K:2 * G * K], ws[name][2 * G * K:]) for name in ("bsrec", "rec0s")}
            seed_of = {}                                             # group -> its request's seed

            def sample_topk(name, logits, scores, n, live, gen, seed, **kw):
                ops.beam_sample_topk_items(logits, scores, ws["part_k"], ws["part_s"], ws["part_i"], ws["part_f"], *rec_of[name], n, nb,
                                           live, gen, ws["bprm"], draw=draw, params=ws["bsprm"], seed=seed, t_add=0, **kw)

            def host_redo(logits_rows, scores, seqs, seed, t):      # the host's rule for one flagged group's selection
                stats["beam_host_steps"] += 1
                acc, flat, _ = beam_sample_select(logits_rows.cpu().numpy(), scores, seqs, int(eos_id) if t < min_length else -1, inv_temp,
                                                  top_k, top_p, pen, seed or 0, t, 0, draw)
                return acc, flat

        def feed(g):                                                 # the group's rows of the next upload
            ids, src, run = sched.feed[g]
            rows = slice(g * nb, (g + 1) * nb)
            h_ids[rows], h_src[rows], h_sc[rows] = ids, g * nb + np.asarray(src), run

        def refill(group):
            lens = []
            for _, (emb, _seed) in group:
                S0 = emb.shape[0] if emb.dim() == 2 else 0
                if S0 < 1 or S0 + max_new_tokens > room:
                    raise ValueError(f"request of shape {tuple(emb.shape)} + max_new_tokens {max_new_tokens} does not fit a slot of "
                                     f"{room} positions")
                lens.append(S0)
            if packed:
                logits0 = L._prefill_packed([req[0] for _, req in group], [g * nb for g, _ in group], caches)
            else:
                (g, req), = group
                logits0 = L._prefill(req[0][None].to(L.dev), [c[g * nb:g * nb + 1] for c in caches])
            n = len(group)
            stats["prefills"] += n
            if sampled:                                              # the prompt's row nb times, HF's initial scores, gen = 0
                seeds_ = [req[1] for _, req in group]
                if draw:
                    ws["seed0"][:n].copy_(torch.tensor(seeds_, dtype=torch.long))
                rows0 = logits0.repeat_interleave(nb, 0)
                sample_topk("rec0s", rows0, ws["score0"], n, ws["live1"], ws["gen0"], ws["seed0"] if draw else None)
                top_s, top_i, flags = _beam_sample_record(ws["rec0s"], G, K)
                for i in np.nonzero(flags[:n])[0]:
                    top_s[i], top_i[i] = host_redo(rows0[i * nb:(i + 1) * nb], ws["score0"][:nb].cpu().numpy(), [()] * nb, seeds_[i], 0)
            else:
                ops.beam_topk(logits0, ws["zero"], ws["part_s"], ws["part_i"], ws["rec0"][0].view(F32), ws["rec0"][1], n, nb,
                              ban_id=ban0)
                top_s, top_i = _beam_record(ws["rec0"], G)
            on = [(g, S0, req[1]) for i, ((g, req), S0) in enumerate(zip(group, lens)) if sched.admit(g, top_s[i], top_i[i])]
            if not on:
                return
            state = torch.zeros((3, G), dtype=i32)                   # the broadcast's lo = 0 | hi = S0 | live, per group
            for g, S0, _ in on:
                state[1, g], state[2, g] = S0, 1
            state = ops.h2d(state, L.dev)
            if nl:
                ops.beam_reorder_kv_items(ws["table"], nl, G, nb, T_cap, C, ws["bsrc"], state[0], state[1], state[2])
            for g, S0, seed in on:
                rows = slice(g * nb, (g + 1) * nb)
                ws["pos"][rows].fill_(S0)                            # position of the incoming token
                ws["kvlen"][rows].fill_(S0 + 1)                      # valid keys after the append
                ws["lo"][g:g + 1].fill_(S0)                          # the prompt prefix is the same in every row of the group
                ws["gen"][g:g + 1].fill_(1)                          # the prefill's selection was token 0
                if sampled:
                    ws["bseen"][rows].zero_()                        # generated ids only, and the last request's are gone
                    seed_of[g] = seed
                    if draw:
                        ws["bseed"][g:g + 1].fill_(seed)
                ws["live"][rows].fill_(1)
                ws["glive"][g:g + 1].fill_(1)
                feed(g)

        def token_step(_ban):
            if nl:
                ws["hi"].copy_(ws["pos"][::nb])                      # each group's position: generated rows are [lo, pos)
                ops.beam_reorder_kv_items(ws["table"], nl, G, nb, T_cap, C, ws["src"], ws["lo"], ws["hi"], ws["glive"])
            if sampled:                                              # the bitmaps follow their hypotheses; the fed token joins
                ops.beam_seen_update_items(ws["bseen"], ws["src"], ws["ids"], G, nb, V, ws["glive"])
                L._step_logits(ws)
                sample_topk("bsrec", ws["logits"], ws["bscore"], G, ws["glive"], ws["gen"], ws["bseed"] if draw else None,
                            seen=ws["bseen"], pos=ws["pos"], kvlen=ws["kvlen"])
                return
            L._step_logits(ws)
            ops.beam_topk_items(ws["logits"], ws["bscore"], ws["part_s"], ws["part_i"], ws["brec"][0].view(F32), ws["brec"][1], G, nb,
                                ws["glive"], ws["gen"], ws["bprm"], ws["pos"], ws["kvlen"])

        def read_sampled(live):                                      # the sampled step's record, flagged groups redone
            top_s, top_i, flags = _beam_sample_record(ws["bsrec"], G, K)
            stats["beam_sampled_steps"] += 1
            for g in live:
                if flags[g]:
                    item, rows = sched.rows[g][1], slice(g * nb, (g + 1) * nb)
                    top_s[g], top_i[g] = host_redo(ws["logits"][rows], h_sc[rows], item.run_seqs, seed_of[g], item.gen)
            return top_s, top_i

        def results():
            for index, seqs, scores in sched.pop():
                yield index, _pad_ids(seqs, pad), torch.from_numpy(np.asarray(scores, dtype=np.float32)), [len(q) for q in seqs]

        try:
            while True:
                group = plan.next_pass()
                while group:
                    refill(group)
                    group = plan.next_pass()
                yield from results()
                live = sched.live()
                if not live:
                    break
                ws["bupd"].copy_(ws["bupd_host"], non_blocking=True)    # ids | src | running scores: one host->device copy
                if L._launch_step(ws, token_step, -1, True, stats):
                    self.graph_captures += 1
                finished = sched.step(*(read_sampled(live) if sampled else _beam_record(ws["brec"], G)))
                for g in live:
                    if g in finished:
                        ws["live"][g * nb:(g + 1) * nb].zero_()
                        ws["glive"][g:g + 1].zero_()
                    else:
                        feed(g)
                yield from results()
        finally:
            stats.update(steps=sched.steps, live_row_steps=sched.live_row_steps, occupancy=sched.occupancy,
                         graph_captures=self.graph_captures, prefill_passes=plan.passes, packed_rows=plan.packed_rows,
                         finished_hypotheses=sched.finished_hypotheses)

    def _draft_args(self, draft_k, dev_sample: bool, penalty: bool, min_length: int, scores: bool, turns) -> int:
        """run(draft=...)'s checks of its arguments; returns K."""
        if not getattr(self.llama, "slot_draft", False):
            raise NotImplementedError("decode slots: draft decoding needs its switch (MYRIAD_SLOT_DRAFT=1 or llama.slot_draft = True)")
        K = int(draft_k)
        if not 1 <= K <= ops.DRAFT_MAX_K:
            raise ValueError(f"draft_k={draft_k}: 1 to {ops.DRAFT_MAX_K} rows per slot in a verify step")
        if self.slots * K > ops.GEMV_WIDE_MAX_ROWS:
            raise ValueError(f"slots={self.slots} x draft_k={K}: the verify step runs the packed token step, at most "
                             f"{ops.GEMV_WIDE_MAX_ROWS} rows")
        bare = not getattr(self.llama, "draft_sampling", False)      # behind that switch the verify step runs the per-row tail
        for on, what in ((bare and dev_sample, "device sampling"), (bare and penalty, "repetition_penalty != 1"),
                         (bare and int(min_length) > 1, "min_length > 1"), (bare and scores, "return_scores"),
                         (turns is not None and not getattr(self.llama, "draft_split", False), "run_turns / ChatPool")):
            if on:
                raise NotImplementedError(f"decode slots: draft decoding with {what} is not implemented")
        return K

    @torch.no_grad()
    def _run(self, requests, turns, weights_version, max_new_tokens: int = 90, stop_ids=((835,), (2277, 29937)), eos_id: int = 2,
             min_length: int = 1, do_sample: bool = False, top_p: float = 1.0, temperature: float = 1.0, top_k: int = 50,
             generator: Optional[torch.Generator] = None, ordered: bool = False, prefill_batch: int = 1, refill_min: int = 1,
             prefill_rows: int = 2048, repetition_penalty: float = 1.0, seeds=None, return_scores: bool = False, watch_ids=(),
             draft=None, draft_k: int = 4):
        """`run` (requests) and `run_turns` (turns + weights_version): one engine, two admission rules."""
        L = self.llama
        scores = bool(return_scores)
        watch = ops.score_watch_table(watch_ids if scores else (), L.V)
        inv_temp, top_k, dev_sample, penalty = _sampling_args(L, do_sample, temperature, top_k, repetition_penalty)
        if penalty and not L.device_sampling:
            raise NotImplementedError(f"decode slots: repetition_penalty={repetition_penalty} needs the device sampling switch "
                                      "(MYRIAD_DEVICE_SAMPLING=1 or llama.device_sampling = True)")
        if seeds is not None and not dev_sample:
            raise ValueError("seeds= names the device sampler's per-request streams: it needs do_sample with device_sampling on")
        rows_tail = dev_sample or penalty or min_length > 1          # else exactly the launches of the plain slot step
        K = 0 if draft is None else self._draft_args(draft_k, dev_sample, penalty, min_length, scores, turns)
        # the attention kernel of every token step of this call, chosen once: `run` does not know its lengths up front
        split = self.split_kv
        if split is None:
            live_rows, longest = (self.slots, 0) if turns is None else (len(turns), max([int(t[1].shape[0]) for t in turns], default=0))
            split = split_kv_rows_rule(live_rows, L.H, longest)
        ws = self._workspace(inv_temp, (dev_sample, penalty) if rows_tail else None, split, scores)
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
            begun = self.sessions.plan([(t[0], list(t[2])) + t[3:] for t in turns], _cache_stamp(L, weights_version))
            seeds_ = [sd for _, sd in seeded_requests(turns, generator, seeds)] if dev_sample else [None] * len(turns)
            # a turn travels as (emb, seed, past) and is admitted in list order: its index is its place in `turns`
            plan = TurnPlanner([(slot, (t[1], sd, past)) for t, sd, (slot, past, _) in zip(turns, seeds_, begun)], prefill_batch,
                               prefill_rows, length=lambda q: int(q[0].shape[0]) - q[2])
            stats["turns"] = [dict(context_tokens=int(t[1].shape[0]), reused_tokens=past, prefilled_tokens=int(t[1].shape[0]) - past,
                                   full_reprefill_reason=reason) for t, (_, past, reason) in zip(turns, begun)]
        self.last_stats = stats
        run = _SlotRun(self, ws, sched, stats, turns, max_new_tokens=max_new_tokens, eos_id=eos_id, min_length=min_length,
                       do_sample=do_sample, top_p=top_p, inv_temp=inv_temp, top_k=top_k, dev_sample=dev_sample, penalty=penalty,
                       rows_tail=rows_tail, generator=generator, scores=scores, W=int((watch >= 0).sum()))
        if scores:
            ws["watch"].copy_(watch)
        dv = None
        if K:                                                        # draft decoding: the verify view, unless the call cannot use it
            split_off = split and not getattr(L, "draft_split", False)   # the split-KV view drafts behind its switch only
            stats.update(draft_k=K, draft_off="split_kv" if split_off else None, verify_steps=0, plain_steps=0, draft_proposed=0,
                         draft_accepted=0, emitted=0, verify_graph_replays=0, plain_graph_replays=0)
            if not split_off and not (ops.attn_decode_split_draft_supported(L.H, L.hd, K, self.T_cap) if split else
                                      ops.attn_decode_draft_supported(L.H, L.hd, K, self.T_cap)):
                stats["draft_off"] = "unsupported"
            if K > 1 and stats["draft_off"] is None:
                # the per-row tail, the scores: the verify step of draft_sampling; else exactly the launches it had before
                dv_tail = (dev_sample, penalty, rows_tail, scores) if rows_tail or scores else None
                dv = run.dv = self._draft_workspace(K, inv_temp, dv_tail, bool(split))
                # the host draws where p_max (f32) < top_p (a double): the device holds the smallest f32 >= top_p, so its
                # p_max >= *top_p is that test's negation for every f32 p_max; <= 0: no row needs a draw
                dv["top_p"].copy_(torch.from_numpy(np.array([f32_at_least(top_p) if do_sample else 0.0], dtype=np.float32)))
        ws["live"].zero_()                                           # an abandoned run may have left slots live
        ws["step"].zero_()
        if rows_tail:
            ws["prm"].copy_(torch.tensor([inv_temp, top_p, float(top_k), float(repetition_penalty), float(min_length), float(eos_id)],
                                         dtype=F32))
        try:
            while True:
                group = plan.next_pass()
                while group:
                    run.refill(group, packed)
                    group = plan.next_pass()
                yield from run.results()
                live = sched.live()
                if not live:
                    break
                guesses = slot_guesses(sched, draft, K) if dv is not None else None
                if guesses is not None and any(guesses.values()):    # THE RULE: a verify step iff a live slot has a real guess
                    run.verify_step(live, guesses)
                    yield from run.results()
                    continue
                replays = stats["graph_replays"]
                if L._launch_step(ws, run.token_step, -1, True, stats):
                    self.graph_captures += 1
                if K:
                    stats["plain_steps"] += 1
                    stats["plain_graph_replays"] += stats["graph_replays"] - replays
                r = run.rec.cpu()                                    # the one device->host copy of the step (it also waits for it)
                ids = run.host_draws(live, r)
                run.note_scores(live, r, ids)
                finished = sched.step(ids, r[1].tolist())
                for s in live:
                    if s in finished:
                        ws["live"][s:s + 1].zero_()
                    elif ids[s] != int(r[0][s]):
                        ws["ids"][s:s + 1].fill_(ids[s])             # a host draw replaces the arg-max the step fed back
                yield from run.results()
        finally:
            stats.update(steps=sched.steps, live_row_steps=sched.live_row_steps, occupancy=sched.occupancy,
                         graph_captures=self.graph_captures, prefill_passes=plan.passes, packed_rows=plan.packed_rows)
            if K:
                stats["emitted"] = sched.emitted


class _SlotRun:
    """One SlotDecoder._run call: its workspace view, scheduler, counters and knobs, and the pieces of its loop -- the token step,
    the refill of free slots, the results that leave, the host's draws."""

    def __init__(self, dec, ws, sched, stats, turns, **knobs):
        self.dec, self.L, self.ws, self.sched, self.stats, self.turns = dec, dec.llama, ws, sched, stats, turns
        # max_new_tokens, eos_id, min_length, do_sample, top_p, inv_temp, top_k, dev_sample, penalty, rows_tail, generator, scores,
        # W (the watch ids in use)
        vars(self).update(knobs)
        self.ban0 = self.eos_id if 0 < self.min_length else -1
        self.rec = ws["rec"] if self.rows_tail or self.scores else ws["rec"][:3]      # with scores: the score rows behind the four
        self.seed_of = {}                                            # slot -> its request's seed
        self.sc_of = {}                                              # request index -> its [pick log-prob, watch log-probs] per token

    def token_step(self, _ban):
        ws, rec = self.ws, self.rec
        self.L._step_logits(ws)
        if not self.rows_tail:
            ops.argmax_pmax_rows(ws["logits"], ws["nxt"], ws["mar"], ws["pmx"], ban_id=-1, inv_temp=self.inv_temp)
            if self.scores:
                ops.token_scores_rows(ws["logits"], ws["nxt"], ws["watch"], rec[4:], ws["live"])
            ops.decode_advance_rows(ws["nxt"], ws["mar"], ws["pmx"], rec, ws["ids"], ws["step"], ws["pos"], ws["kvlen"],
                                    ws["live"])
            return
        if self.penalty:                                             # ws["ids"] = the token fed in: it joins the seen set first
            ops.repetition_penalty_rows_slots(ws["logits"], ws["seen"], ws["ids"], ws["prm"][3:], ws["live"])
        if self.dev_sample:                                          # row r draws Philox step gen[r] of seed[r]
            ops.sample_rows_slots(ws["logits"], ws["nxt"], ws["mar"], ws["pmx"], ws["kept"], ws["prm"], ws["seed"], ws["gen"],
                                  ws["live"])
        else:
            ops.argmax_pmax_rows_slots(ws["logits"], ws["nxt"], ws["mar"], ws["pmx"], ws["prm"], ws["gen"], ws["live"])
        if self.scores:
            ops.token_scores_rows(ws["logits"], ws["nxt"], ws["watch"], rec[4:], ws["live"])
        ops.decode_advance_kept_rows(ws["nxt"], ws["mar"], ws["pmx"], ws["kept"] if self.dev_sample else None, rec, ws["ids"],
                                     ws["step"], ws["pos"], ws["kvlen"], ws["gen"], ws["live"])

    def verify_token_step(self, _ban):
        """The verify step of draft decoding (SlotDecoder._draft_workspace): slots x K rows, K consecutive tokens per slot."""
        dv = self.dv
        K = dv["draft_k"]
        self.L._step_logits(dv)
        if "arec" not in dv:                                         # no per-row tail, no scores: the launches of the greedy verify step
            ops.argmax_pmax_rows(dv["logits"], dv["nxt"], dv["mar"], dv["pmx"], ban_id=-1, inv_temp=self.inv_temp)
            ops.draft_accept_rows(dv["nxt"], dv["mar"], dv["pmx"], dv["ids"], dv["next_ids"], dv["nguess"], dv["live"], dv["top_p"],
                                  dv["drec"], dv["pos"], dv["kvlen"], dv["step"], K)
            return
        # row (g, j) is the plain step's row g at token gen[g] + j: its seen set is seen[g] + the ids fed in rows 0 .. j, its draw
        # Philox step gen[g] + j of seed[g], its ban the one of that token index
        if self.penalty:
            ops.repetition_penalty_draft_rows(dv["logits"], dv["seen"], dv["ids"], dv["nrow"], dv["live"], dv["prm"][3:], K)
        if self.rows_tail:
            ops.sample_rows_draft(dv["logits"], dv["nxt"], dv["mar"], dv["pmx"], dv["kept"], dv["prm"],
                                  dv["seed"] if self.dev_sample else None, dv["gen"], dv["nrow"], dv["live"], K, self.dev_sample)
        else:
            ops.argmax_pmax_rows(dv["logits"], dv["nxt"], dv["mar"], dv["pmx"], ban_id=-1, inv_temp=self.inv_temp)
        if self.scores:                                              # after the penalty and the pick; an idle row's id is -1: zeros
            ops.token_scores_rows(dv["logits"], dv["nxt"], dv["watch"], dv["sc"])
        ops.draft_accept_sampled_rows(dv["nxt"], dv["mar"], dv["pmx"], dv["kept"] if self.dev_sample else None, dv["ids"],
                                      dv["next_ids"], dv["nguess"], dv["live"], dv["top_p"], dv["seen"] if self.penalty else None,
                                      dv["arec"], dv["pos"], dv["kvlen"], dv["gen"], dv["step"], K, self.L.V)

    def verify_step(self, live, guesses) -> list:
        """One verify step for the `live` slots with their real `guesses`: two host->device copies (per slot the fed token, its
        guesses and id 0 as filler; the counts), the launch, one device->host copy (the record).  A slot's window is the n_out
        picks the device kept; under do_sample a pick with p_max < top_p (it ends the window on the device) is drawn here from
        its row of the verify logits and handed to the plain step's fed ids as well.  Returns the slots that finished."""
        dv, ws, sched, stats = self.dv, self.ws, self.sched, self.stats
        K, S = dv["draft_k"], self.dec.slots
        ids_k, cnt = [0] * (S * K), [[0] * S, [1] * S]
        for s in live:
            g = guesses[s]
            ids_k[s * K:s * K + 1 + len(g)] = [sched.rows[s][1][-1]] + g
            cnt[0][s], cnt[1][s] = len(g), 1 + len(g)
        dv["ids"].copy_(torch.tensor(ids_k, dtype=torch.long))
        dv["cnt"].copy_(torch.tensor(cnt, dtype=torch.int32))
        replays = stats["graph_replays"]
        if self.L._launch_step(dv, self.verify_token_step, -1, True, stats):
            self.dec.graph_captures += 1
        stats["verify_steps"] += 1
        stats["verify_graph_replays"] += stats["graph_replays"] - replays
        stats["draft_proposed"] += sum(len(guesses[s]) for s in live)
        r = dv["drec"].cpu()                                         # the one device->host copy of the step (it also waits for it)
        tail, sc = "arec" in dv, None
        if tail:                                                     # (4K + 1) floats per slot, then the score rows
            n_acc = S * (4 * K + 1)
            r, sc = r[:n_acc].view(S, 4 * K + 1).tolist(), r[n_acc:].view(ops.SCORE_ROWS, S * K).tolist() if self.scores else None
        else:
            r = r.tolist()
        windows, drawn = {}, {}
        for s in live:
            n = int(r[s][-1])
            if not 1 <= n <= cnt[1][s]:
                raise RuntimeError(f"verify step: slot {s} kept {n} of {cnt[1][s]} rows")
            hist, ids = list(sched.rows[s][1]), []
            for j in range(n):                                       # token by token, so no draw is made past the request's end
                tok = int(r[s][j])
                if self.dev_sample and r[s][3 * K + j] >= 0:
                    stats["device_sampled_rows"] += 1                # drawn by the step itself
                elif self.do_sample and (self.dev_sample or r[s][2 * K + j] < self.top_p):
                    # the plain step's rule per row: the sampler handed the row back, or p_max is below top_p -- the host draws
                    if j != n - 1:
                        raise RuntimeError("a row that needs a host draw must end its window")
                    tok = drawn[s] = self.host_draw(dv["logits"][s * K + j], len(hist), self.seed_of.get(s))
                if sc is not None:
                    self.sc_of[sched.rows[s][0]].append(self.score_entry([row[s * K + j] for row in sc], tok != int(r[s][j]),
                                                                         dv["logits"][s * K + j], tok))
                ids.append(tok)
                hist.append(tok)
                if sched._ended(hist):
                    break
            windows[s] = (ids, r[s][K:K + len(ids)])
        finished = sched.step_windows(windows)
        stats["draft_accepted"] += sum(sched.taken[s] - 1 for s in live)
        for s in live:
            if s in finished:
                ws["live"][s:s + 1].zero_()
            elif s in drawn:
                ws["ids"][s:s + 1].fill_(drawn[s])                   # a host draw replaces the pick the step fed back
        return finished

    def results(self):
        for index, ids, mar in self.sched.pop():
            n = index                                                # the request's place in the input: what sc_of is keyed by
            if self.turns is not None:                               # the slot now holds the context and every id but the last
                session, _, keys = self.turns[index][:3]
                self.dec.sessions.end(session, keys, ids)
                index = session
            out = (index, torch.tensor(ids, dtype=torch.long), torch.tensor(mar, dtype=F32))
            if self.scores:
                sc = torch.tensor(self.sc_of.pop(n), dtype=torch.float64).to(F32).view(len(ids), 1 + self.W)
                out += (dict(token_logprobs=sc[:, 0].contiguous(), watch_logprobs=sc[:, 1:].contiguous()),)
            yield out

    def fits(self, emb: torch.Tensor) -> int:
        S0 = emb.shape[0] if emb.dim() == 2 else 0
        room = min(self.dec.T_cap, self.L.cos.shape[0])
        if S0 < 1 or S0 + self.max_new_tokens > room:
            raise ValueError(f"request of shape {tuple(emb.shape)} + max_new_tokens {self.max_new_tokens} does not fit a slot of "
                             f"{room} positions")
        return S0

    def go_live(self, s: int, first: int, S0: int, seed) -> None:
        ws, sl = self.ws, slice(s, s + 1)
        ws["ids"][sl].fill_(first)
        ws["pos"][sl].fill_(S0)                                      # position of the incoming token
        ws["kvlen"][sl].fill_(S0 + 1)                                # valid keys after the append
        if self.rows_tail:
            ws["gen"][sl].fill_(1)                                   # the prefill pick was token 0
            if self.dev_sample:
                ws["seed"][sl].fill_(seed)
                self.seed_of[s] = seed
            if self.penalty:
                ws["seen"][sl].zero_()                               # generated ids only, and the last request's are gone
        ws["live"][sl].fill_(1)

    def first_picks(self, logits0: torch.Tensor, sl: slice, seeds_) -> list:
        """The first pick of each prefilled request (rows of logits0) in one launch into the step's result buffers at `sl` and
        one device->host copy: rows of [id, margin, p_max, kept].  The per-row tail's pick is its step kernel at gen = 0.  With
        scores the SCORE_ROWS entries of mh_token_scores_rows on the same logits are the last items of each row."""
        ws = self.ws
        out = [ws["nxt"][sl], ws["mar"][sl], ws["pmx"][sl]]
        R = logits0.shape[0]
        if self.dev_sample:
            ws["seed0"][:R].copy_(torch.tensor(seeds_, dtype=torch.long))
            ops.sample_rows_slots(logits0, *out, ws["kept"][sl], ws["prm"], ws["seed0"][:R], ws["gen0"][:R])
            out.append(ws["kept"][sl])
        elif self.rows_tail:
            ops.argmax_pmax_rows_slots(logits0, *out, ws["prm"], ws["gen0"][:R])
        else:
            ops.argmax_pmax_rows(logits0, *out, ban_id=self.ban0, inv_temp=self.inv_temp)
        if self.scores:
            sc0 = ops.token_scores_rows(logits0, out[0], ws["watch"], ws["sc0"][:, :R])
            out.extend(sc0[i] for i in range(ops.SCORE_ROWS))
        return torch.stack([o.to(torch.float64) for o in out], 1).tolist()

    def host_draw(self, logits_row: torch.Tensor, t: int, seed) -> int:
        """Token t of a request, drawn on the host: from a generator derived from the request's seed and t where the device
        sampler handed the row back, else from the run's own; the EOS ban is the step's for that t."""
        self.stats["host_sampled_rows"] += 1
        return _host_draw(logits_row, self.eos_id if t < self.min_length else -1, self.inv_temp, self.top_k, self.top_p,
                          _request_generator(seed, t) if self.dev_sample else self.generator)

    def first_id(self, pick, logits_row: torch.Tensor, seed) -> int:
        """The request's first token from its pick: the device's draw, or the host's where the rules hand the row to it."""
        if self.dev_sample and pick[3] >= 0:
            self.stats["device_sampled_rows"] += 1
        elif self.dev_sample or (self.do_sample and pick[2] < self.top_p):
            return self.host_draw(logits_row, 0, seed)
        return int(pick[0])

    def refill(self, group, packed: bool) -> None:
        """Prefill the group's requests, each into its slot: one request alone into the slot's slice of every cache (_prefill), or
        -- `packed` -- the group in one packed pass (_prefill_packed; their GEMM plans differ).  Then one pick launch and one
        device->host copy for all first picks, and admission in input order; a slot goes live if its request goes on."""
        L, ws, turns = self.L, self.ws, self.turns
        lens = [self.fits(req[0]) for _, req in group]
        if packed:
            pasts = None if turns is None else [req[2] for _, req in group]
            logits0 = L._prefill_packed([req[0] for _, req in group], [s for s, _ in group], ws["caches"], pasts)
        else:
            (s, req), = group
            logits0 = L._prefill(req[0][None].to(L.dev), [c[s:s + 1] for c in ws["caches"]], req[2] if turns is not None else 0)
        sl = slice(0, len(group)) if packed else slice(s, s + 1)
        self.stats["prefills"] += len(group)
        picks = self.first_picks(logits0, sl, [req[1] for _, req in group])
        for i, (s, req) in enumerate(group):
            first = self.first_id(picks[i], logits0[i], req[1])
            if self.scores:
                self.sc_of[self.sched.admitted] = [self.score_entry(picks[i][-ops.SCORE_ROWS:], first != int(picks[i][0]), logits0[i],
                                                                    first)]
            if self.sched.admit(s, first, picks[i][1]):
                self.go_live(s, first, lens[i], req[1])

    def score_entry(self, sc, redrawn: bool, logits_row: torch.Tensor, tok: int) -> list:
        """One token's [pick log-prob, watch log-probs] from its SCORE_ROWS entries `sc` (lse, pick, watch slots); a token the host
        drew instead takes x[id] - lse in f32 from the logits row the draw read."""
        lp = float(logits_row[tok].cpu() - torch.tensor(sc[0], dtype=F32)) if redrawn else float(sc[1])
        return [lp] + [float(v) for v in sc[2:2 + self.W]]

    def note_scores(self, live, r, ids) -> None:
        """The scores of one token step's record `r` join their requests' lists (before the scheduler retires finished rows);
        `ids` = host_draws' answer for the step."""
        if not self.scores:
            return
        sc = r[4:].tolist()
        for s in live:
            index = self.sched.rows[s][0]
            self.sc_of[index].append(self.score_entry([row[s] for row in sc], ids[s] != int(r[0][s]), self.ws["logits"][s], ids[s]))

    def host_draws(self, live, r) -> list:
        """The ids of one token step's record `r`, with the rows the rules hand to the host drawn there."""
        ids = r[0].long().tolist()
        for s in live if self.do_sample else ():
            if self.dev_sample and float(r[3][s]) >= 0:
                self.stats["device_sampled_rows"] += 1               # drawn by the step itself
            elif self.dev_sample or float(r[2][s]) < self.top_p:     # greedy_generate's rule per row: below top_p the host draws
                t = len(self.sched.rows[s][1])                       # the row's gen when the step ran
                ids[s] = self.host_draw(self.ws["logits"][s], t, self.seed_of.get(s))
        return ids
