#!/usr/bin/env python3
"""Closed-set answer ranking on the full-size synthetic model: MyriadHIP.score_answers against the two ways to a closed answer
the project had before it.  148-row prompts (the stage-1 wrap without BOS: 4 ids, the image rows and 45 ids), batch 8; the default two candidates and a 4- and an 8-candidate case, every candidate --tokens (12) ids.

    python tools/rank_bench.py [--batch 8] [--cands 2,4,8] [--tokens 12] [--repeats 5] [--lora 1]

Per case three whole calls are timed in one process, interleaved (one round = each of them once; round 0 warms up and is dropped),
wall clock around a device synchronise, median / min / max of --repeats:

  1. score   model.score_answers(samples, candidate_ids=...): the vision encode, one packed prompt prefill, one scoring pass over
             all candidates of all prompts (mh_attn_prefill_ragged_shared), the lm-head and mh_token_scores_rows on their rows;
  2. solo    the same numbers from what was there before: the same vision encode and prompt assembly once, then per candidate
             one solo LlamaHIP._prefill of prompt + candidate at the batch's size (its launches restated here from the engine's
             pieces, because _prefill itself returns the last row's logits only), followed by the same lm-head and
             mh_token_scores_rows on the rows that score the candidate.  Its log-probs are compared with (1)'s and the largest
             difference is printed: the two differ through the GEMMs' row-count-dependent plans only;
  3. decode  model.generate(samples, max_new_tokens=--tokens): the vision encode, the prefill and --tokens - 1 token steps.  On
             random weights no stop sequence ends the answer, so the answer's length is pinned to the candidates' (no stop id, no
             EOS, as tools/decode_bench.py decodes)."""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myriad_amd import ops  # noqa: E402
from myriad_amd.myriad import MyriadHIP  # noqa: E402
from myriad_amd.synthetic import SyntheticWeights, full_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--cands", default="2,4,8")
ap.add_argument("--tokens", type=int, default=12)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--llm-layers", type=int, default=32)
ap.add_argument("--lora", type=int, default=1)
a = ap.parse_args()
dev, F32 = "cuda:0", torch.float32
cfg = full_config(llm_layers=a.llm_layers)
model = MyriadHIP(SyntheticWeights(cfg, dev, seed=0), dict(need_backward=False, use_lora=bool(a.lora)), device=dev)
model.eval()
L = model.llama
g = torch.Generator().manual_seed(1)
B = a.batch
samples = dict(image=torch.randn(B, 3, 224, 224, generator=g), anomaly_maps=torch.rand(B, 1, 224, 224, generator=g),
               before_ids=torch.randint(3, 32000, (1, 4), generator=g).expand(B, -1).contiguous(),
               after_ids=torch.randint(3, 32000, (1, 45), generator=g).expand(B, -1).contiguous())


def prompt_embs():
    """score_answers' prompt assembly: [B, S, D] f32 without the BOS row."""
    image = samples["image"].to(dev, F32)
    maps = model._maps_for(samples, "anomaly_maps", image)
    parts = model.encode_img(image, maps, 1, False)
    emb, _, _, _ = model._assemble(parts, samples["before_ids"], samples["after_ids"], None, None)
    return emb[:, 1:].contiguous()


def solo_rows(x, S):
    """LlamaHIP._prefill(x, caches)'s launches on [B, S0, D], returning the hidden rows S - 1 .. S0 - 1 of every batch row (the
    rows whose logits score the continuation) where _prefill keeps the last one."""
    Bn, S0, D = x.shape
    H, hd, W, scale = L.H, L.hd, L.D, 1.0 / math.sqrt(L.hd)
    pos = torch.arange(0, S0, dtype=torch.int32).repeat(Bn).to(dev)
    caches = L._decode_workspace(Bn, S0, 1.0)["caches"]

    def attention(li, qkv):
        q3, cache = qkv.view(Bn, S0, 3 * W), caches[li]
        ops.rope_(qkv, 0, 2 * H, hd, pos, L.cos, L.sin, 1.0)
        ops.copy3d_bf16(q3[:, :, W:], cache[:, :S0])
        kc = cache[:, :S0]
        return ops.attn_fwd(q3[:, :, :W], kc[:, :, :W], kc[:, :, W:], H, hd, scale, causal=True, need_lse=False)[0]

    h = L._decode_layers(x.reshape(Bn * S0, D).contiguous(), L._gemm_lin, attention, L.lora)
    rows = torch.cat([torch.arange(b * S0 + S - 1, b * S0 + S0, dtype=torch.int32) for b in range(Bn)])
    return ops.gather_rows_f32(h, ops.h2d(rows, dev))


def run_score(ids):
    return model.score_answers(samples, candidate_ids=ids)["answer_token_logprobs"]


def run_solo(ids):
    model.finish_update()
    if L.lora is not None:
        L.lora.refresh(L.layers)
    emb = prompt_embs()
    S, out = emb.shape[1], []
    for c in ids:
        n = len(c)
        tail = torch.zeros((n - 1, L.D), dtype=F32, device=dev)
        L.embed_tokens_into(c[:-1].to(dev), tail)
        x = torch.cat([emb, tail[None].expand(B, -1, -1)], 1).contiguous()
        logits = L._last_rows_logits(solo_rows(x, S))                    # [B * n, V]
        out.append(L._token_logprobs(logits, c.tolist() * B).cpu().view(B, n))
    return [[out[c][b] for c in range(len(ids))] for b in range(B)]


def run_decode(_ids):
    return model.generate(samples, max_new_tokens=a.tokens, stop_ids=((-1,),), min_length=0, eos_token_id=-5)["token_ids"]


def timed(fn, ids):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(ids)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


print(f"full-size synthetic model, {len(L.layers)} LLaMA layers, LoRA {'on' if a.lora else 'off'}, batch {B}, prompts of "
      f"{prompt_embs().shape[1]} rows, candidates of {a.tokens} tokens; ms per call, median / min / max of {a.repeats} interleaved")
for C in [int(x) for x in a.cands.split(",") if x]:
    ids = [torch.randint(3, 32000, (a.tokens,), generator=g) for _ in range(C)]
    ts = {"score": [], "solo": [], "decode": []}
    diff, mag = 0.0, 0.0
    for rnd in range(a.repeats + 1):
        for name, fn in (("score", run_score), ("solo", run_solo), ("decode", run_decode)):
            t, out = timed(fn, ids)
            if rnd:
                ts[name].append(t)
            if name == "score":
                mine = out
                mag = max(float(x.abs().max()) for row in out for x in row)
            elif name == "solo":
                diff = max(diff, max(float((x - y).abs().max()) for ra, rb in zip(mine, out) for x, y in zip(ra, rb)))
    st = model.last_score_stats
    line = [f"{C} candidates ({st['passes']} passes, {st['packed_rows']} packed rows, {st['segments']} segments):"]
    for name in ("score", "solo", "decode"):
        v = sorted(ts[name])
        line.append(f"{name} {v[len(v) // 2] * 1e3:.2f} / {v[0] * 1e3:.2f} / {v[-1] * 1e3:.2f}")
    med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
    line.append(f"solo / score {med['solo'] / med['score']:.2f}x, decode / score {med['decode'] / med['score']:.2f}x; "
                f"max |log-prob score - solo| {diff:.2e} (largest |log-prob| {mag:.2f})")
    print("  ".join(line), flush=True)
