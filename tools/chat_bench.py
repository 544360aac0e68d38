#!/usr/bin/env python3
"""Chat-session decode on the full-size LLaMA (Vicuna-7B shapes, synthetic weights), batch 1:

  * ms per token at cached contexts of 256 / 1,024 / 2,048 keys, with the split-KV decode attention (mh_attn_decode_rope_split)
    and with the single-workgroup kernel (mh_attn_decode_rope), each in a DecodeSession (captured token step);
  * time to first token of turn 2 (turn 1's context + its answer + a new question) with the cache reused and with a full
    re-prefill;
  * --chunks: the attention launch alone (32 launches = one token's layers, replayed from a graph) for the single-workgroup kernel
    and the split kernel at 128 / 256 / 512 keys per chunk;
  * --ragged-past: mh_attn_prefill_ragged_past alone against the three launches per request it replaces (rope, cache copy,
    causal attention over past + len keys), R = 8 requests, at (past, len) = (256, 32) and (1024, 32);
  * --pool N[,N...]: N conversations of 3 turns each (a context of --pool-context keys, then per turn the answer of --tokens
    tokens and a 24-token question) through SlotDecoder.run_turns on N slots -- what ChatPool.answer_many runs -- against the same
    turns through N DecodeSessions one after the other -- what N Chat objects run; tokenising and image encoding are the same on
    both sides and left out.  The two are interleaved per repeat; wall ms per turn, median of --repeats with min and max;
  * --pool-split: the --pool protocol on two SlotDecoders, split_kv=False (the single-workgroup rows kernel) and split_kv=True
    (mh_attn_decode_rope_split_rows), interleaved per repeat in one process, for N in --pool (default 1,2,4,7,8) and first
    contexts in --pool-contexts (default 512,1024,2048,4096): wall ms per turn and ms per token step -- (a turn of --tokens + 1
    tokens) - (a turn of 1 token) on the cached third context --, median of --repeats (default 5 here) with min and max.  Before
    it, the two attention launches alone (32 launches = one token's layers, from a graph) at R = 1, 4, 8 live rows on 1,024 /
    4,096 cached keys;
  * --split-draft: draft-and-verify decoding on the split-KV view (behind llama.draft_split).  First the attention launch pair
    alone (32 pairs = one step's layers, from a graph, interleaved per round): mh_attn_decode_rope_split_draft_rows at 1,024 /
    2,160 keys and (G, K) = (1, 4), (1, 8), (2, 4) against K sequential mh_attn_decode_rope_split_rows launches and against
    mh_attn_decode_rope_draft_rows at the same shape.  Then a turn of --tokens tokens on a cached context of --pool-context keys
    (one row prefilled) with no drafter, a drafter taught the answers and an untaught one, interleaved per repeat: one
    DecodeSession(split=True), and N conversations (--pool, default 1,2,8) through run_turns on split_kv=True and False decoders;
    the ids are asserted equal to the run without a drafter.

python tools/chat_bench.py [--layers 32] [--tokens 32] [--repeats 3] [--chunks] [--ragged-past] [--pool 1,4,8,16] [--pool-split]
                           [--split-draft]
-> one JSON line per measurement"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from myriad_amd import ops  # noqa: E402
from myriad_amd.decode import DecodeSession  # noqa: E402
from myriad_amd.llama import LlamaHIP  # noqa: E402
from myriad_amd.synthetic import SyntheticWeights, full_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--tokens", type=int, default=32, help="timed token steps per measurement")
ap.add_argument("--repeats", type=int, default=None, help="default 3, 5 with --pool-split")
ap.add_argument("--contexts", default="256,1024,2048")
ap.add_argument("--chunks", action="store_true", help="also time the attention launch alone per chunk size")
ap.add_argument("--skip-model", action="store_true", help="only the --chunks / --ragged-past launch timings")
ap.add_argument("--ragged-past", action="store_true", help="time mh_attn_prefill_ragged_past against the launches it replaces")
ap.add_argument("--pool", default="", help="conversation counts for the pool-against-sequential-sessions comparison")
ap.add_argument("--pool-context", type=int, default=256, help="keys of a conversation's first context")
ap.add_argument("--pool-split", action="store_true", help="the pool with split_kv=False against split_kv=True")
ap.add_argument("--pool-contexts", default="512,1024,2048,4096", help="first contexts of the --pool-split comparison")
ap.add_argument("--split-draft", action="store_true", help="draft decoding on the split-KV view: the attention pair alone, a chat "
                "turn and the pool with a taught / an untaught drafter against no drafter")
ap.add_argument("--draft-k", type=int, default=4, help="rows per verify step of the --split-draft turns")
a = ap.parse_args()
if a.repeats is None:
    a.repeats = 5 if a.pool_split or a.split_draft else 3
if a.split_draft and not a.pool:
    a.pool = "1,2,8"
if a.split_draft and a.pool_context == 256:
    a.pool_context = 1136                                            # past the split-KV threshold of a solo chat turn
if a.pool_split and not a.pool:
    a.pool = "1,2,4,7,8"
dev = "cuda:0"
torch.manual_seed(0)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def chunk_bench():
    B, H, D, T = 1, 32, 128, 2048 + 64
    W = H * D
    cache = (torch.randn((B, T, 2 * W), device=dev) * 0.5).to(torch.bfloat16)
    qkv = (torch.randn((B, 3 * W), device=dev) * 0.5).to(torch.bfloat16)
    fr = torch.arange(T).float()[:, None] * (1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D)))[None]
    cos, sin = fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)
    part = ops.attn_decode_split_ws(B, H, T, dev, chunk=128)
    out = torch.empty((B, W), dtype=torch.bfloat16, device=dev)
    for kv in [int(x) for x in a.contexts.split(",")]:
        pos = torch.full((B,), kv - 1, dtype=torch.int32, device=dev)
        kvl = torch.full((B,), kv, dtype=torch.int32, device=dev)
        variants = [("single", None)] + [("split", c) for c in (128, 256, 512)]
        for name, ch in variants:
            def one():
                for _ in range(32):
                    if ch is None:
                        ops.attn_decode_rope(qkv, cache, pos, pos, kvl, cos, sin, H, D, 1.0 / D ** 0.5)
                    else:
                        ops.attn_decode_rope_split(qkv, cache, pos, pos, kvl, cos, sin, H, D, 1.0 / D ** 0.5, part, chunk=ch, out=out)
            one()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                one()
            ts = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                g.replay()
                e0.record()
                for _ in range(20):
                    g.replay()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) / 20 / 32 * 1000.0)
            emit(what="attn_launch_us", kernel=name, chunk=ch, kv=kv, us_per_layer=round(statistics.median(ts), 2))
            del g


def ragged_past_bench():
    R, H, D, T = 8, 32, 128, 2048
    W, scale = H * D, 1.0 / D ** 0.5
    fr = torch.arange(T).float()[:, None] * (1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D)))[None]
    cos, sin = fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)
    cache = (torch.randn((R, T, 2 * W), device=dev) * 0.5).to(torch.bfloat16)
    for past, n in ((256, 32), (1024, 32)):
        M = R * n
        qkv = (torch.randn((M, 3 * W), device=dev) * 0.5).to(torch.bfloat16)
        work = qkv.clone()
        seg_host = torch.tensor([(i * n, n, i, past) for i in range(R)], dtype=torch.int32)
        seg = seg_host.to(dev)
        pos = (torch.arange(n, dtype=torch.int32) + past).repeat(R).to(dev)
        pos1 = pos[:n].contiguous()
        out = torch.empty((M, W), dtype=torch.bfloat16, device=dev)

        def fused():
            ops.attn_prefill_ragged_past(qkv, pos, seg, seg_host, cache, cos, sin, H, D, scale, out=out)

        def three():                                                 # per request, as R solo _prefill(emb, cache, past) calls do
            for i in range(R):
                x = work[i * n:(i + 1) * n]
                ops.rope_(x, 0, 2 * H, D, pos1, cos, sin, 1.0)
                q3 = x.view(1, n, 3 * W)
                ops.copy3d_bf16(q3[:, :, W:], cache[i:i + 1, past:past + n])
                kc = cache[i:i + 1, :past + n]
                ops.attn_fwd(q3[:, :, :W], kc[:, :, :W], kc[:, :, W:], H, D, scale, causal=True, need_lse=False)

        for name, fn in (("ragged_past", fused), ("three_launches_per_request", three)):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) / 20 * 1000.0)
            emit(what="prefill_attn_us", kernel=name, past=past, len=n, R=R, H=H, D=D, us=round(statistics.median(ts), 1),
                 min=round(min(ts), 1), max=round(max(ts), 1))


def rows_bench():
    """mh_attn_decode_rope_rows against mh_attn_decode_rope_split_rows, R live rows of kv cached keys each."""
    H, D = 32, 128
    W = H * D
    for kv in (1024, 4096):
        T = kv + 64
        fr = torch.arange(T).float()[:, None] * (1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D)))[None]
        cos, sin = fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)
        for R in (1, 4, 8):
            cache = (torch.randn((R, T, 2 * W), device=dev) * 0.5).to(torch.bfloat16)
            qkv = (torch.randn((R, 3 * W), device=dev) * 0.5).to(torch.bfloat16)
            work = qkv.clone()
            pos = torch.full((R,), kv - 1, dtype=torch.int32, device=dev)
            kvl = torch.full((R,), kv, dtype=torch.int32, device=dev)
            live = torch.ones((R,), dtype=torch.int32, device=dev)
            part = ops.attn_decode_split_ws(R, H, T, dev)
            out = torch.empty((R, W), dtype=torch.bfloat16, device=dev)
            res = {}
            for name in ("rows", "split_rows"):
                def one():
                    for _ in range(32):
                        if name == "rows":                           # rotates q in place: a scratch copy, the values do not matter
                            ops.attn_decode_rope_rows(work, cache, pos, kvl, live, cos, sin, H, D, 1.0 / D ** 0.5)
                        else:
                            ops.attn_decode_rope_split_rows(qkv, cache, pos, kvl, live, cos, sin, H, D, 1.0 / D ** 0.5, part, out=out)
                one()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    one()
                ts = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    g.replay()
                    e0.record()
                    for _ in range(20):
                        g.replay()
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) / 20 / 32 * 1000.0)
                emit(what="attn_rows_launch_us", kernel=name, rows=R, kv=kv, us_per_layer=round(statistics.median(ts), 2),
                     min=round(min(ts), 2), max=round(max(ts), 2))
                del g
            del cache, part
            torch.cuda.empty_cache()


def split_draft_attn_bench():
    """The split verify-step attention pair against the launches it stands for and against the non-split draft kernel."""
    H, D = 32, 128
    W, scale = H * D, 1.0 / D ** 0.5
    i32 = lambda v, n: torch.full((n,), v, dtype=torch.int32, device=dev)
    for kv in (1024, 2160):
        T = kv + 64
        fr = torch.arange(T).float()[:, None] * (1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D)))[None]
        cos, sin = fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)
        for G, K in ((1, 4), (1, 8), (2, 4)):
            cache = (torch.randn((G, T, 2 * W), device=dev) * 0.5).to(torch.bfloat16)
            qkv = (torch.randn((G * K, 3 * W), device=dev) * 0.5).to(torch.bfloat16)
            work = qkv.clone()                                       # the non-split draft kernel rotates q in place
            pos, live, nrow = i32(kv, G), i32(1, G), i32(K, G)
            pos_j = [i32(kv + j, G) for j in range(K)]
            kvl_j = [i32(kv + j + 1, G) for j in range(K)]
            part_d = ops.attn_decode_split_draft_ws(G, K, H, T, dev)
            part_s = ops.attn_decode_split_ws(G, H, T, dev)
            out = torch.empty((G * K, W), dtype=torch.bfloat16, device=dev)
            rows_j = [qkv[j::K] for j in range(K)]                   # row j of every group: [G, 3W], strided

            def split_draft():
                for _ in range(32):
                    ops.attn_decode_rope_split_draft_rows(qkv, cache, pos, live, nrow, cos, sin, H, D, scale, K, part_d, out=out)

            def sequential():
                for _ in range(32):
                    for j in range(K):
                        ops.attn_decode_rope_split_rows(rows_j[j], cache, pos_j[j], kvl_j[j], live, cos, sin, H, D, scale, part_s, out=out[j::K])

            def draft_rows():
                for _ in range(32):
                    ops.attn_decode_rope_draft_rows(work, cache, pos, live, nrow, cos, sin, H, D, scale, K, out=out)

            graphs = {}
            for name, fn in (("split_draft_rows", split_draft), ("sequential_split_rows", sequential), ("draft_rows", draft_rows)):
                fn()
                torch.cuda.synchronize()
                graphs[name] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[name]):
                    fn()
            ts = {name: [] for name in graphs}
            for rnd in range(6):                                     # round 0 warms up; the three interleaved per round
                for name, g in graphs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    g.replay()
                    e0.record()
                    for _ in range(20):
                        g.replay()
                    e1.record()
                    e1.synchronize()
                    if rnd:
                        ts[name].append(e0.elapsed_time(e1) / 20 / 32 * 1000.0)
            for name in graphs:
                emit(what="split_draft_attn_us", kernel=name, G=G, K=K, kv=kv, us_per_layer=round(statistics.median(ts[name]), 2),
                     min=round(min(ts[name]), 2), max=round(max(ts[name]), 2))
            del graphs, cache, part_d, part_s
            torch.cuda.empty_cache()


if a.chunks or (a.skip_model and not a.ragged_past and not a.pool_split and not a.split_draft):
    chunk_bench()
if a.split_draft:
    split_draft_attn_bench()
if a.pool_split:
    rows_bench()
if a.ragged_past:
    ragged_past_bench()
if a.skip_model:
    sys.exit(0)

cfg = full_config(llm_layers=a.layers)
max_pos = 4096
if a.pool_split:                                                     # the rotary table covers the longest conversation
    max_pos = max(4096, 256 + max(int(x) for x in a.pool_contexts.split(",")) + 3 * (a.tokens + 24) + 2)
llama = LlamaHIP(SyntheticWeights(cfg, dev, seed=0), cfg["llm_heads"], dev, need_backward=False, max_pos=max_pos)
D = llama.D
gen = torch.Generator().manual_seed(1)


def turn(sess, emb, keys, n_new, reset=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ids = sess.generate(emb, [keys], weights_version=0, reset_reason=reset, max_new_tokens=n_new, stop_ids=(), eos_id=-1,
                        min_length=0)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, ids


def ctx(n, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, cfg["vocab"], (n,), generator=g)
    emb = llama.embed[ids.to(dev)].float()[None].contiguous()
    return emb, [("t", int(t)) for t in ids]


def pool_bench(N):
    """3 turns of N conversations: the pool (one run_turns call per turn) against N sessions one after the other."""
    n_new, Q = a.tokens, 24
    kw = dict(max_new_tokens=n_new, stop_ids=(), eos_id=-1, min_length=0)
    dec = llama.slot_decoder(N, a.pool_context + 3 * (n_new + Q) + 2)
    sess = [DecodeSession(llama, a.pool_context + 3 * (n_new + Q) + 2) for _ in range(N)]     # kept, as a Chat keeps its own
    times = {"pool": [[], [], []], "sessions": [[], [], []]}
    for r in range(a.repeats + 1):                                   # repeat 0 warms both sides up (graph captures)
        first = [ctx(a.pool_context, 1000 * N + 10 * c + r) for c in range(N)]
        for mode in ("pool", "sessions"):
            state = [(e[0], list(k)) for e, k in first]
            for t in range(3):
                reset = "bench" if t == 0 else None                  # a new conversation: nothing of the last repeat is reused
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if mode == "pool":
                    got = {c: ids for c, ids, _ in dec.run_turns([(c, e, k, reset) for c, (e, k) in enumerate(state)], weights_version=0,
                                                                 prefill_batch=8, **kw)}
                else:
                    got = {c: sess[c].generate(e[None], [k], weights_version=0, reset_reason=reset, **kw)[0].cpu() for c, (e, k) in enumerate(state)}
                torch.cuda.synchronize()
                if r:
                    times[mode][t].append((time.perf_counter() - t0) * 1000.0)
                for c, (e, k) in enumerate(state):
                    q_emb, q_keys = ctx(Q, 7000 + 100 * c + 10 * t + r)
                    state[c] = (torch.cat([e, llama.embed[got[c].to(dev)].float(), q_emb[0]], 0).contiguous(),
                                k + [("t", int(i)) for i in got[c]] + q_keys)
            if mode == "pool":
                reused = [s["reused_tokens"] for s in dec.last_stats["turns"]]
    for mode in times:
        for t in range(3):
            ts = times[mode][t]
            emit(what="pool_turn_ms", mode=mode, conversations=N, turn=t + 1, first_context=a.pool_context, tokens=n_new,
                 ms=round(statistics.median(ts), 2), min=round(min(ts), 2), max=round(max(ts), 2),
                 **(dict(turn3_reused=reused[:2]) if mode == "pool" else {}))
    del dec, sess
    torch.cuda.empty_cache()


def pool_split_bench(N, context):
    """3 turns of N conversations through run_turns on two decoders of N slots, split_kv False and True, interleaved per repeat;
    then, on the cached third context, (a turn of n_new + 1 tokens) - (a turn of 1 token): both prefill one row."""
    n_new, Q = a.tokens, 24
    kw = dict(stop_ids=(), eos_id=-1, min_length=0, weights_version=0, prefill_batch=8)
    cap = context + 3 * (n_new + Q) + n_new + 4
    decs = {mode: llama.slot_decoder(N, cap, split_kv=mode) for mode in (False, True)}
    turn_ms = {mode: [[], [], []] for mode in decs}
    step_ms = {mode: [] for mode in decs}

    def timed(dec, turns, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = {c: ids for c, ids, _ in dec.run_turns(turns, max_new_tokens=n, **kw)}
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000.0, got

    for r in range(a.repeats + 1):                                   # repeat 0 warms both sides up (graph captures)
        first = [ctx(context, 1000 * N + 10 * c + r) for c in range(N)]
        for mode, dec in decs.items():
            state = [(e[0], list(k)) for e, k in first]
            for t in range(3):
                reset = ("bench",) if t == 0 else ()                 # a new conversation: nothing of the last repeat is reused
                ms, got = timed(dec, [(c, e, k) + reset for c, (e, k) in enumerate(state)], n_new)
                assert dec.last_stats["split_kv"] is mode
                if r:
                    turn_ms[mode][t].append(ms)
                if t < 2:
                    for c, (e, k) in enumerate(state):
                        q_emb, q_keys = ctx(Q, 7000 + 100 * c + 10 * t + r)
                        state[c] = (torch.cat([e, llama.embed[got[c].to(dev)].float(), q_emb[0]], 0).contiguous(),
                                    k + [("t", int(i)) for i in got[c]] + q_keys)
            turns = [(c, e, k) for c, (e, k) in enumerate(state)]    # the third context again: cached, one row prefilled
            t_one, _ = timed(dec, turns, 1)
            t_long, _ = timed(dec, turns, n_new + 1)
            assert all(s["prefilled_tokens"] == 1 for s in dec.last_stats["turns"])
            if r:
                step_ms[mode].append((t_long - t_one) / n_new)
    keys3 = state[0][0].shape[0]
    for mode in decs:
        for t in range(3):
            ts = turn_ms[mode][t]
            emit(what="pool_split_turn_ms", split_kv=mode, conversations=N, turn=t + 1, first_context=context, tokens=n_new,
                 ms=round(statistics.median(ts), 2), min=round(min(ts), 2), max=round(max(ts), 2))
        ts = step_ms[mode]
        emit(what="pool_split_step_ms", split_kv=mode, conversations=N, first_context=context, keys=keys3, tokens=n_new,
             ms=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))
    del decs
    torch.cuda.empty_cache()


def split_draft_turn_bench():
    """A turn of --tokens tokens on a cached context with no drafter, a taught one and an untaught one (see the module docstring)."""
    from myriad_amd.decode_host import NgramDrafter
    llama.slot_draft = llama.draft_split = True
    n_new, K, context = a.tokens, a.draft_k, a.pool_context
    cap = context + n_new + K + 8
    kw = dict(max_new_tokens=n_new, stop_ids=(), eos_id=-1, min_length=0, weights_version=0)
    cases = [("session", 1, True)] + [("pool", N, sk) for N in [int(x) for x in a.pool.split(",")] for sk in (True, False)]
    for kind, N, sk in cases:
        convs = [ctx(context, 4000 + c) for c in range(N)]
        if kind == "session":
            sess = DecodeSession(llama, cap, split=True)

            def run(**dkw):
                ids = sess.generate(convs[0][0], [convs[0][1]], **kw, **dkw)
                return [ids[0].tolist()], dict(sess.last_stats)
        else:
            dec = llama.slot_decoder(N, cap, split_kv=sk)

            def run(**dkw):
                got = {c: ids.tolist() for c, ids, _ in dec.run_turns([(c, e[0], k) for c, (e, k) in enumerate(convs)], prefill_batch=8,
                                                                      **kw, **dkw)}
                return [got[c] for c in range(N)], dict(dec.last_stats)
        run()                                                        # fills the caches: every later turn prefills one row ...
        ref, _ = run()                                               # ... and so repeats this one's ids
        modes = (("none", lambda: {}), ("taught", lambda: dict(draft=NgramDrafter(ref), draft_k=K)),
                 ("untaught", lambda: dict(draft=NgramDrafter(), draft_k=K)))
        ms, last = {m: [] for m, _ in modes}, {}
        for r in range(a.repeats + 1):                               # repeat 0 warms up (graph captures)
            for m, mk in modes:
                dkw = mk()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ids, st = run(**dkw)
                torch.cuda.synchronize()
                if r:
                    ms[m].append((time.perf_counter() - t0) * 1000.0)
                assert ids == ref, (kind, N, sk, m)
                last[m] = st
        for m, _ in modes:
            st = last[m]
            emit(what="split_draft_turn_ms", entry=kind, conversations=N, split_kv=bool(st["split_kv"]), drafter=m, draft_k=K if m != "none" else 0,
                 context=context, tokens=n_new, ms=round(statistics.median(ms[m]), 2), min=round(min(ms[m]), 2), max=round(max(ms[m]), 2),
                 steps=st["steps"], verify_steps=st.get("verify_steps", 0), draft_accepted=st.get("draft_accepted", 0),
                 draft_proposed=st.get("draft_proposed", 0), draft_off=st.get("draft_off"))
        if kind == "session":
            del sess
        else:
            del dec
        torch.cuda.empty_cache()


if a.split_draft:
    split_draft_turn_bench()
    sys.exit(0)

if a.pool_split:
    for context in [int(x) for x in a.pool_contexts.split(",")]:
        for N in [int(x) for x in a.pool.split(",")]:
            pool_split_bench(N, context)
    sys.exit(0)

if a.pool:
    for N in [int(x) for x in a.pool.split(",")]:
        pool_bench(N)
    sys.exit(0)

# ---- ms per token at a cached context of L keys: (turn of 1 + W + K tokens) - (turn of 1 token), both fully prefilled
for split in (True, False):
    sess = DecodeSession(llama, 2048 + a.tokens + 64 + 2, split=split)
    for L in [int(x) for x in a.contexts.split(",")]:
        emb, keys = ctx(L, L)
        turn(sess, emb, keys, a.tokens + 4, reset="bench")            # warm: captures the graph
        per = []
        for _ in range(a.repeats):
            t_long, _ = turn(sess, emb, keys, a.tokens + 1, reset="bench")
            t_one, _ = turn(sess, emb, keys, 1, reset="bench")
            per.append((t_long - t_one) / a.tokens * 1000.0)
        emit(what="ms_per_token", split_kv=sess.split, context=L, batch=1, layers=a.layers, ms=round(statistics.median(per), 3),
             runs=[round(x, 3) for x in per])
    del sess
    torch.cuda.empty_cache()

# ---- time to first token of turn 2: reuse vs full re-prefill
L1, A, Q = 1000, 32, 24
for mode in ("reuse", "full"):
    ttft = []
    for r in range(a.repeats):
        sess = DecodeSession(llama, 2000 + 300 + 2)
        emb1, keys1 = ctx(L1, 7 + r)
        _, ids = turn(sess, emb1, keys1, A)
        ans = ids[0].tolist()
        q_emb, q_keys = ctx(Q, 100 + r)
        emb2 = torch.cat([emb1, llama.embed[ids[0].to(dev)].float()[None], q_emb], 1).contiguous()
        keys2 = keys1 + [("t", t) for t in ans] + q_keys
        t, _ = turn(sess, emb2, keys2, 1, reset="bench" if mode == "full" else None)
        st = sess.last_stats
        ttft.append(t * 1000.0)
        del sess
    emit(what="turn2_ttft_ms", mode=mode, context=emb2.shape[1], reused=st["reused_tokens"], prefilled=st["prefilled_tokens"],
         split_kv=st["split_kv"], ms=round(statistics.median(ttft), 3), runs=[round(x, 3) for x in ttft])
