#!/usr/bin/env python3
"""Decode throughput of the full-size model: prefill + N single-token steps with KV cache.
python tools/decode_bench.py [--batch 1] [--new 32] [--sample] [--penalty P] [--modes greedy,host,device] [--repeats 5]
--sample: the chat call's do_sample=True, top_p=0.9, top_k=50 (drawn on the device when MYRIAD_DEVICE_SAMPLING=1, else on the
host); --modes times several decodes in one process, interleaved per repeat: greedy, host (sampled, host draw), device (sampled,
device draw), beam (num_beams = --beams, which also times greedy at batch * beams: the same row count), beam_sample (beam-search
multinomial sampling, top_p=0.9, top_k=50, behind the beam sampling switch); --penalty adds repetition_penalty to every mode but
beam.  --weights bf16,fp8,fp4 times each mode with the token step streaming bf16, FP8
and MXFP4 weight copies (LlamaHIP.decode_fp8 / decode_fp4), interleaved in the same way; without it the kind is the one
MYRIAD_DECODE_FP8 / MYRIAD_DECODE_FP4 set.  --merge 0,1 (with --lora 1)
times each of those with the bordered LoRA qkv product and with the LoRA merged into the step's qkv copy
(LlamaHIP.decode_merge_lora), interleaved again, and reports the one-time cost of packing every decoder matrix into each kind named by --weights and of merging every layer (bf16,
fp8 and fp4 copies).
--slots N measures a run instead of a call: a fixed synthetic request list (--requests of them, prompt lengths mixed between 24
and 160 rows, each answer's length between 8 and --new tokens forced by a stop id of its own) decoded three ways, interleaved per
repeat -- streamed through N decode slots (LlamaHIP.slot_decoder), greedy_generate at batch N over consecutive groups of N (the
row-0 rule: a group runs until its first request stops, later rows are cut or idle), and greedy_generate at batch 1 -- as
generated tokens per second and samples per second (the tokens each request is due, i.e. what batch 1 produces, count for all).
--prefill-batch 1,8 --refill-min 1,2,4 (with --slots) adds one slots mode per pair, interleaved with the others: the packed prefill
of SlotDecoder.run (prefill_batch = 1, refill_min = 1 is the one-request refill, the baseline).
--slots N --sample [--modes host,device] [--penalty P] times the sampled slots run instead (do_sample=True, top_p=0.9, top_k=50, one
generator seed per run), interleaved per repeat: host = the device sampling switch off, rows below top_p drawn on the host from the
shared generator; device = the switch on, every pick drawn inside the step from the request's own stream, with --penalty as its
repetition_penalty (the host mode has none: the switch is off there).  A sampled answer leaves the countdown chain, so requests
run to --new tokens or their stop id, whichever the draws meet first; the generated tokens are counted.  The chain's logits are
peaked (p_max >= 0.9 at temperature 1, so the host mode never draws there); --temperature T flattens them until rows fall below
top_p and the host mode draws them.
--slots 8,16,32,64 (a comma list) times the greedy slots run at each slot count in ONE process, interleaved per repeat, each with
the one-request refill and with every --prefill-batch / --refill-min pair; batch 1 runs once, as the answers every column must
reproduce.  Give it --requests 256 or more: one wave of 64 slots would otherwise be the whole run.
--step-rows 16,32,48,64 times the slot engine's captured token step alone, every row live at --step-keys cached keys, for each
kind of --weights, interleaved per repeat (--repeats rounds of --step-replays replays each): up to 16 rows the 16-row kernel,
above it ops.gemv_packed_wide.  --step-gemm 32,64 adds greedy_generate's step at those row counts: the row-major bf16 GEMMs that
every decode loop but the slot engine runs above 16 rows.
--slots 8,16,32 --num-beams 4 [--weights bf16,fp4] [--prefill-batch 1,8] times beam search in the slots (S / nb groups, one request
per group, behind llama.slot_beams) against beam_generate over consecutive batches of S / nb left-padded requests and at batch 1,
all interleaved per repeat; the stop id is then also the runner-up after every chain token, so that hypotheses finish.
With --sample [--penalty P] (or --penalty alone) both sides run beam sampling instead (do_sample=True, top_p=0.9, top_k=50,
--temperature; behind llama.beam_sampling as well): the sampled beam slots against beam_generate(do_sample=True) over the same
padded batches, and then the captured slot step alone, sampled against deterministic at the same rows, every group live at
--step-keys keys, --step-replays replays per round.

--scores (with --slots 8,64, the default there) measures what return_scores costs: the same request list decoded at batch 1 (the
first --requests / 8 requests), and through each slot count, with and without the token scores (two watched ids), interleaved per
repeat in one process, as run time and samples/s; then the captured token step of each of those views alone, every row live,
replayed --step-replays times per round from --step-keys keys (fewer where the view's cache is shorter); then mh_token_scores_rows alone at 1 and 64 rows of the model's
vocabulary.  min / median / max of both sides.

--draft-k 1,2,4,8 [--weights bf16,fp8,fp4] measures draft-and-verify decoding at batch 1: the captured K-row verify step at each
K beside the captured plain one-row step, replayed interleaved from --step-keys keys (--step-replays replays per round, median
of --repeats rounds; every guess is wrong, so each replay moves the position by one), with the kept-guess rate at which each K
breaks even; then greedy_generate end to end on a prompt of --step-keys rows and a countdown chain of --new tokens with a drafter
taught the chain, one whose guesses hold in every other window, and none -- the answer is asserted to be the chain each time.
--draft-k .. --split-kv: the same on the split-KV view (behind llama.draft_split): the verify step's attention is
mh_attn_decode_rope_split_draft, the plain step's mh_attn_decode_rope_split, and the end-to-end runs go through a
DecodeSession(split=True); give it --step-keys 1136 or 2160.

--slots S[,S..] --draft-k K[,K..] [--weights ..] measures draft decoding in the decode slots for every (S, K) with S * K <= 64
(with --sample --modes device, --penalty P and --scores also the verify and plain steps under the per-row tail, and the sampled runs),
interleaved in one process, medians of --repeats rounds: the captured verify step at S * K rows against the plain step at S and at
S * K slots (--step-keys keys, --step-replays replays per round) with the share of guesses kept at which it breaks even,
(t_verify / t_plain - 1) / (K - 1); the draft-rows attention launch alone against mh_attn_decode_rope_rows at 256 and 1,024 keys;
and samples/s on the --requests ragged countdown requests with no drafter and with one taught the chain, one right every other
time, and an untaught one -- every answer length is asserted."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from myriad_amd.myriad import MyriadHIP
from myriad_amd.synthetic import SyntheticWeights, full_config

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--new", type=int, default=32)
ap.add_argument("--llm-layers", type=int, default=32)
ap.add_argument("--lora", type=int, default=0, help="1: PEFT LoRA r = 8 on q_proj / v_proj attached (the fine-tuned model's generate)")
ap.add_argument("--sample", action="store_true", help="do_sample=True, top_p=0.9, top_k=50")
ap.add_argument("--penalty", type=float, default=1.0, help="repetition_penalty")
ap.add_argument("--temperature", type=float, default=1.0, help="with --slots --sample: the sampled run's temperature")
ap.add_argument("--modes", default="", help="comma list of greedy / host / device, timed interleaved in one process")
ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--beams", type=int, default=4, help="num_beams of the beam mode")
ap.add_argument("--weights", default="", help="comma list of bf16 / fp8 / fp4: the token step's weight copies, timed interleaved")
ap.add_argument("--slots", default="0", help="N > 0: the run-level comparison slots / batch N / batch 1; a comma list: the slots "
                "run at each count, interleaved (see above)")
ap.add_argument("--step-rows", default="", help="comma list of row counts: time the slot engine's token step alone at each")
ap.add_argument("--step-gemm", default="", help="with --step-rows: row counts at which greedy_generate's (row-major GEMM) step is timed too")
ap.add_argument("--step-keys", type=int, default=128, help="with --step-rows: cached keys per row when the timing starts")
ap.add_argument("--step-replays", type=int, default=40, help="with --step-rows: graph replays per timed round")
ap.add_argument("--requests", type=int, default=64, help="requests of the --slots run")
ap.add_argument("--num-beams", type=int, default=1, help="with --slots S[,S..]: beam search in the slots (S / nb groups, behind "
                "llama.slot_beams) against beam_generate over batches of S / nb padded prompts and at batch 1; --weights and "
                "--prefill-batch add their variants, all interleaved in one process")
ap.add_argument("--prefill-batch", default="1", help="comma list: prefill_batch of the --slots run, timed interleaved")
ap.add_argument("--refill-min", default="1", help="comma list: refill_min of the --slots run, timed interleaved")
ap.add_argument("--scores", action="store_true", help="the cost of return_scores: batch 1 and each --slots count, with and without")
ap.add_argument("--draft-k", default="", help="comma list of K (1..8): time the captured K-row verify step of draft decoding against the "
                "plain batch-1 step at --step-keys keys for each of --weights, interleaved, medians of --repeats rounds; then end-to-end "
                "tokens/s on a countdown chain of --new tokens with a drafter taught the chain, one that confirms half of its guesses, none")
ap.add_argument("--split-kv", action="store_true", help="with --draft-k (batch 1): the plain and the verify step of the split-KV view")
ap.add_argument("--merge", default="", help="comma list of 0 / 1: bordered / merged LoRA qkv in the token step, timed interleaved")
a = ap.parse_args()
# --slots is a string so that it can be a list; from here on a.slots is the single count (0: none or a list) and slot_counts the list
slot_counts = [int(x) for x in a.slots.split(",") if x]
if a.scores and slot_counts in ([], [0]):
    slot_counts = [8, 64]
a.slots = slot_counts[0] if len(slot_counts) == 1 else 0
modes = [m for m in a.modes.split(",") if m] or ["sample" if a.sample else "greedy"]
if "beam" in modes and "greedy" in modes:
    modes.append("greedy_x%d" % a.beams)             # greedy at batch * beams rows: the beam step's row count
kinds = [w for w in a.weights.split(",") if w] or [None]
assert all(w in (None, "bf16", "fp8", "fp4") for w in kinds), kinds
merges = [int(m) for m in a.merge.split(",") if m] or [None]
assert all(m in (None, 0, 1) for m in merges), merges
assert a.lora or merges == [None], "--merge needs --lora 1"
dev = "cuda:0"
cfg = full_config(llm_layers=a.llm_layers)
model = MyriadHIP(SyntheticWeights(cfg, dev, seed=0), dict(need_backward=False, use_lora=bool(a.lora)), device=dev)
model.eval()
g = torch.Generator().manual_seed(1)
B = a.batch


def make_samples(n):
    return dict(image=torch.randn(n, 3, 224, 224, generator=g), anomaly_maps=torch.rand(n, 1, 224, 224, generator=g),
                before_ids=torch.randint(3, 32000, (1, 4), generator=g).expand(n, -1).contiguous(),
                after_ids=torch.randint(3, 32000, (1, 28), generator=g).expand(n, -1).contiguous())


if a.draft_k and slot_counts not in ([], [0]):
    # Draft decoding in the decode slots, --slots S[,S..] --draft-k K[,K..], every (S, K) with S * K <= 64, everything interleaved in
    # this one process: (1) the captured verify step at S * K rows against the plain step at S and at S * K slots -- assembled from
    # the engine's own pieces (SlotDecoder._workspace / _draft_workspace, LlamaHIP._step_logits and the three-line tails of
    # _SlotRun.token_step / verify_token_step: copies, change them together); every guess is a random id that is never confirmed, so
    # pos moves by one per replay in all three; (2) the draft-rows attention launch alone against mh_attn_decode_rope_rows at 256
    # and 1,024 keys; (3) samples/s on the ragged countdown requests of the --slots run with the drafter taught, half right, untaught.
    from myriad_amd import ops
    from myriad_amd.decode_host import NgramDrafter
    L, D, new = model.llama, model.llama.D, a.new
    L.slot_draft = True                                              # the engine's switch (MYRIAD_SLOT_DRAFT), off by default
    Ks = [int(x) for x in a.draft_k.split(",") if x]
    pairs = [(S, K) for S in slot_counts for K in Ks if K > 1 and S * K <= ops.GEMV_WIDE_MAX_ROWS]
    rounds, n_rep = max(1, a.repeats) + 1, a.step_replays           # round 0 is the warm-up of the graphs themselves
    T_cap = 64 * ((max(a.step_keys, 160) + max(rounds * n_rep, new) + 16 + 63) // 64)
    gi, gq = torch.Generator().manual_seed(3), torch.Generator().manual_seed(11)
    lens = [int(x) for x in torch.randint(24, 161, (a.requests,), generator=gq)]
    due = [int(x) for x in torch.randint(8, new + 1, (a.requests,), generator=gq)]
    dirs = torch.nn.functional.normalize(torch.randn(new + 1, D, generator=gq), dim=1)      # the countdown chain of the --slots run
    emb_rows = dirs * (D ** 0.5) * 2.0
    L.embed[1000:1001 + new].copy_(emb_rows.to(L.embed.dtype).to(dev))
    head = L.lm_head[1000:1001 + new].float().cpu()
    head[:new] += 2.5 * dirs[1:]
    L.lm_head[1000:1001 + new].copy_(head.to(L.lm_head.dtype).to(dev))
    reqs = []
    for n, d in zip(lens, due):
        x = torch.randn(n, D, generator=gq) * 0.02
        x[-1] = emb_rows[d]
        reqs.append(x.to(dev))
    chain = list(range(1000 + new - 1, 999, -1))
    kw = dict(max_new_tokens=new, stop_ids=((1000,),), eos_id=-5, min_length=0)
    wkinds = kinds if kinds != [None] else ["bf16"]

    class Half:
        """Every other call's guesses are the chain's, the others are wrong: about half of the guesses are confirmed."""
        def __init__(self):
            self.good, self.n = NgramDrafter([chain]), 0

        def propose(self, history, k):
            self.n += 1
            return self.good.propose(history, k) if self.n % 2 else [7] * k

    def set_kind(kind):
        L.decode_fp8, L.decode_fp4 = kind == "fp8", kind == "fp4"

    def capture(step):
        step()                                                       # eager once: kernels loaded, attributes set
        torch.cuda.synchronize()
        g_ = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_):
            step()
        return g_

    decs, steps, keep = {}, [], []                                   # (kind, S, K or 0, rows, graph, reset[, tail tag])
    # the per-row tails to time beside the greedy steps: tag -> (device-sampled, penalty, scores)
    from myriad_amd.decode import _SlotRun
    dev_mode, inv_temp_t = a.sample and "device" in modes, 1.0 / a.temperature
    tails = {}
    if dev_mode:
        tails["sampler"] = (True, False, False)
    if dev_mode and a.penalty != 1.0:
        tails["sampler+penalty"] = (True, True, False)
    if a.scores:
        tails["sampler+scores" if dev_mode else "scores"] = (dev_mode, False, True)
    if tails:
        L.device_sampling = L.draft_sampling = True
    for kind in wkinds:
        set_kind(kind)
        for S in dict.fromkeys([S for S, _ in pairs] + [S * K for S, K in pairs]):
            dec = decs[kind, S] = L.slot_decoder(S, T_cap)
            ws = dec._workspace(1.0)
            for c in ws["caches"]:
                c[:, :a.step_keys].normal_(0.0, 0.5)

            def reset(ws=ws, S=S):
                ws["ids"].copy_(torch.randint(3, 32000, (S,), generator=gi))
                ws["live"].fill_(1)
                ws["pos"].fill_(a.step_keys)
                ws["kvlen"].fill_(a.step_keys + 1)

            def plain(ws=ws):
                L._step_logits(ws)
                ops.argmax_pmax_rows(ws["logits"], ws["nxt"], ws["mar"], ws["pmx"], ban_id=-1, inv_temp=1.0)
                ops.decode_advance_rows(ws["nxt"], ws["mar"], ws["pmx"], ws["rec"][:3], ws["ids"], ws["step"], ws["pos"], ws["kvlen"],
                                        ws["live"])
            reset()
            steps.append((kind, S, 0, S, capture(plain), reset))
            for K in [K for S_, K in pairs if S_ == S]:
                dv = dec._draft_workspace(K, 1.0)

                def vreset(dv=dv, reset=reset, K=K):
                    reset()
                    dv["ids"].copy_(torch.randint(3, 32000, (dv["ids"].shape[0],), generator=gi))
                    dv["nguess"].fill_(K - 1)
                    dv["nrow"].fill_(K)

                def verify(dv=dv, K=K):
                    L._step_logits(dv)
                    ops.argmax_pmax_rows(dv["logits"], dv["nxt"], dv["mar"], dv["pmx"], ban_id=-1, inv_temp=1.0)
                    ops.draft_accept_rows(dv["nxt"], dv["mar"], dv["pmx"], dv["ids"], dv["next_ids"], dv["nguess"], dv["live"], dv["top_p"],
                                          dv["drec"], dv["pos"], dv["kvlen"], dv["step"], K)
                vreset()
                steps.append((kind, S, K, S * K, capture(verify), vreset))
            # the same two steps under the per-row tail (--sample --modes device, --penalty P, --scores; behind draft_sampling): the
            # engine's own _SlotRun.token_step / verify_token_step on its own views, so nothing is copied here
            for tag, (dv_s, pen, sc) in tails.items():
                if S not in [S_ for S_, _ in pairs]:
                    continue
                ws_t = dec._workspace(inv_temp_t, (dv_s, pen), False, sc)
                srun = _SlotRun(dec, ws_t, None, {}, None, max_new_tokens=new, eos_id=-5, min_length=0, do_sample=dv_s, top_p=0.9,
                                inv_temp=inv_temp_t, top_k=50, dev_sample=dv_s, penalty=pen, rows_tail=True, generator=None, scores=sc, W=0)

                def treset(ws=ws_t, reset=reset, S=S):
                    reset()
                    ws["prm"].copy_(torch.tensor([inv_temp_t, 0.9, 50.0, a.penalty, 0.0, -5.0]))
                    ws["seed"].copy_(torch.randint(0, 2**62, (S,), generator=gi))
                    ws["gen"].fill_(1)
                    ws["seen"].copy_(torch.randint(-2**31, 2**31 - 1, ws["seen"].shape, generator=gi, dtype=torch.int64).to(torch.int32)
                                     & torch.randint(-2**31, 2**31 - 1, ws["seen"].shape, generator=gi, dtype=torch.int64).to(torch.int32)
                                     & 0x01010101)                   # about 1 id in 128 seen
                treset()
                steps.append((kind, S, 0, S, capture(lambda srun=srun: srun.token_step(-1)), treset, tag))
                keep.append(srun)
                for K in [K for S_, K in pairs if S_ == S]:
                    vrun = _SlotRun(dec, ws_t, None, {}, None, **{k_: getattr(srun, k_) for k_ in (
                        "max_new_tokens", "eos_id", "min_length", "do_sample", "top_p", "inv_temp", "top_k", "dev_sample", "penalty",
                        "rows_tail", "generator", "scores", "W")})
                    dv = vrun.dv = dec._draft_workspace(K, inv_temp_t, (dv_s, pen, True, sc))

                    def tvreset(dv=dv, treset=treset, K=K):
                        treset()
                        dv["ids"].copy_(torch.randint(3, 32000, (dv["ids"].shape[0],), generator=gi))
                        dv["nguess"].fill_(K - 1)
                        dv["nrow"].fill_(K)
                    tvreset()
                    steps.append((kind, S, K, S * K, capture(lambda vrun=vrun: vrun.verify_token_step(-1)), tvreset, tag))
                    keep.append(vrun)
    # the attention launches alone: one graph of 16 launches each (q is rotated in place again and again: the time does not care)
    attn, W, scale = [], L.H * L.hd, 1.0 / L.hd ** 0.5
    i32 = lambda v, n: torch.full((n,), v, dtype=torch.int32, device=dev)
    for keys in (256, 1024):
        for S, K in pairs:
            R, T = S * K, keys + 64
            qkv = (torch.randn(R, 3 * W, device=dev) * 0.5).to(torch.bfloat16)
            cache_s = (torch.randn(S, T, 2 * W, device=dev) * 0.5).to(torch.bfloat16)
            cache_r = cache_s.repeat(K, 1, 1)
            pos_s, pos_r, kv_r, one_s, one_r, nrow = i32(keys, S), i32(keys, R), i32(keys + 1, R), i32(1, S), i32(1, R), i32(K, S)
            out = torch.empty((R, W), dtype=torch.bfloat16, device=dev)

            def draft_rows(qkv=qkv, c=cache_s, p=pos_s, lv=one_s, nr=nrow, K=K, out=out):
                for _ in range(16):
                    ops.attn_decode_rope_draft_rows(qkv, c, p, lv, nr, L.cos, L.sin, L.H, L.hd, scale, K, out=out)

            def rows(qkv=qkv, c=cache_r, p=pos_r, kv=kv_r, lv=one_r):
                for _ in range(16):
                    ops.attn_decode_rope_rows(qkv, c, p, kv, lv, L.cos, L.sin, L.H, L.hd, scale)
            attn += [(keys, S, K, "draft_rows", capture(draft_rows)), (keys, S, K, "rows", capture(rows))]
            keep += [draft_rows, rows]                               # the graphs read these closures' tensors: they must outlive them
    res, ares = {i: [] for i in range(len(steps))}, {i: [] for i in range(len(attn))}
    for rnd in range(rounds):
        for table, out_, per, reps in ((steps, res, n_rep, n_rep), (attn, ares, 16 * 8, 8)):
            for i, cfg_ in enumerate(table):
                if table is steps:
                    cfg_[5]()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    cfg_[4].replay()
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    out_[i].append(e0.elapsed_time(e1) / per)
    med = lambda ts: sorted(ts)[len(ts) // 2]
    t_of = {(kind, S, K) + tuple(st_[6:]): med(res[i]) for i, st_ in enumerate(steps) for kind, S, K in [st_[:3]]}
    print(f"slot token steps, every row live, {a.step_keys}+ keys, {len(L.layers)} layers; median of {rounds - 1} rounds of {n_rep} replays")
    for kind in wkinds:
        for S, K in pairs:
            tv, tp, tw = t_of[kind, S, K], t_of[kind, S, 0], t_of[kind, S * K, 0]
            print(f"weights {kind} slots {S} K={K} ({S * K} rows): verify {tv:.3f} ms, plain {S}-row {tp:.3f} ms, plain {S * K}-row {tw:.3f} ms; "
                  f"verify / plain = {tv / tp:.3f}, verify / plain at {S * K} rows = {tv / tw:.3f}; breaks even at "
                  f"{(tv / tp - 1) / (K - 1):.3f} of the guesses kept")
            for tag in tails:                                        # against the greedy verify step and the tail's own plain step
                tt, tpt = t_of[kind, S, K, tag], t_of[kind, S, 0, tag]
                print(f"weights {kind} slots {S} K={K} {tag}: verify {tt:.3f} ms = {tt / tv:.3f} x the greedy verify step, {tt / tpt:.3f} x "
                      f"its plain step ({tpt:.3f} ms); breaks even at {(tt / tpt - 1) / (K - 1):.3f} of the guesses kept")
    print("attention launch alone, every row live; median of the same rounds, 128 launches each")
    for i in range(0, len(attn), 2):
        keys, S, K = attn[i][:3]
        td, tr = med(ares[i]), med(ares[i + 1])
        print(f"keys {keys} slots {S} K={K}: draft_rows {td * 1e3:.1f} us, rope_rows at {S * K} rows {tr * 1e3:.1f} us, ratio {td / tr:.3f}")
    # ---- end to end: the ragged requests through the slots
    e2e, modes_ = {}, [("none", None, 0)] + [(name, mk, K) for name, mk in (("taught", lambda: NgramDrafter([chain])), ("half", Half),
                                                                             ("untaught", NgramDrafter))
                                             for K in dict.fromkeys(K for _, K in pairs)]
    for rnd in range(rounds):
        for kind in wkinds:
            set_kind(kind)
            for S in dict.fromkeys(S for S, _ in pairs):
                for name, mk, K in modes_:
                    if K and (S, K) not in pairs:
                        continue
                    dkw = {} if mk is None else dict(draft=mk(), draft_k=K)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got = {i: len(ids) for i, ids, _ in decs[kind, S].run(reqs, **kw, **dkw)}
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    assert [got[i] for i in range(len(reqs))] == due, (name, S, K)
                    if rnd:
                        st = decs[kind, S].last_stats
                        e2e.setdefault((kind, S, name, K), []).append((dt, st["steps"], st.get("verify_steps", 0), st.get("draft_accepted", 0),
                                                                       st.get("draft_proposed", 0)))
    print(f"end to end, {len(reqs)} requests, prompts {min(lens)}..{max(lens)} rows, answers {min(due)}..{max(due)} tokens (prefills "
          f"included); median of {rounds - 1}")
    for (kind, S, name, K), rs in e2e.items():
        rs.sort()
        dt, st_, vs, acc, prop = rs[len(rs) // 2]
        print(f"weights {kind} slots {S} drafter {name}{f' K={K}' if K else ''}: {len(reqs) / dt:.1f} samples/s ({dt * 1e3:.0f} ms, min "
              f"{rs[0][0] * 1e3:.0f}, max {rs[-1][0] * 1e3:.0f}; {st_} steps, {vs} verify; {acc} of {prop} guesses kept)")
    # ---- the same requests sampled on the device (and with the penalty): the drafter is taught the sampled answers of the run
    # without it -- same seeds, so the answers with a drafter must be those, which is checked
    for tag, (dv_s, pen, sc) in tails.items():
        if not dv_s or sc:
            continue
        skw = dict(kw, do_sample=True, top_p=0.9, top_k=50, temperature=a.temperature, repetition_penalty=a.penalty if pen else 1.0)
        e2s = {}
        for kind in wkinds:
            set_kind(kind)
            for S in dict.fromkeys(S for S, _ in pairs):
                ref_ids = {i: ids.tolist() for i, ids, _ in decs[kind, S].run(reqs, seeds=range(len(reqs)), **skw)}
                taught = [ref_ids[i] for i in range(len(reqs))]

                class HalfS(Half):
                    def __init__(self):
                        self.good, self.n = NgramDrafter(taught), 0
                for rnd in range(rounds):
                    for name, mk, K in [("none", None, 0)] + [(n_, m_, K) for n_, m_ in (("taught", lambda: NgramDrafter(taught)), ("half", HalfS))
                                                              for K in dict.fromkeys(K for S_, K in pairs if S_ == S)]:
                        dkw = {} if mk is None else dict(draft=mk(), draft_k=K)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        got = {i: ids.tolist() for i, ids, _ in decs[kind, S].run(reqs, seeds=range(len(reqs)), **skw, **dkw)}
                        torch.cuda.synchronize()
                        dt = time.perf_counter() - t0
                        assert got == ref_ids, (tag, name, S, K)
                        if rnd:
                            st = decs[kind, S].last_stats
                            e2s.setdefault((kind, S, name, K), []).append((dt, st["steps"], st.get("verify_steps", 0),
                                                                           st.get("draft_accepted", 0), st.get("draft_proposed", 0)))
        print(f"end to end, {tag} (top_p 0.9, top_k 50, temperature {a.temperature}, penalty {a.penalty if pen else 1.0}); median of {rounds - 1}")
        for (kind, S, name, K), rs in e2s.items():
            rs.sort()
            dt, st_, vs, acc, prop = rs[len(rs) // 2]
            print(f"weights {kind} slots {S} {tag} drafter {name}{f' K={K}' if K else ''}: {len(reqs) / dt:.1f} samples/s ({dt * 1e3:.0f} ms, "
                  f"min {rs[0][0] * 1e3:.0f}, max {rs[-1][0] * 1e3:.0f}; {st_} steps, {vs} verify; {acc} of {prop} guesses kept)")
    L.decode_fp8 = L.decode_fp4 = False
    sys.exit(0)

if a.draft_k:
    # The verify step is assembled from the loop's own pieces (_draft_view for the buffers, LlamaHIP._step_logits, the arg-max and
    # mh_draft_accept tail of LlamaHIP._draft_core's verify_token_step): a copy of its three lines -- change them together.  Every
    # guess is id 0 and never confirmed, so pos moves by one per replay, as in the plain step beside it.
    from myriad_amd import ops
    from myriad_amd.decode_host import NgramDrafter
    from myriad_amd.decode import DecodeSession, _buffer_view, _decode_buffers, _draft_view
    L = model.llama
    L.draft_split = bool(a.split_kv)                                 # the switch (MYRIAD_DRAFT_SPLIT), off by default
    Ks = [int(x) for x in a.draft_k.split(",") if x]
    rounds, n_rep = max(1, a.repeats) + 1, a.step_replays           # round 0 is the warm-up of the graph itself
    T_cap = 64 * ((a.step_keys + rounds * n_rep + 16 + 63) // 64)
    if T_cap > L.cos.shape[0]:                                       # a longer rotary table (the model's default holds 2,048 positions)
        fr = torch.einsum("i,j->ij", torch.arange(T_cap).float(), 1.0 / (10000.0 ** (torch.arange(0, L.hd, 2).float() / L.hd)))
        L.cos, L.sin = fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)
    gi = torch.Generator().manual_seed(3)
    # the countdown chain of the end-to-end runs below (token 1000+k is followed by 1000+k-1, 1000 stops), written into the
    # embedding / lm-head rows before any packed copy of them is made
    new, D = a.new, L.D
    gq = torch.Generator().manual_seed(11)
    dirs = torch.nn.functional.normalize(torch.randn(new + 1, D, generator=gq), dim=1)
    emb_rows = dirs * (D ** 0.5) * 2.0
    L.embed[1000:1001 + new].copy_(emb_rows.to(L.embed.dtype).to(dev))
    head = L.lm_head[1000:1001 + new].float().cpu()
    head[:new] += 2.5 * dirs[1:]
    L.lm_head[1000:1001 + new].copy_(head.to(L.lm_head.dtype).to(dev))
    configs, keep = [], []                                           # (kind, K or 0 = plain, graph, reset)
    for kind in (kinds if kinds != [None] else ["bf16"]):
        L.decode_fp8, L.decode_fp4 = kind == "fp8", kind == "fp4"
        L._prepare_decode_weights(1)
        ws = _decode_buffers(L, 1, T_cap)
        if a.split_kv:
            ws = _buffer_view(L, ws, True)
        for c in ws["caches"]:
            c[:, :a.step_keys].normal_(0.0, 0.5)

        def reset(ws=ws):
            ws["ids_k"].copy_(torch.randint(3, 32000, (8,), generator=gi))
            ws["pos"].fill_(a.step_keys)
            ws["kvlen"].fill_(a.step_keys + 1)

        def plain(ws=ws):
            L._step_logits(ws)
            ops.argmax_pmax_rows(ws["logits"], ws["nxt"], ws["mar"], ws["pmx"], ban_id=-1, inv_temp=1.0)
            ops.decode_advance(ws["nxt"], ws["mar"], ws["pmx"], ws["rec"][:3], ws["ids"], ws["step"], ws["pos"], ws["kvlen"])

        steps = [(0, plain)]
        for K in Ks:
            dv = _draft_view(L, ws, K, 1.0, None, a.split_kv)

            def verify(dv=dv, ws=ws, K=K):
                L._step_logits(dv)
                ops.argmax_pmax_rows(dv["logits"], dv["nxt"], dv["mar"], dv["pmx"], ban_id=-1, inv_temp=1.0)
                ops.draft_accept(dv["nxt"], dv["mar"], dv["pmx"], dv["ids"], dv["top_p"], dv["drec"], ws["pos"], ws["kvlen"], ws["step"], K)
            steps.append((K, verify))
        for K, step in steps:
            reset()
            step()                                                   # eager once: kernels loaded, attributes set
            torch.cuda.synchronize()
            g_ = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_):
                step()
            configs.append((kind, K, g_, reset))
        keep.append(ws)
    res = {i: [] for i in range(len(configs))}
    for rnd in range(rounds):
        for i, (_, _, g_, reset) in enumerate(configs):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n_rep):
                g_.replay()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                res[i].append(e0.elapsed_time(e1) / n_rep)
    print(f"batch-1 token step{' on the split-KV view' if a.split_kv else ''}, {a.step_keys}+ keys, {len(L.layers)} layers; median of {rounds - 1} rounds of {n_rep} replays")
    base = {}
    for i, (kind, K, _, _) in enumerate(configs):
        ts = sorted(res[i])
        t = ts[len(ts) // 2]
        if K == 0:
            base[kind] = t
            print(f"weights {kind} plain step: {t:.3f} ms (min {ts[0]:.3f}, max {ts[-1]:.3f})")
        else:                                                        # break-even: mean tokens per verify step that pays for it
            print(f"weights {kind} verify step K={K}: {t:.3f} ms (min {ts[0]:.3f}, max {ts[-1]:.3f}), {t / base[kind]:.3f}x the plain step; "
                  f"all {K} kept: {t / K:.3f} ms/token; breaks even at {t / base[kind]:.2f} tokens/step"
                  + (f" = {(t / base[kind] - 1) / (K - 1):.2f} of the guesses kept" if K > 1 else ""))
    # ---- end to end: greedy_generate at batch 1 on the countdown chain
    x = torch.randn(1, a.step_keys, D, generator=gq) * 0.02
    x[0, -1] = emb_rows[new]
    x = x.to(dev)
    kw = dict(max_new_tokens=new, stop_ids=((1000,),), eos_id=-5, min_length=0)
    chain = list(range(1000 + new - 1, 999, -1))

    class Half:
        """Every other window's guesses are the chain's, the others are wrong: half of the guesses are confirmed."""
        def __init__(self):
            self.good, self.n = NgramDrafter([chain]), 0

        def propose(self, history, k):
            self.n += 1
            return self.good.propose(history, k) if self.n % 2 else [7] * k

    # a session per kind of weights: a change of the decode weights drops a session's cache and graphs, which would charge a
    # capture to the first run after every switch
    sessions = {} if a.split_kv else None
    x_keys = [[("r", j) for j in range(a.step_keys)]]
    e2e = {}
    drafters = [("none", None)] + [(f"{name} K={K}", mk) for K in Ks if K > 1 for name, mk in (("taught", lambda: NgramDrafter([chain])), ("half", Half))]
    for rnd in range(rounds):
        for kind in (kinds if kinds != [None] else ["bf16"]):
            L.decode_fp8, L.decode_fp4 = kind == "fp8", kind == "fp4"
            for label, mk in drafters:
                dkw = {} if mk is None else dict(draft=mk(), draft_k=int(label.split("=")[1]))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if sessions is not None and kind not in sessions:
                    sessions[kind] = DecodeSession(L, a.step_keys + new + 16, split=True)
                sess = None if sessions is None else sessions[kind]
                if sess is None:
                    ids = L.greedy_generate(x, **kw, **dkw)
                else:                                                # a chat turn: every repeat prefills the whole context
                    ids = sess.generate(x, x_keys, weights_version=0, reset_reason="bench", **kw, **dkw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert ids[0].tolist() == chain, (label, ids)
                if rnd:
                    st = L.last_generate_stats
                    assert sess is None or (sess.last_stats["split_kv"] and st.get("draft_off") is None)
                    e2e.setdefault((kind, label), []).append((dt, st.get("verify_steps", 0), st.get("plain_steps", st["steps"] - 1),
                                                              st.get("draft_accepted", 0), st.get("draft_proposed", 0)))
    print(f"end to end, batch 1, prompt {a.step_keys} rows + {new} tokens of the countdown chain (prefill included); median of {rounds - 1}")
    for (kind, label), rs in e2e.items():
        rs.sort()
        dt, vs, ps, acc, prop = rs[len(rs) // 2]
        print(f"weights {kind} drafter {label}: {new / dt:.1f} tok/s ({dt * 1e3:.1f} ms; {vs} verify + {ps} plain steps; "
              f"{acc} of {prop} guesses kept)")
    L.decode_fp8 = L.decode_fp4 = False
    sys.exit(0)

if a.step_rows:
    # The timed step is assembled here from the engine's own pieces (SlotDecoder._workspace for the buffers and weights,
    # LlamaHIP._step_logits, the plain arg-max + mh_decode_advance_rows tail of SlotDecoder.run's greedy token_step): the same
    # launches as the step run() captures, but a copy of its three lines -- if run()'s greedy tail changes, change it here too.
    from myriad_amd import ops
    from myriad_amd.llama import _decode_buffers
    L = model.llama
    rows_list = [int(x) for x in a.step_rows.split(",") if x]
    gemm_rows = [int(x) for x in a.step_gemm.split(",") if x]
    rounds, n_rep = max(1, a.repeats) + 1, a.step_replays           # round 0 is the warm-up of the graph itself
    T_cap = 64 * ((a.step_keys + rounds * n_rep + 8 + 63) // 64)
    gi = torch.Generator().manual_seed(3)

    def capture(ws, step):
        R = ws["ids"].shape[0]
        ws["ids"].copy_(torch.randint(3, 32000, (R,), generator=gi))
        ws["pos"].fill_(a.step_keys)
        ws["kvlen"].fill_(a.step_keys + 1)
        for c in ws["caches"]:
            c[:, :a.step_keys].normal_(0.0, 0.5)
        step()                                                       # eager once: kernels loaded, attributes set
        torch.cuda.synchronize()
        g_ = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_):
            step()
        return g_

    configs = []                                                     # (label, kind, rows, graph)
    keep = []
    for kind in (kinds if kinds != [None] else ["bf16"]):
        L.decode_fp8, L.decode_fp4 = kind == "fp8", kind == "fp4"
        for R in rows_list:
            dec = L.slot_decoder(R, T_cap)
            ws = dec._workspace(1.0)
            ws["live"].fill_(1)

            def step(ws=ws):
                L._step_logits(ws)
                ops.argmax_pmax_rows(ws["logits"], ws["nxt"], ws["mar"], ws["pmx"], ban_id=-1, inv_temp=1.0)
                ops.decode_advance_rows(ws["nxt"], ws["mar"], ws["pmx"], ws["rec"][:3], ws["ids"], ws["step"], ws["pos"], ws["kvlen"],
                                        ws["live"])
            configs.append((f"slots step, weights {kind}", kind, R, capture(ws, step)))
            keep.append((dec, ws))
    L.decode_fp8 = L.decode_fp4 = False
    for R in gemm_rows:                                              # greedy_generate's step: row-major GEMMs above 16 rows
        L._prepare_decode_weights(R)
        ws = _decode_buffers(L, R, T_cap)

        def step(ws=ws):
            L._step_logits(ws)
            ops.argmax_pmax_rows(ws["logits"], ws["nxt"], ws["mar"], ws["pmx"], ban_id=-1, inv_temp=1.0)
            ops.decode_advance(ws["nxt"], ws["mar"], ws["pmx"], ws["rec"][:3], ws["ids"], ws["step"], ws["pos"], ws["kvlen"])
        configs.append(("greedy step, row-major bf16 GEMM", "bf16", R, capture(ws, step)))
        keep.append((None, ws))
    res = {i: [] for i in range(len(configs))}
    for rnd in range(rounds):
        for i, (_, _, _, g_) in enumerate(configs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n_rep):
                g_.replay()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                res[i].append(e0.elapsed_time(e1) / n_rep)
    base = {}
    print(f"token step, every row live, {a.step_keys}+ keys, {len(L.layers)} layers; median of {rounds - 1} rounds of {n_rep} replays")
    for i, (label, kind, R, _) in enumerate(configs):
        ts = sorted(res[i])
        t = ts[len(ts) // 2]
        if label.startswith("slots") and R == 16:
            base[kind] = t
        ratio = ""
        if label.startswith("slots") and kind in base and R > 16:
            ratio = f"; {t / base[kind]:.3f}x the 16-row step, R/16 = {R / 16:.2f} -> ratio to R/16: {t / base[kind] / (R / 16):.3f}"
        print(f"{label} rows {R}: {t:.3f} ms/step (min {ts[0]:.3f}, max {ts[-1]:.3f}), {R / t * 1e3:.0f} row-tok/s{ratio}")
    sys.exit(0)

if a.slots or len(slot_counts) > 1 or a.scores:
    L, N, new = model.llama, a.slots or slot_counts[0], a.new
    gq = torch.Generator().manual_seed(11)
    lens = [int(x) for x in torch.randint(24, 161, (a.requests,), generator=gq)]
    due = [int(x) for x in torch.randint(8, new + 1, (a.requests,), generator=gq)]
    # Answer lengths are forced by a countdown chain written into the embedding / lm-head rows of ids 1000..1000+new (the
    # peaked construction of tests/golden_utils.decode_chain_weights): token 1000+k is followed by 1000+k-1 with a margin of
    # several logits, and 1000 is the stop id.  A prompt whose last row is the embedding of 1000+d answers d tokens, then stops.
    D = L.D
    dirs = torch.nn.functional.normalize(torch.randn(new + 1, D, generator=gq), dim=1)
    emb_rows = (dirs * (D ** 0.5) * 2.0)
    L.embed[1000:1001 + new].copy_(emb_rows.to(L.embed.dtype).to(dev))
    head = L.lm_head[1000:1001 + new].float().cpu()
    head[:new] += 2.5 * dirs[1:]
    L.lm_head[1000:1001 + new].copy_(head.to(L.lm_head.dtype).to(dev))
    reqs = []
    for n, d in zip(lens, due):
        x = torch.randn(n, D, generator=gq) * 0.02
        x[-1] = emb_rows[d]
        reqs.append(x.to(dev))
    kw = dict(max_new_tokens=new, stop_ids=((1000,),), eos_id=-5, min_length=0)
    if a.num_beams > 1:
        # Beams need hypotheses that finish: the stop id is also the runner-up after every chain token, so the pool fills while
        # the chain counts down and a search ends soon after its chain does -- requests end at their own lengths, as above.
        nb = a.num_beams
        head = L.lm_head[1000:1001].float().cpu()
        head[0] += 2.0 * dirs[2:].sum(0)
        L.lm_head[1000:1001].copy_(head.to(L.lm_head.dtype).to(dev))
        L.slot_beams = True
        cap = 64 * ((160 + new + 2 + 63) // 64)
        decs = {(n, kind): L.slot_decoder(n, cap) for n in slot_counts for kind in kinds}     # a kind's graphs stay its own
        bkw = dict(kw, num_beams=nb)
        stats = {}
        sampled = a.sample or a.penalty != 1.0                     # beam sampling / the penalty under beams, on both sides
        skw = {}
        if sampled:
            L.beam_sampling = True
            skw = dict(do_sample=a.sample, top_p=0.9, top_k=50, temperature=a.temperature, repetition_penalty=a.penalty)

        def gen_kw():                                              # the same seeds every repeat: the same work every repeat
            return dict(generator=torch.Generator().manual_seed(0)) if a.sample else {}

        def set_kind(kind):
            L.decode_fp8, L.decode_fp4 = kind == "fp8", kind == "fp4"

        def beam_slots(n, kind, pb):
            set_kind(kind)
            out = {i: lens_ for i, _, _, lens_ in decs[n, kind].run(reqs, prefill_batch=pb, **bkw, **skw, **gen_kw())}
            stats[(n, kind, pb)] = dict(decs[n, kind].last_stats)
            return [out[i][0] for i in range(len(reqs))]

        def beam_batch(n, kind):
            set_kind(kind)
            got, steps = [], 0
            for g0 in range(0, len(reqs), n):
                grp = reqs[g0:g0 + n]
                S = max(x.shape[0] for x in grp)                   # one stacked prompt per group: left-pad with the first row
                emb = torch.stack([torch.cat([x[:1].expand(S - x.shape[0], -1), x]) for x in grp])
                L.beam_generate(emb, nb, **kw, **skw, **gen_kw())
                got += L.last_generate_stats["lengths"]
                steps += L.last_generate_stats["steps"]
            stats[("batch", n, kind)] = dict(steps=steps)
            return got

        pbs = [int(x) for x in a.prefill_batch.split(",")]
        bmodes = []
        for kind in kinds:
            for n in slot_counts:
                G = n // nb
                bmodes += [(f"beam slots {n} ({G} groups) prefill_batch {pb} weights {kind or 'bf16'}", (n, kind, pb),
                            lambda n=n, kind=kind, pb=pb: beam_slots(n, kind, pb)) for pb in pbs]
                bmodes.append((f"beam_generate batch {G} weights {kind or 'bf16'}", ("batch", G, kind),
                               lambda G=G, kind=kind: beam_batch(G, kind)))
            bmodes.append((f"beam_generate batch 1 weights {kind or 'bf16'}", ("batch", 1, kind), lambda kind=kind: beam_batch(1, kind)))
        for _, _, fn in bmodes:
            fn()                                                   # warm-up: kernels, graphs, packed copies
        print("warm-up done", file=sys.stderr, flush=True)
        res = {name: [] for name, _, _ in bmodes}
        for rep in range(max(1, a.repeats)):
            for name, _, fn in bmodes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = fn()
                torch.cuda.synchronize()
                res[name].append((time.perf_counter() - t0, got))
            print(f"repeat {rep + 1} of {max(1, a.repeats)} done", file=sys.stderr, flush=True)
        mode = (f", {'sampled top_p 0.9 top_k 50 temperature %g' % a.temperature if a.sample else 'deterministic'}"
                f"{' penalty %g' % a.penalty if a.penalty != 1.0 else ''}") if sampled else ""
        print(f"{len(reqs)} requests, prompts {min(lens)}..{max(lens)} rows, num_beams {nb}, max_new_tokens {new}{mode}")
        for name, key, _ in bmodes:
            ts = sorted(t for t, _ in res[name])
            t, got, st = ts[len(ts) // 2], res[name][-1][1], stats[key]
            tail = (f"; group occupancy {st['occupancy']:.3f}, {st['prefills']} prefills in {st['prefill_passes']} passes, "
                    f"{st['graph_replays']} replays") if "occupancy" in st else ""
            print(f"{name}: {t * 1e3:.1f} ms (median of {len(ts)}, min {ts[0] * 1e3:.1f}, max {ts[-1] * 1e3:.1f}) -> "
                  f"{len(reqs) / t:.2f} samples/s; {st['steps']} steps, {t * 1e3 / st['steps']:.3f} ms per step incl. prefills; best "
                  f"hypothesis {min(got)}..{max(got)} tokens, mean {sum(got) / len(got):.1f}{tail}")
        if sampled:
            # the captured slot step alone, sampled against deterministic at the same rows: every group live, identity parents,
            # reset to --step-keys keys before each round
            views = []
            for kind in kinds:
                for n in slot_counts:
                    set_kind(kind)
                    list(decs[n, kind].run(reqs[:2 * (n // nb)], **bkw))       # the deterministic view's graph
                    bv = decs[n, kind].beam_views
                    views += [(f"slots {n} weights {kind or 'bf16'}", which, bv[key]) for which, key in
                              (("deterministic", (nb, False)), ("sampled", (nb, False, bool(a.sample))))]
            n_rep, step_t = a.step_replays, {}
            for rnd in range(max(1, a.repeats) + 1):                   # round 0 warms the replays up
                for name, which, ws in views:
                    keys = min(a.step_keys, ws["T"] - n_rep - 2)        # the round's appends stay inside the cache
                    assert keys > 0 and ws["graph"] is not None, (ws["T"], n_rep)
                    R_ = ws["pos"].shape[0]
                    ws["bupd_host"].zero_()
                    ws["bupd_host"][2 * R_:3 * R_].copy_(torch.arange(R_, dtype=torch.int32))
                    ws["bupd"].copy_(ws["bupd_host"])
                    for k, v in (("pos", keys), ("kvlen", keys + 1), ("lo", keys), ("gen", 4), ("live", 1), ("glive", 1)):
                        ws[k].fill_(v)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(n_rep):
                        ws["graph"].replay()
                    e1.record()
                    torch.cuda.synchronize()
                    if rnd:
                        step_t.setdefault((name, which), []).append(e0.elapsed_time(e1) / n_rep)
            for name in dict.fromkeys(v[0] for v in views):
                det, smp_ = sorted(step_t[(name, "deterministic")]), sorted(step_t[(name, "sampled")])
                md, ms = det[len(det) // 2], smp_[len(smp_) // 2]
                print(f"{name} beam step: deterministic {det[0]:.3f} / {md:.3f} / {det[-1]:.3f} ms, sampled {smp_[0]:.3f} / {ms:.3f} / "
                      f"{smp_[-1]:.3f} ms (min / median / max, {n_rep} replays per round) -> sampled / deterministic {ms / md:.3f}")
        sys.exit(0)
    if a.scores:
        from myriad_amd import ops
        cap, skw = 64 * ((160 + new + 63) // 64), dict(return_scores=True, watch_ids=[1000, 1001])
        decs = {n: L.slot_decoder(n, cap) for n in slot_counts}
        # batch 1: requests of one workspace capacity (greedy_generate keeps three workspaces; here two, with and without scores)
        few = [x for x in reqs if 64 < x.shape[0] + new + 2 <= 128][:max(1, len(reqs) // 8)]
        cols = [("batch 1", 0)] + [(f"slots {n}", n) for n in slot_counts]

        def run_col(n, on):
            extra = skw if on else {}
            if n == 0:
                return sum(L.greedy_generate(x[None], **kw, **extra)[0].shape[-1] for x in few), len(few)
            return sum(len(out[1]) for out in decs[n].run(reqs, **kw, **extra)), len(reqs)

        for _, n in cols:
            for on in (False, True):
                run_col(n, on)                                         # warm-up: kernels, both graphs of every column
        res = {(name, on): [] for name, _ in cols for on in (False, True)}
        for _ in range(max(1, a.repeats)):
            for name, n in cols:
                for on in (False, True):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    toks, samples = run_col(n, on)
                    torch.cuda.synchronize()
                    res[(name, on)].append((time.perf_counter() - t0, toks, samples))

        def mmm(ts, scale=1.0, fmt="{:.3f}"):
            ts = sorted(ts)
            return " / ".join(fmt.format(v * scale) for v in (ts[0], ts[len(ts) // 2], ts[-1]))

        print(f"{len(reqs)} requests (batch 1: the first {len(few)}), prompts {min(lens)}..{max(lens)} rows, {len(L.layers)} layers, "
              f"weights {L._packed['kind'] if L._packed else 'bf16'}; min / median / max of {max(1, a.repeats)} interleaved repeats")
        for name, _ in cols:
            for on in (False, True):
                r = res[(name, on)]
                print(f"{name} scores {'on ' if on else 'off'}: run {mmm([t for t, _, _ in r], 1e3, '{:.1f}')} ms, "
                      f"{mmm([sm / t for t, _, sm in r], 1.0, '{:.2f}')} samples/s, {r[-1][1]} tokens")
        # the captured step of each view alone: every row live at --step-keys keys, reset before each round
        views = [("batch 1", on, next(w for k, w in L._decode_ws.items() if (k[-1] == "scores") == on and k[0] == 1))
                 for on in (False, True)]
        for n in slot_counts:
            views += [(f"slots {n}", on, decs[n].views[decs[n]._view_key(1.0, None, False, on)]) for on in (False, True)]
        n_rep, step_t = a.step_replays, {}
        for rnd in range(max(1, a.repeats) + 1):                       # round 0 warms the replays up
            for name, on, ws in views:
                keys = min(a.step_keys, ws["T"] - n_rep - 2)            # the round's appends stay inside the cache
                assert keys > 0, (ws["T"], n_rep)
                ws["pos"].fill_(keys)
                ws["kvlen"].fill_(keys + 1)
                if "live" in ws:
                    ws["live"].fill_(1)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n_rep):
                    ws["graph"].replay()
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    step_t.setdefault((name, on), []).append(e0.elapsed_time(e1) / n_rep)
        for name, on, _ in views:
            print(f"{name} token step, scores {'on ' if on else 'off'}: {mmm(step_t[(name, on)])} ms/step ({n_rep} replays per round)")
        for name in dict.fromkeys(v[0] for v in views):
            off, on_ = sorted(step_t[(name, False)]), sorted(step_t[(name, True)])
            print(f"{name}: median step +{(on_[len(on_) // 2] - off[len(off) // 2]) * 1e3:.1f} us with scores "
                  f"({on_[len(on_) // 2] / off[len(off) // 2] - 1:+.2%})")
        for rows in (1, 64):                                           # the launch alone, 50 per captured graph
            lg = torch.randn(rows, L.V, device=dev)
            ids = torch.randint(0, L.V, (rows,), device=dev)
            wt, out = ops.score_watch_table([1000, 1001], L.V).to(dev), torch.zeros(ops.SCORE_ROWS, rows, device=dev)
            ops.token_scores_rows(lg, ids, wt, out)
            torch.cuda.synchronize()
            g_ = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_):
                for _ in range(50):
                    ops.token_scores_rows(lg, ids, wt, out)
            ts = []
            for rnd in range(max(1, a.repeats) + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g_.replay()
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    ts.append(e0.elapsed_time(e1) / 50)
            print(f"mh_token_scores_rows, {rows} rows of V = {L.V}: {mmm(ts, 1e3, '{:.2f}')} us per launch (50 back to back in a graph)")
        sys.exit(0)
    dec = L.slot_decoder(N, 64 * ((160 + new + 63) // 64))

    if a.sample:
        smodes = [m for m in a.modes.split(",") if m] or ["host", "device"]
        assert all(m in ("host", "device") for m in smodes), smodes
        default_dev, sstats = L.device_sampling, {}

        def run_sampled(mode):
            L.device_sampling = mode == "device"
            pen = a.penalty if mode == "device" else 1.0
            out = [len(ids) for _, ids, _ in dec.run(reqs, do_sample=True, top_p=0.9, top_k=50, repetition_penalty=pen, temperature=a.temperature,
                                                     generator=torch.Generator().manual_seed(0), **kw)]
            sstats[mode] = dict(dec.last_stats)
            return sum(out)

        for m in smodes:
            run_sampled(m)                                         # warm-up: kernels, the mode's graph
        res = {m: [] for m in smodes}
        for _ in range(max(1, a.repeats)):
            for m in smodes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = run_sampled(m)
                torch.cuda.synchronize()
                res[m].append((time.perf_counter() - t0, n))
        L.device_sampling = default_dev
        print(f"{len(reqs)} requests, prompts {min(lens)}..{max(lens)} rows, sampled top_p 0.9 top_k 50 temperature {a.temperature}, {N} slots, "
              f"weights {L._packed['kind'] if L._packed else 'bf16'}")
        for m in smodes:
            ts = sorted(t for t, _ in res[m])
            t, n, st = ts[len(ts) // 2], res[m][-1][1], sstats[m]
            pen = f" penalty {a.penalty}" if m == "device" and a.penalty != 1.0 else ""
            print(f"slots {N} sampled {m}{pen}: {t * 1e3:.1f} ms (median of {len(ts)}, min {ts[0] * 1e3:.1f}, max {ts[-1] * 1e3:.1f}) -> "
                  f"{n / t:.0f} tokens/s ({n} tokens), {len(reqs) / t:.1f} samples/s (min {len(reqs) / ts[-1]:.1f}, max "
                  f"{len(reqs) / ts[0]:.1f}); host-drawn rows {st['host_sampled_rows']}, device-drawn {st['device_sampled_rows']}, "
                  f"{st['steps']} steps, graph replays {st['graph_replays']}, occupancy {st['occupancy']:.3f}")
        sys.exit(0)

    if len(slot_counts) > 1:
        assert not a.sample, "a list of slot counts times the greedy run"
        cap = 64 * ((160 + new + 63) // 64)
        decs = {n: L.slot_decoder(n, cap) for n in slot_counts}
        pairs = [(1, 1)] + [(pb, rm) for pb in (int(x) for x in a.prefill_batch.split(","))
                            for rm in (int(x) for x in a.refill_min.split(",")) if (pb, rm) != (1, 1)]
        cols = [(n, pb, rm) for n in slot_counts for pb, rm in pairs]
        cstats = {}

        def run_col(c):
            n, pb, rm = c
            out = {i: ids for i, ids, _ in decs[n].run(reqs, prefill_batch=pb, refill_min=rm, **kw)}
            cstats[c] = dict(decs[n].last_stats)
            return [len(out[i]) for i in range(len(reqs))]

        want = [L.greedy_generate(x[None], **kw).shape[1] for x in reqs]      # batch 1: the answers every column must reproduce
        for c in cols:
            run_col(c)                                                 # warm-up: kernels, graphs, GEMM plans
        res = {c: [] for c in cols}
        for _ in range(max(1, a.repeats)):
            for c in cols:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = run_col(c)
                torch.cuda.synchronize()
                res[c].append((time.perf_counter() - t0, got))
        print(f"{len(reqs)} requests, prompts {min(lens)}..{max(lens)} rows, {sum(want)} tokens due ({min(want)}..{max(want)} per request), "
              f"weights {L._packed['kind'] if L._packed else 'bf16'}")
        for c in cols:
            ts = sorted(t for t, _ in res[c])
            t, got, st = ts[len(ts) // 2], res[c][-1][1], cstats[c]
            whole = sum(g == w for g, w in zip(got, want))
            print(f"slots {c[0]} prefill_batch {c[1]} refill_min {c[2]}: {t * 1e3:.1f} ms (median of {len(ts)}, min {ts[0] * 1e3:.1f}, max "
                  f"{ts[-1] * 1e3:.1f}) -> {len(reqs) / t:.1f} samples/s (min {len(reqs) / ts[-1]:.1f}, max {len(reqs) / ts[0]:.1f}), "
                  f"{sum(want) / t:.0f} due tokens/s; {whole}/{len(reqs)} answers complete; occupancy {st['occupancy']:.3f}, "
                  f"{st['steps']} steps, {st['prefills']} prefills in {st['prefill_passes']} passes")
        sys.exit(0)

    slot_stats = {}

    def run_slots(pb=1, rm=1):
        out = {i: ids for i, ids, _ in dec.run(reqs, prefill_batch=pb, refill_min=rm, **kw)}
        slot_stats[(pb, rm)] = dict(dec.last_stats)
        return [len(out[i]) for i in range(len(reqs))]

    def run_batch(n):
        got = []
        for g0 in range(0, len(reqs), n):
            grp = reqs[g0:g0 + n]
            S = max(x.shape[0] for x in grp)                       # one stacked prompt per group: left-pad with the first row
            emb = torch.stack([torch.cat([x[:1].expand(S - x.shape[0], -1), x]) for x in grp])
            ids = L.greedy_generate(emb, **kw)
            got += [ids.shape[1]] * len(grp)
        return got

    pairs = [(pb, rm) for pb in (int(x) for x in a.prefill_batch.split(",")) for rm in (int(x) for x in a.refill_min.split(","))
             if (pb, rm) != (1, 1)]
    slot_modes = {"slots %d" % N: (1, 1)}
    slot_modes.update({"slots %d prefill_batch %d refill_min %d" % (N, pb, rm): (pb, rm) for pb, rm in pairs})
    modes = (("slots %d" % N, run_slots), ("batch %d" % N, lambda: run_batch(N)), ("batch 1", lambda: run_batch(1)))
    modes += tuple((name, lambda pr=pr: run_slots(*pr)) for name, pr in slot_modes.items() if pr != (1, 1))
    for _, fn in modes:
        fn()                                                       # warm-up: kernels, graphs
    want = modes[2][1]()
    res = {name: [] for name, _ in modes}
    for _ in range(max(1, a.repeats)):
        for name, fn in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0, got))
    print(f"{len(reqs)} requests, prompts {min(lens)}..{max(lens)} rows, {sum(want)} tokens due ({min(want)}..{max(want)} per request), "
          f"weights {L._packed['kind'] if L._packed else 'bf16'}")
    for name, _ in modes:
        ts = sorted(t for t, _ in res[name])
        t, got = ts[len(ts) // 2], res[name][-1][1]
        whole = sum(g >= w for g, w in zip(got, want))
        st = slot_stats.get(slot_modes.get(name))
        tail = (f"; occupancy {st['occupancy']:.3f}, {st['steps']} steps, {st['prefills']} prefills in {st['prefill_passes']} passes "
                f"of {st['packed_rows']} rows") if st else ""
        print(f"{name}: {t * 1e3:.1f} ms (median of {len(ts)}, min {ts[0] * 1e3:.1f}, max {ts[-1] * 1e3:.1f}) -> "
              f"{sum(min(g, w) for g, w in zip(got, want)) / t:.0f} due tokens/s, {len(reqs) / t:.1f} samples/s; "
              f"{whole}/{len(reqs)} requests decoded to their own stop{tail}")
    sys.exit(0)

smp = make_samples(B)
smp_rows = make_samples(B * a.beams) if "beam" in modes else None
default_dev = model.llama.device_sampling
default_beam_sampling = model.llama.beam_sampling
default_fp8, default_fp4 = model.llama.decode_fp8, model.llama.decode_fp4
default_merge = model.llama.decode_merge_lora


def run(n, mode, kind=None, merge=None):
    kw, sm = {}, smp
    if mode == "beam":
        kw = dict(num_beams=a.beams, early_stopping="never")    # no early stop: every run decodes n tokens
    elif mode == "beam_sample":                                 # the chat call's knobs; the penalty rides in the same step
        kw = dict(num_beams=a.beams, early_stopping="never", do_sample=True, top_p=0.9, top_k=50,
                  generator=torch.Generator().manual_seed(0))
    elif mode.startswith("greedy_x"):
        sm = smp_rows
    elif mode != "greedy":
        kw = dict(do_sample=True, top_p=0.9, top_k=50, generator=torch.Generator().manual_seed(0))
    if mode != "beam":
        kw["repetition_penalty"] = a.penalty
    model.llama.device_sampling = {"host": False, "device": True}.get(mode, default_dev)
    model.llama.beam_sampling = mode == "beam_sample" or default_beam_sampling
    model.llama.decode_fp8 = default_fp8 if kind is None else kind == "fp8"
    model.llama.decode_fp4 = default_fp4 if kind is None else kind == "fp4"
    model.llama.decode_merge_lora = default_merge if merge is None else bool(merge)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.generate(sm, max_new_tokens=n, stop_ids=((-1,),), min_length=0, eos_token_id=-5, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


runs = [(m, w, mg) for m in modes for w in kinds for mg in merges]
for m, w, mg in runs:
    run(2, m, w, mg); run(6, m, w, mg)   # warm-up: kernels, then the token-step graph of this batch size is captured
res = {r: [] for r in runs}
for _ in range(a.repeats):
    for m, w, mg in runs:
        t_short, _ = run(a.new // 4, m, w, mg)
        t_long, out = run(a.new, m, w, mg)
        n_long, n_short = out["token_ids"].shape[1], a.new // 4
        if m in ("beam", "beam_sample"):
            n_long = model.last_generate_stats["steps"]       # hypotheses may end before the last step; the step count does not
        res[(m, w, mg)].append(((t_long - t_short) / (n_long - n_short), t_long, n_long, dict(model.last_generate_stats)))
for m, w, mg in runs:
    ts = sorted(r[0] for r in res[(m, w, mg)])
    per_tok, t_long, n_long, st = res[(m, w, mg)][-1]
    per_tok = ts[len(ts) // 2]                        # prefill / vision cancel: pure single-token decode steps (median)
    extra = (f" [{m}: device-drawn rows {st.get('device_sampled_rows', 0)}, host-drawn {st.get('host_sampled_rows', 0)}, "
             f"graph replays {st.get('graph_replays', 0)}]" if m != "greedy" or a.penalty != 1.0 else "")
    if m == "beam_sample":
        extra = (f" [beam_sample: sampled steps {st['beam_sampled_steps']}, item-steps redone on the host {st['beam_host_steps']}, "
                 f"graph replays {st['graph_replays']}]")
    rows = B * a.beams if m in ("beam", "beam_sample", "greedy_x%d" % a.beams) else B
    wb = st["decode_weight_bytes"]
    lora_tag = (" +LoRA merged" if st.get("lora_merged") else " +LoRA") if a.lora else ""
    print(f"batch {B} rows {rows}{lora_tag} {m} weights {st['decode_weights']}"
          f"{f' penalty {a.penalty}' if a.penalty != 1.0 else ''}: {n_long} tokens in "
          f"{t_long*1e3:.1f} ms (incl. ViT+Q-Former+prefill); decode step {per_tok*1e3:.3f} ms/token (median of {len(ts)}, "
          f"min {ts[0]*1e3:.3f}, max {ts[-1]*1e3:.3f}) -> {rows / per_tok:.1f} row-tok/s steady; weight stream "
          f"{wb / 1e9:.2f} GB/token, {wb / per_tok / 1e12:.2f} TB/s of 6.3 achievable{extra}")

if kinds != [None]:
    # one-time cost of packing wo, gate|up and down of every layer (and wqkv without LoRA) into each kind, median of --repeats
    L = model.llama
    names = ("wo", "wgu", "wd") + (() if a.lora else ("wqkv",))
    for kind in kinds:
        outs = [L._pack_quantised(kind, Lr[k], k) for Lr in L.layers for k in names]
        ts = []
        for _ in range(max(3, a.repeats)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            it = iter(outs)
            for Lr in L.layers:
                for k in names:
                    L._pack_quantised(kind, Lr[k], k, next(it))
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        rd = sum(Lr[k].numel() * 2 for Lr in L.layers for k in names)
        print(f"pack of {len(outs)} matrices into the {kind} copy: {ts[len(ts) // 2] * 1e3:.3f} ms (median of {len(ts)}, min "
              f"{ts[0] * 1e3:.3f}); {rd / 1e9:.2f} GB of bf16 rows read")
        del outs

if a.lora and 1 in merges:
    # one-time cost of a merge of every layer (what generate() pays when the LoRA weights moved), median of --repeats
    L = model.llama
    for kind in ("bf16", "fp8", "fp4"):
        def merge_all(outs=None, kind=kind):
            if kind != "fp4":
                return L.lora.merge(L.layers, kind, outs)
            res = []                                  # two launches per layer: the row-major merge into one scratch, then the packer
            for i, Lr in enumerate(L.layers):
                L._merge_rows = L.lora.merge_layer(i, Lr, "rows", L._merge_rows)
                res.append(L._pack_quantised(kind, L._merge_rows, "merged wqkv", None if outs is None else outs[i]))
            return res
        outs = merge_all()
        ts = []
        for _ in range(max(3, a.repeats)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            merge_all(outs)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        D, nl = L.D, len(L.layers)
        rd = nl * 3 * D * D * 2 * (2 if kind != "bf16" else 1)
        wr = nl * 3 * D * D * {"bf16": 2, "fp8": 1, "fp4": 2.53}[kind]        # fp4: the bf16 rows, then codes and scale bytes
        print(f"merge of {nl} layers into the {kind} copy: {ts[len(ts) // 2] * 1e3:.3f} ms (median of {len(ts)}, min "
              f"{ts[0] * 1e3:.3f}); W read {rd / 1e9:.2f} GB (fp8: two passes; fp4: W, then the merged rows), written {wr / 1e9:.2f} GB -> "
              f"{(rd + wr) / ts[len(ts) // 2] / 1e12:.2f} TB/s")
        del outs
