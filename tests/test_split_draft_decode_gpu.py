"""Draft-and-verify decoding on the split-KV view and in SlotDecoder.run_turns / ChatPool (behind `draft_split`,
MYRIAD_DRAFT_SPLIT=1): the verify step's attention is mh_attn_decode_rope_split_draft[_rows], whose rows carry the bits of the
one-row split-KV step, so whatever the drafter proposes the ids, margins, scores and reused prefixes are those of the same call
without `draft`.  With the switch off every entry answers as before."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import ops  # noqa: E402
from myriad_amd.decode_host import NgramDrafter, replay_slot_run  # noqa: E402
from myriad_amd.llama import DecodeSession  # noqa: E402
from tests import chat_pool_case as C  # noqa: E402
from tests import golden_utils as gu  # noqa: E402
from tests.test_draft_decode_gpu import Noise  # noqa: E402
from tests.test_draft_slots_gpu import CAP, COUNTS, KW, _run, _same, chain  # noqa: E402,F401
from tests.test_entrypoints_gpu import _batch, fx, model  # noqa: E402,F401

DEV = "cuda:0"
DRAFT_COUNTS = ("verify_steps", "plain_steps", "draft_proposed", "draft_accepted")


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _session_turns(lm, first, second, split=True, draft=None, capacity=C.CAPACITY, **kw):
    """Two turns of one DecodeSession: [(ids, margins, extras)] and the per-turn stats.  first = (ctx [S, D], keys); second(ids) =
    the second turn's (ctx, keys) given the first turn's ids."""
    sess = DecodeSession(lm, capacity, split=split)
    if draft is not None:
        kw = dict(kw, draft=draft, draft_k=4)
    outs, stats = [], []
    ctx, keys = first
    for turn in range(2):
        gen = dict(generator=torch.Generator().manual_seed(11 + turn)) if kw.get("do_sample") else {}
        out = sess.generate(ctx[None].to(DEV), [keys], weights_version=0, return_margins=True, **gen, **kw)
        outs.append(out)
        stats.append(dict(sess.last_stats))
        if turn == 0:
            ctx, keys = second(out[0][0].tolist(), ctx, keys)
    return outs, stats


def _equal_turns(a, b):
    for x, y in zip(a, b):
        if not (torch.equal(x[0], y[0]) and torch.equal(_bits(x[1]), _bits(y[1])) and len(x) == len(y)):
            return False
        if len(x) == 3 and not all(torch.equal(_bits(x[2][k]), _bits(y[2][k])) for k in ("token_logprobs", "watch_logprobs")):
            return False
    return len(a) == len(b)


def _chain_turns(lm):
    emb_w = gu.decode_chain_weights()["llama_model.model.embed_tokens.weight"]
    return C.first_turn("a", emb_w), lambda ids, ctx, keys: C.next_turn("a", 1, ctx, keys, ids, emb_w[ids].to(torch.bfloat16).float(), emb_w)


GEN = dict(max_new_tokens=C.MAX_NEW, stop_ids=C.STOPS, eos_id=C.EOS, min_length=1)


# ------------------------------------------------------------------------------------------------ the switch off
def test_with_the_switch_off_the_split_view_runs_plain_steps_and_run_turns_refuses(chain):
    lm = chain.lm
    assert lm.draft_split is False                                             # off by default
    first, second = _chain_turns(lm)
    ref, ref_st = _session_turns(lm, first, second, **GEN)
    d = NgramDrafter([o[0][0].tolist() for o in ref])
    out, st = _session_turns(lm, first, second, draft=d, **GEN)
    assert _equal_turns(out, ref) and all(s["draft_off"] == "split_kv" and s["verify_steps"] == 0 and s["split_kv"] for s in st)
    with pytest.raises(NotImplementedError, match="run_turns"):
        lm.slot_decoder(2, CAP, split_kv=True).run_turns([("s", chain.reqs[0], list(range(chain.lens[0])))], draft=d)
    outs, st = _run(lm.slot_decoder(4, CAP, split_kv=True), chain.reqs[:4], draft=NgramDrafter(chain.ids), draft_k=4, **KW)
    assert st["draft_off"] == "split_kv" and st["verify_steps"] == 0


# ------------------------------------------------------------------------------------------------ one session
def test_a_two_turn_split_session_with_draft_has_the_bits_and_the_reuse_of_the_session_without(chain, monkeypatch):
    lm = chain.lm
    first, second = _chain_turns(lm)
    ref, ref_st = _session_turns(lm, first, second, **GEN)
    assert all(s["split_kv"] and "draft_off" not in s for s in ref_st)
    monkeypatch.setattr(lm, "draft_split", True)
    out, st = _session_turns(lm, first, second, draft=NgramDrafter([o[0][0].tolist() for o in ref]), **GEN)
    assert _equal_turns(out, ref), ([o[0] for o in out], [o[0] for o in ref])
    assert all(s["draft_off"] is None and s["verify_steps"] > 0 and s["split_kv"] for s in st) and st[0]["draft_accepted"] > 0
    assert [s["reused_tokens"] for s in st] == [s["reused_tokens"] for s in ref_st] and st[1]["reused_tokens"] > 0
    out, st = _session_turns(lm, first, second, draft=Noise(gu.DECODE_CHAIN["vocab"]), **GEN)      # taught noise: nothing stands
    assert _equal_turns(out, ref) and all(s["draft_off"] is None and s["verify_steps"] > 0 and s["draft_accepted"] == 0 for s in st)
    assert [s["reused_tokens"] for s in st] == [s["reused_tokens"] for s in ref_st]
    monkeypatch.setattr(ops, "attn_decode_split_draft_supported", lambda *a: False)
    out, st = _session_turns(lm, first, second, draft=NgramDrafter([o[0][0].tolist() for o in ref]), **GEN)
    assert _equal_turns(out, ref) and all(s["draft_off"] == "unsupported" and s["verify_steps"] == 0 for s in st)


@pytest.mark.parametrize("lora", ["bordered", "merged"])
@pytest.mark.parametrize("kind", ["bf16", "fp8", "fp4"])
def test_every_kind_of_decode_weights_on_the_split_view(kind, lora, monkeypatch):
    from tests.test_fp4_decode_gpu import _lora_model
    emb, _, _, lm = _lora_model()
    lm.decode_fp8, lm.decode_fp4, lm.decode_merge_lora = kind == "fp8", kind == "fp4", lora == "merged"
    lm.decode_lora_version = 0                                                 # as its owner sets it: one merge, kept across the turns
    kw = dict(max_new_tokens=16, stop_ids=())
    first = (emb[0, :7].float(), [("r", 0, j) for j in range(7)])

    def second(ids, ctx, keys):
        rows = torch.empty((len(ids), lm.D), dtype=torch.float32, device=DEV)
        lm.embed_tokens_into(torch.tensor(ids, dtype=torch.long, device=DEV), rows)
        return (torch.cat([ctx, rows.cpu(), emb[1, :5].float()], 0), list(keys) + [("t", int(t)) for t in ids] + [("r", 1, j) for j in range(5)])

    ref, ref_st = _session_turns(lm, first, second, **kw)
    monkeypatch.setattr(lm, "draft_split", True)
    out, st = _session_turns(lm, first, second, draft=NgramDrafter([o[0][0].tolist() for o in ref]), **kw)
    assert _equal_turns(out, ref), ([o[0] for o in out], [o[0] for o in ref])
    assert all(s["draft_off"] is None and s["verify_steps"] > 0 and s["split_kv"] for s in st) and st[0]["draft_accepted"] > 0
    assert [s["reused_tokens"] for s in st] == [s["reused_tokens"] for s in ref_st] and st[1]["reused_tokens"] > 0
    assert lm.last_generate_stats["decode_weights"] == kind and lm.last_generate_stats["lora_merged"] is (lora == "merged")


def test_a_sampled_penalised_scored_turn_on_the_split_view_equals_the_turn_without_draft(chain, monkeypatch):
    lm = chain.lm
    for name in ("draft_split", "draft_sampling", "device_sampling"):
        monkeypatch.setattr(lm, name, True)
    first, second = _chain_turns(lm)
    kw = dict(GEN, do_sample=True, top_p=0.9, top_k=50, temperature=1.5, repetition_penalty=1.2, return_scores=True, watch_ids=(2, 835))
    ref, ref_st = _session_turns(lm, first, second, **kw)
    assert len(ref[0]) == 3
    for d in (NgramDrafter([o[0][0].tolist() for o in ref]), Noise(gu.DECODE_CHAIN["vocab"])):
        out, st = _session_turns(lm, first, second, draft=d, **kw)
        assert _equal_turns(out, ref), (type(d).__name__, [o[0] for o in out], [o[0] for o in ref])
        assert all(s["draft_off"] is None and s["verify_steps"] > 0 and s["split_kv"] for s in st)
        assert [s["reused_tokens"] for s in st] == [s["reused_tokens"] for s in ref_st]


# ------------------------------------------------------------------------------------------------ the slots
@pytest.mark.parametrize("split_kv", [True, None])
def test_a_split_slot_decoder_drafts_with_the_solo_bits_and_the_predicted_counts(chain, monkeypatch, split_kv):
    lm = chain.lm
    monkeypatch.setattr(lm, "draft_split", True)
    if split_kv is None:                                                       # the rule chooses the split-KV view
        import myriad_amd.decode as decode
        monkeypatch.setattr(decode, "split_kv_rows_rule", lambda *a: True)
    out, st = _run(lm.slot_decoder(4, CAP, split_kv=split_kv), chain.reqs, draft=NgramDrafter(chain.ids), draft_k=4, **KW)
    assert _same(out, chain.solo)
    assert st["split_kv"] and st["draft_off"] is None and st["verify_steps"] > 0 and st["draft_accepted"] > 0
    want = replay_slot_run(chain.lens, chain.ids, 4, 90, draft=NgramDrafter(chain.ids), draft_k=4, stop_ids=((835,), (2277, 29937)))
    assert {k: st[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, (st, want)


# ------------------------------------------------------------------------------------------------ turns
def _two_calls(lm, split_kv, draft=None, **kw):
    """Three sessions, two run_turns calls each: per call {session: (ids, margins)}, the per-turn stats, the call's stats."""
    emb_w = gu.decode_chain_weights()["llama_model.model.embed_tokens.weight"]
    dec = lm.slot_decoder(C.SLOTS, C.CAPACITY, split_kv=split_kv)
    state = {s: C.first_turn(s, emb_w) for s in C.SESSIONS}
    if draft is not None:
        kw = dict(kw, draft=draft, draft_k=4)
    log = []
    for k in range(2):
        turns = [(s, state[s][0], state[s][1]) for s in C.SESSIONS]
        got = {s: (ids.cpu(), mar.cpu()) for s, ids, mar in dec.run_turns(turns, **dict(GEN, **kw))}
        st = dict(dec.last_stats)
        log.append((got, st))
        for s in C.SESSIONS:
            ids = got[s][0].tolist()
            state[s] = C.next_turn(s, k + 1, state[s][0], state[s][1], ids, emb_w[ids].to(torch.bfloat16).float(), emb_w)
    return log


@pytest.mark.parametrize("split_kv", [False, True])
def test_run_turns_with_draft_has_the_bits_and_the_reuse_of_run_turns_without(chain, monkeypatch, split_kv):
    lm = chain.lm
    ref = _two_calls(lm, split_kv)
    monkeypatch.setattr(lm, "draft_split", True)
    corpus = [got[s][0].tolist() for got, _ in ref for s in C.SESSIONS]
    for d in (NgramDrafter(corpus), Noise(gu.DECODE_CHAIN["vocab"])):
        log = _two_calls(lm, split_kv, draft=d)
        for k, ((got, st), (r_got, r_st)) in enumerate(zip(log, ref)):
            assert _same(got, r_got), (k, type(d).__name__)
            assert st["turns"] == r_st["turns"], (k, st["turns"], r_st["turns"])       # the reused prefixes: no stale row recorded or read
            assert st["split_kv"] is split_kv and st["draft_off"] is None and st["verify_steps"] > 0
            if isinstance(d, NgramDrafter):
                ids = [got[s][0].tolist() for s in C.SESSIONS]
                want = replay_slot_run([t["prefilled_tokens"] for t in st["turns"]], ids, C.SLOTS, C.MAX_NEW, stop_ids=C.STOPS, eos_id=C.EOS,
                                       draft=NgramDrafter(corpus), draft_k=4)
                assert {c: st[c] for c in ("steps",) + DRAFT_COUNTS} == {c: want[c] for c in ("steps",) + DRAFT_COUNTS}, (k, st, want)
                assert st["draft_accepted"] > 0 and st["steps"] < r_st["steps"]
            else:
                assert st["draft_accepted"] == 0
        assert log[1][1]["turns"][0]["reused_tokens"] > 0
    assert "draft_k" not in ref[0][1]


# ------------------------------------------------------------------------------------------------ the chat pool
def test_chat_pool_answers_with_draft_what_it_answers_without(model, monkeypatch):
    from myriad_amd.chat import CONV_VISION, ChatPool
    model.eval()
    try:
        samples = _batch(2, train=False, seed=5)
        questions = [("Is there a defect?", "Where is it?"), ("What is shown?", "Is it damaged?")]

        def two_rounds(**kw):
            pool = ChatPool(model, slots=2, capacity=1024)
            convs = []
            for i in range(2):
                conv, imgs = CONV_VISION.copy(), []
                pool.upload_img(samples["image"][i:i + 1], conv, imgs, anomaly_maps=samples["anomaly_maps"][i:i + 1])
                convs.append((conv, imgs))
            outs = []
            for t in range(2):
                for i in range(2):
                    pool.ask(questions[i][t], convs[i][0])
                texts = [text for text, _ in pool.answer_many(convs, max_new_tokens=12, do_sample=False, prefill_batch=1, **kw)]
                outs.append((texts, [ids.tolist() for ids in pool.last_token_ids], [dict(s) for s in pool.last_stats]))
            return outs

        plain = two_rounds()
        d = NgramDrafter([ids for _, all_ids, _ in plain for ids in all_ids])
        with pytest.raises(NotImplementedError):                               # both switches off
            two_rounds(draft=d, draft_k=4)
        monkeypatch.setattr(model.llama, "slot_draft", True)
        with pytest.raises(NotImplementedError, match="MYRIAD_DRAFT_SPLIT"):
            two_rounds(draft=d, draft_k=4)
        monkeypatch.setattr(model.llama, "draft_split", True)
        got = two_rounds(draft=d, draft_k=4)
        turn_keys = ("context_tokens", "reused_tokens", "prefilled_tokens", "full_reprefill_reason", "split_kv")
        for (texts, ids, st), (r_texts, r_ids, r_st) in zip(got, plain):
            assert texts == r_texts and ids == r_ids
            for s, r in zip(st, r_st):
                assert {k: s[k] for k in turn_keys} == {k: r[k] for k in turn_keys}
                assert s["draft_k"] == 4 and s["draft_off"] is None and s["verify_steps"] > 0 and s["draft_accepted"] > 0
                assert s["steps"] < r["steps"] and "draft_k" not in r
        assert got[1][2][0]["reused_tokens"] > 0
    finally:
        model.train()
