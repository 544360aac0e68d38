"""The decode slots on the split-KV rows kernel (SlotDecoder(split_kv=True), mh_attn_decode_rope_split_rows in the captured
token step): conversations of the peaked token-transition LLaMA (tests/golden_utils.py decode_chain_weights, the chains and tails
of tests/chat_pool_case.py) whose contexts grow across 128-key chunk boundaries, against a solo DecodeSession(split=True) each bit
for bit, alone against seven neighbours, against the single-workgroup rows kernel up to the oracle's near tie, at 17 slots (the
wide step), and myriad_amd.chat.ChatPool(split_kv=True) against solo Chats on the model built from the reference's on-disk files."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd.chat import CONV_VISION, Chat, ChatPool  # noqa: E402
from myriad_amd.llama import DecodeSession, LlamaHIP  # noqa: E402
from oracle import myriad_ref as R  # noqa: E402
from tests import chat_pool_case as C  # noqa: E402
from tests import fp8_ref as F  # noqa: E402
from tests import golden_utils as gu  # noqa: E402
from tests.test_entrypoints_gpu import DEV, _batch, fx, model  # noqa: E402,F401

F32 = torch.float32
KW = dict(max_new_tokens=C.MAX_NEW, stop_ids=C.STOPS, eos_id=C.EOS, min_length=1)
CAP = 512
# First-context rows and the rows each later turn adds, placed by the chains' lengths under KW (row0 / row1 make 8 ids, row2 4,
# stop835 3, row3 2; n ids are n - 1 token steps that see S0 + 1 .. S0 + n - 1 keys): "a" decodes across key 128 in turn 1 and
# across 256 in turn 3, "b" across 256 in turn 1 and 384 in turn 2, "c" across 128 in turn 2, and its one step of turn 3 appends
# row 256 -- the first row of a chunk that holds nothing else yet.
FIRST = {"a": 124, "b": 255, "c": 60}
ADDED = {"a": [60, 58], "b": [122, 30], "c": [61, 123]}


@pytest.fixture(scope="module")
def lm():
    c = gu.DECODE_CHAIN
    sd = gu.decode_chain_weights()
    return dict(lm=LlamaHIP(sd, c["heads"], DEV, need_backward=False), sd=sd, heads=c["heads"],
                emb_w=sd["llama_model.model.embed_tokens.weight"])


def _id_rows(lm, ids):
    out = torch.empty((len(ids), lm.D), dtype=F32, device=DEV)
    lm.embed_tokens_into(torch.tensor(ids, dtype=torch.long, device=DEV), out)
    return out.cpu()


def _first(s, emb_w, n=None):
    g = torch.Generator().manual_seed(4000 + C.SESSIONS.index(s) if s in C.SESSIONS else 4100 + int(s))
    n = FIRST[s] if n is None else n
    start = C.STARTS[s][0] if s in C.SESSIONS else ["row0", "row2", "stop835", "row3"][int(s) % 4]
    return C._tail(n, start, emb_w, g), [("r", s, 0, j) for j in range(n)]


def _next(s, k, n, ctx, keys, ids, id_rows, emb_w):
    """Turn k of session s: the last context, every id the last turn generated and n new rows that end on the turn's chain."""
    g = torch.Generator().manual_seed(5000 + 10 * C.SESSIONS.index(s) + k)
    new = C._tail(n, C.STARTS[s][k], emb_w, g)
    return torch.cat([ctx, id_rows, new], 0), list(keys) + [("t", int(t)) for t in ids] + [("r", s, k, j) for j in range(n)]


def _turns(dec, turns, **kw):
    return {s: (ids.tolist(), mar) for s, ids, mar in dec.run_turns(turns, **dict(KW, **kw))}


@pytest.fixture(scope="module")
def talks(lm):
    """Three conversations x three turns on SlotDecoder(3 slots, split_kv=True), prefill_batch = 1, run once: per turn and session
    the context, its keys, the pool's ids and margins, and a solo DecodeSession(split=True)'s on the same context."""
    L, emb_w = lm["lm"], lm["emb_w"]
    dec = L.slot_decoder(3, CAP, split_kv=True)
    solo = {s: DecodeSession(L, CAP, split=True) for s in C.SESSIONS}
    state = {s: _first(s, emb_w) for s in C.SESSIONS}
    log = []
    for k in range(3):
        got = _turns(dec, [(s, state[s][0], state[s][1]) for s in C.SESSIONS], prefill_batch=1)
        split_kv = dec.last_stats["split_kv"]
        row = {}
        for s in C.SESSIONS:
            ctx, keys = state[s]
            ids, mar = got[s]
            s_ids, s_mar = solo[s].generate(ctx[None].to(DEV), [keys], weights_version=0, return_margins=True, **KW)
            row[s] = dict(ctx=ctx, keys=keys, ids=ids, margins=mar, solo_ids=s_ids[0].tolist(), solo_margins=s_mar[0].cpu(),
                          solo_split=solo[s].last_stats["split_kv"], split_kv=split_kv)
            if k < 2:
                state[s] = _next(s, k + 1, ADDED[s][k], ctx, keys, ids, _id_rows(L, ids), emb_w)
        log.append(row)
    return dict(log=log, dec=dec, graph_captures=dec.graph_captures)


def test_three_conversations_on_the_split_rows_kernel_equal_a_solo_split_session_each(talks):
    crossed = set()
    for k, row in enumerate(talks["log"]):
        for s in C.SESSIONS:
            r = row[s]
            assert r["split_kv"] is True and r["solo_split"] is True
            assert r["ids"] == r["solo_ids"], (k, s, r["ids"], r["solo_ids"])
            n = len(r["ids"])
            assert torch.equal(r["margins"], r["solo_margins"][:n]), (k, s, r["margins"], r["solo_margins"])
            lo, hi = r["ctx"].shape[0], r["ctx"].shape[0] + n - 1    # keys the turn's token steps saw: lo + 1 .. hi
            crossed |= {(s, c) for c in (128, 256, 384) if lo <= c < hi}
    assert len({c for _, c in crossed}) == 3 and len(crossed) >= 5, crossed      # decoded across chunk boundaries
    assert max(r["ctx"].shape[0] for r in talks["log"][2].values()) > 384
    assert talks["graph_captures"] == 1                              # one captured split step over all three calls


def test_a_conversation_alone_equals_itself_among_seven_neighbours(lm):
    """Two turns of one conversation in an 8-slot split decoder: alone (slot 0, seven idle rows whose partial records are never
    written) and fourth of eight (slot 3; a neighbour on the stop835 chain ends early and its row idles on).  Rows meet only in
    the attention launch, so its ids and margins differ only through a leak across rows."""
    L, emb_w = lm["lm"], lm["emb_w"]
    runs = []
    for others in (0, 7):
        dec = L.slot_decoder(8, CAP, split_kv=True)
        names = [str(i) for i in range(others)]
        names.insert(min(3, others), "a")
        state = {s: _first(s, emb_w, None if s == "a" else 20 + 37 * int(s)) for s in names}
        got = []
        for k in range(2):
            out = _turns(dec, [(s, state[s][0], state[s][1]) for s in names], prefill_batch=1)
            assert dec.last_stats["split_kv"] is True
            got.append(out["a"])
            for s in names:
                ctx, keys = state[s]
                ids = out[s][0]
                if s == "a":
                    state[s] = _next(s, k + 1, ADDED[s][k], ctx, keys, ids, _id_rows(L, ids), emb_w)
                else:
                    state[s] = (torch.cat([ctx, _id_rows(L, ids)], 0), list(keys) + [("t", int(t)) for t in ids])
        if others:
            assert dec.sessions.slot_of("a") == 3 and len({len(out[s][0]) for s in names}) > 1       # ragged stops
        runs.append(got)
    for (ids0, mar0), (ids1, mar1) in zip(*runs):
        assert ids0 == ids1 and torch.equal(mar0, mar1), (ids0, ids1, mar0, mar1)


def test_split_and_single_workgroup_steps_agree_up_to_the_near_tie_and_keep_a_graph_each(lm, talks):
    L = lm["lm"]
    row = talks["log"][2]                                            # the longest contexts
    turns = [(s, row[s]["ctx"], row[s]["keys"], "test") for s in C.SESSIONS]     # a reset: every call prefills in full
    dec = L.slot_decoder(3, CAP)
    assert dec.split_kv is False
    single = _turns(dec, turns, prefill_batch=1)
    assert dec.last_stats["split_kv"] is False and dec.graph_captures == 1
    dec.split_kv = True
    split = _turns(dec, turns, prefill_batch=1)
    assert dec.last_stats["split_kv"] is True and dec.graph_captures == 2        # the split view's own capture
    dec.split_kv = False
    again = _turns(dec, turns, prefill_batch=1)
    assert dec.last_stats["split_kv"] is False and dec.graph_captures == 2       # the first graph was kept
    dec.split_kv = True
    _turns(dec, turns, prefill_batch=1)
    assert dec.graph_captures == 2
    compared = 0
    for s in C.SESSIONS:
        assert again[s][0] == single[s][0] and torch.equal(again[s][1], single[s][1])
        with torch.no_grad():
            _, mar, sc = R.greedy_generate(lm["sd"], row[s]["ctx"][None], lm["heads"], return_margins=True, return_scales=True, **KW)
        horizon = F.two_ulp_horizon(mar, sc)
        n = min(horizon, len(single[s][0]), len(split[s][0]))
        assert split[s][0][:n] == single[s][0][:n], (s, horizon, split[s][0], single[s][0])
        if horizon >= mar.shape[1]:                                  # no near tie anywhere: the whole turn, its length too
            assert split[s][0] == single[s][0]
        compared += n
    assert compared > 0


def test_the_wide_step_takes_the_split_rows_kernel_with_the_same_ids(lm):
    L, emb_w = lm["lm"], lm["emb_w"]
    reqs = [_first(str(i), emb_w, n)[0] for i, n in enumerate((125, 60, 200))]    # the first decodes across key 128
    want = sorted(L.slot_decoder(4, 256, split_kv=True).run(reqs, **KW), key=lambda r: r[0])
    dec = L.slot_decoder(17, 256, split_kv=True)
    got = sorted(dec.run(reqs, **KW), key=lambda r: r[0])
    assert dec.last_stats["split_kv"] is True and dec.ws["x_in"].shape[0] == 17 and dec.ws["split"] is not None
    assert [r[0] for r in got] == [0, 1, 2]
    for g, w in zip(got, want):
        assert torch.equal(g[1], w[1]) and torch.equal(g[2], w[2]), (g, w)


# ------------------------------------------------------------------ ChatPool
QUESTIONS = [("Is there a defect?", "Where is it?"), ("Describe the image.", "Is the object damaged?")]
MAX_NEW = 8


def _open(chat, samples, i):
    conv, imgs = CONV_VISION.copy(), []
    assert chat.upload_img(samples["image"][i:i + 1], conv, imgs, anomaly_maps=samples["anomaly_maps"][i:i + 1])[0] == "Received."
    return conv, imgs


def test_chat_pool_on_the_split_kernel_answers_like_solo_chats_forced_to_split(model):
    """prefill_batch = 1: every prefill is the solo one on both sides, and the token step's rows do not depend on the row count,
    so the pool's answers are the solo split sessions' bit for bit."""
    model.eval()
    try:
        samples = _batch(2, train=False, seed=5)
        pool = ChatPool(model, slots=4, capacity=1024, split_kv=True)
        solos = [Chat(model, device=DEV) for _ in range(2)]
        for c in solos:
            c.session = DecodeSession(model.llama, 1024, split=True)
        convs = [_open(pool, samples, i) for i in range(2)]
        twins = [_open(solos[i], samples, i) for i in range(2)]
        for t in range(2):
            for i in range(2):
                pool.ask(QUESTIONS[i][t], convs[i][0])
                solos[i].ask(QUESTIONS[i][t], twins[i][0])
            out = pool.answer_many(convs, max_new_tokens=MAX_NEW, do_sample=False, prefill_batch=1)
            assert [st["split_kv"] for st in pool.last_stats] == [True, True]
            for i in range(2):
                text, _ = solos[i].answer(*twins[i], max_new_tokens=MAX_NEW, do_sample=False)
                assert solos[i].last_stats["split_kv"] is True
                assert torch.equal(pool.last_token_ids[i], solos[i].last_token_ids[0].cpu()), (t, i)
                assert out[i][0] == text == convs[i][0].messages[-1][1]
                assert (pool.last_stats[i]["reused_tokens"] > 0) == (t > 0)
        assert pool.last_stats[0]["graph_captures"] == 1
    finally:
        model.train()
