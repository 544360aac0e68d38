"""Several conversations at once on the decode slots: SlotDecoder.run_turns (every session in its own slot, only the rows past the
reused prefix prefilled, packed through mh_attn_prefill_ragged_past or solo with `past`) on the peaked token-transition LLaMA
against a DecodeSession per conversation and from-scratch decoding, and myriad_amd.chat.ChatPool against solo Chats on the model
built from the reference's on-disk files."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd.chat import CONV_VISION, STOP_WORDS, Chat, ChatPool  # noqa: E402
from myriad_amd.llama import DecodeSession, LlamaHIP, SessionTable  # noqa: E402
from oracle import myriad_ref as R  # noqa: E402
from tests import chat_pool_case as C  # noqa: E402
from tests import fp8_ref as F  # noqa: E402
from tests import golden_utils as gu  # noqa: E402
from tests.test_entrypoints_gpu import DEV, _batch, fx, model  # noqa: E402,F401

F32 = torch.float32
KW = dict(max_new_tokens=C.MAX_NEW, stop_ids=C.STOPS, eos_id=C.EOS, min_length=1)


def _turns(dec, turns, **kw):
    """One run_turns call: ({session: (ids list, margins tensor)}, the per-turn stats in the turns' order)."""
    got = {s: (ids.tolist(), mar) for s, ids, mar in dec.run_turns(turns, **dict(KW, **kw))}
    assert set(got) == {t[0] for t in turns}
    return got, dec.last_stats["turns"]


def _id_rows(lm, ids):
    out = torch.empty((len(ids), lm.D), dtype=F32, device=DEV)
    lm.embed_tokens_into(torch.tensor(ids, dtype=torch.long, device=DEV), out)
    return out


def _oracle(p, ctx, **kw):
    """(horizon, whole): the steps before the oracle's first two-ulp near tie on this context, and whether there is none."""
    with torch.no_grad():
        _, mar, sc = R.greedy_generate(p["sd"], ctx[None], p["heads"], return_margins=True, return_scales=True, **dict(KW, **kw))
    h = F.two_ulp_horizon(mar, sc)
    return h, h >= mar.shape[1]


def _gate(got, want, horizon, whole, what):
    n = min(horizon, len(want), len(got))
    assert got[:n] == want[:n], (what, got, want)
    if whole:                                                        # no near tie anywhere: the whole turn, its length too
        assert got == want, (what, got, want)


@pytest.fixture(scope="module")
def peaked():
    """Three sessions x three turns on 3 slots of capacity 128 (tests/chat_pool_case.py), prefill_batch = 3, run once: per turn and
    session the context, its keys, the pool's ids and margins and per-turn stats, what a SessionTable of its own predicts, a
    per-conversation DecodeSession's ids, from-scratch greedy_generate's ids and the oracle's two-ulp horizon."""
    c = gu.DECODE_CHAIN
    sd = gu.decode_chain_weights()
    lm = LlamaHIP(sd, c["heads"], DEV, need_backward=False)
    emb_w = sd["llama_model.model.embed_tokens.weight"]
    p = dict(lm=lm, sd=sd, heads=c["heads"], emb_w=emb_w)
    dec = lm.slot_decoder(C.SLOTS, C.CAPACITY)
    solo = {s: DecodeSession(lm, C.CAPACITY) for s in C.SESSIONS}
    table = SessionTable(C.SLOTS)
    state = {s: C.first_turn(s, emb_w) for s in C.SESSIONS}
    log = []
    for k in range(3):
        turns = [(s, state[s][0], state[s][1]) for s in C.SESSIONS]
        got, stats = _turns(dec, turns, prefill_batch=3)
        row = {}
        for i, s in enumerate(C.SESSIONS):
            ctx, keys = state[s]
            ids = got[s][0]
            pred = table.begin(s, keys)
            table.end(s, keys, ids)
            x = ctx[None].to(DEV)
            sess = solo[s].generate(x, [keys], weights_version=0, **KW)[0].tolist()
            scratch = lm.greedy_generate(x, **KW)[0].tolist()
            horizon, whole = _oracle(p, ctx)
            row[s] = dict(ctx=ctx, keys=keys, ids=ids, margins=got[s][1], stats=stats[i], pred=pred, session=sess, scratch=scratch,
                          horizon=horizon, whole=whole)
            if k < 2:
                state[s] = C.next_turn(s, k + 1, ctx, keys, ids, _id_rows(lm, ids), emb_w)
        log.append(row)
    p.update(log=log, graph_captures=dec.graph_captures, dec=dec)
    return p


def test_three_sessions_three_turns_match_a_session_each_and_from_scratch(peaked):
    p, whole = peaked, 0
    lens = set()
    for k, row in enumerate(p["log"]):
        for s in C.SESSIONS:
            r = row[s]
            _gate(r["ids"], r["session"], r["horizon"], r["whole"], (k, s, "DecodeSession"))
            _gate(r["ids"], r["scratch"], r["horizon"], r["whole"], (k, s, "from scratch"))
            whole += bool(r["whole"])
            slot, past, reason = r["pred"]
            S = r["ctx"].shape[0]
            lens.add(S - past)
            assert r["stats"] == dict(context_tokens=S, reused_tokens=past, prefilled_tokens=S - past, full_reprefill_reason=reason)
            if k == 0:
                assert past == 0 and reason == "empty cache"
            else:                                                    # the last context and every id but the last pick
                last = p["log"][k - 1][s]
                assert past == last["ctx"].shape[0] + len(last["ids"]) - 1 and reason is None
    assert whole >= C.MIN_WHOLE, whole                               # a condition of the fixture, picked with the oracle
    assert len(lens) > 3                                             # ragged new-row counts
    assert p["graph_captures"] == 1                                  # one captured step over all three calls


def test_solo_prefill_with_past_gives_the_packed_pass_its_ids(peaked):
    p = peaked
    dec = p["lm"].slot_decoder(C.SLOTS, C.CAPACITY)
    for k, row in enumerate(p["log"]):
        got, stats = _turns(dec, [(s, row[s]["ctx"], row[s]["keys"]) for s in C.SESSIONS], prefill_batch=1)
        assert dec.last_stats["prefill_passes"] == 3
        for i, s in enumerate(C.SESSIONS):
            assert stats[i] == row[s]["stats"]
            _gate(got[s][0], row[s]["ids"], row[s]["horizon"], row[s]["whole"], (k, s))


def test_a_session_sees_nothing_of_its_neighbours_across_turns(peaked):
    """Session "b" between two neighbours, twice: the neighbours' contexts have the same lengths and pasts in both runs but other
    contents.  Equal shapes give equal GEMM plans and rows are independent everywhere but in the attention, so b's turn-2 ids and
    margins can differ only through a leak across a segment or slot boundary.  No stop rule: every turn makes 6 ids."""
    lm, D = peaked["lm"], peaked["lm"].D
    kw = dict(max_new_tokens=6, stop_ids=(), eos_id=-5, min_length=0, prefill_batch=3)
    g = torch.Generator().manual_seed(5)
    b1, b2 = torch.randn(11, D, generator=g) * 0.3, torch.randn(70, D, generator=g) * 0.3     # turn 2 crosses a key tile
    runs = []
    for seed in (6, 7):
        gs = torch.Generator().manual_seed(seed)
        n1 = {"a": torch.randn(5, D, generator=gs) * 0.3, "c": torch.randn(17, D, generator=gs) * 0.3}
        n2 = {"a": torch.randn(9, D, generator=gs) * 0.3, "c": torch.randn(4, D, generator=gs) * 0.3}
        dec = lm.slot_decoder(3, 128)
        ctx = {"a": n1["a"], "b": b1, "c": n1["c"]}
        keys = {s: [("r", s, 0, j) for j in range(ctx[s].shape[0])] for s in ctx}
        got, _ = _turns(dec, [(s, ctx[s], keys[s]) for s in "abc"], **kw)
        for s, new in (("a", n2["a"]), ("b", b2), ("c", n2["c"])):
            ids = got[s][0]
            ctx[s] = torch.cat([ctx[s], _id_rows(lm, ids).cpu(), new], 0)
            keys[s] = keys[s] + [("t", t) for t in ids] + [("r", s, 1, j) for j in range(new.shape[0])]
        first_b = got["b"]
        got, stats = _turns(dec, [(s, ctx[s], keys[s]) for s in "abc"], **kw)
        assert [st["reused_tokens"] for st in stats] == [5 + 5, 11 + 5, 17 + 5]
        assert dec.last_stats["prefill_passes"] == 1
        runs.append((first_b, got))
    assert runs[0][0][0] == runs[1][0][0]                            # b's first turn was the same, so its second context is
    assert runs[0][1]["b"][0] == runs[1][1]["b"][0] and torch.equal(runs[0][1]["b"][1], runs[1][1]["b"][1])
    assert not torch.equal(runs[0][1]["a"][1], runs[1][1]["a"][1])   # the neighbours did differ


def test_edited_and_rolled_back_contexts_reuse_only_what_still_holds(peaked):
    p = peaked
    lm, emb_w = p["lm"], p["emb_w"]
    g = torch.Generator().manual_seed(31)
    a1 = C._tail(12, "row0", emb_w, g)                               # "a": edited at row 4 in turn 2, then extended
    b1 = torch.cat([C._tail(7, "row1", emb_w, g), C._tail(6, "row3", emb_w, g)], 0)   # "b": rolled back to its first 7 rows
    c1 = C._tail(150, "row2", emb_w, g)                              # "c": unchanged -- ONE new row on 149 cached keys, packed
    ctx = dict(a=a1, b=b1, c=c1)
    keys = {s: [("r", s, 0, j) for j in range(ctx[s].shape[0])] for s in ctx}
    dec = lm.slot_decoder(3, 256)
    got, _ = _turns(dec, [(s, ctx[s], keys[s]) for s in "abc"], prefill_batch=3)
    ids_a = got["a"][0]
    a2 = torch.cat([a1, _id_rows(lm, ids_a).cpu(), C._tail(5, "row2", emb_w, g)], 0)
    a2[4] = torch.randn(lm.D, generator=g) * 0.3
    ka = keys["a"] + [("t", t) for t in ids_a] + [("r", "a", 1, j) for j in range(5)]
    ka[4] = ("r", "a", "edited")
    turns = [("a", a2, ka), ("b", b1[:7].clone(), keys["b"][:7]), ("c", c1, keys["c"])]
    got, stats = _turns(dec, turns, prefill_batch=3)
    assert [st["reused_tokens"] for st in stats] == [4, 6, 149]      # the edit's row; len - 1; len - 1
    assert all(st["full_reprefill_reason"] is None for st in stats)
    for s, x, _ in turns:                                            # stale rows past the new context are not seen
        want = lm.greedy_generate(x[None].to(DEV), **KW)[0].tolist()
        horizon, whole = _oracle(p, x)
        _gate(got[s][0], want, horizon, whole, s)
    assert got["b"][0][0] == 201                                     # row1's chain, not row3's that the slot held


def test_a_weights_version_change_and_a_run_in_between_drop_the_cached_rows(peaked):
    p = peaked
    dec = p["lm"].slot_decoder(C.SLOTS, C.CAPACITY)
    turn = lambda k: [(s, p["log"][k][s]["ctx"], p["log"][k][s]["keys"]) for s in C.SESSIONS]
    _turns(dec, turn(0), prefill_batch=3, weights_version=0)
    got, stats = _turns(dec, turn(1), prefill_batch=3, weights_version=1)
    assert [(st["reused_tokens"], st["full_reprefill_reason"]) for st in stats] == [(0, "weights changed")] * 3
    for s in C.SESSIONS:
        r = p["log"][1][s]
        _gate(got[s][0], r["ids"], r["horizon"], r["whole"], s)
    list(dec.run([p["log"][0]["a"]["ctx"]], **KW))                    # overwrites slot 0 from row 0
    got, stats = _turns(dec, turn(2), prefill_batch=3, weights_version=1)
    assert [(st["reused_tokens"], st["full_reprefill_reason"]) for st in stats] == [(0, "empty cache")] * 3
    for s in C.SESSIONS:
        r = p["log"][2][s]
        _gate(got[s][0], r["ids"], r["horizon"], r["whole"], s)
    with pytest.raises(ValueError, match="one turn per session"):
        dec.run_turns(turn(0) + turn(1)[:1], **KW)
    with pytest.raises(ValueError, match="close"):
        list(dec.run_turns([("d", p["log"][0]["a"]["ctx"], p["log"][0]["a"]["keys"])], **KW))
    dec.close("b")
    got, stats = _turns(dec, [("d", p["log"][0]["a"]["ctx"], p["log"][0]["a"]["keys"])])
    assert dec.sessions.slot_of("d") == 1 and stats[0]["full_reprefill_reason"] == "empty cache"
    r = p["log"][0]["a"]
    _gate(got["d"][0], r["ids"], r["horizon"], r["whole"], "d")


def test_three_live_sessions_at_17_slots_take_the_wide_step_with_the_same_ids(peaked):
    p = peaked
    dec = p["lm"].slot_decoder(17, C.CAPACITY)
    for k in (0, 1):
        got, stats = _turns(dec, [(s, p["log"][k][s]["ctx"], p["log"][k][s]["keys"]) for s in C.SESSIONS], prefill_batch=3)
        for i, s in enumerate(C.SESSIONS):
            r = p["log"][k][s]
            assert stats[i] == r["stats"]
            _gate(got[s][0], r["ids"], r["horizon"], r["whole"], (k, s))
    assert dec.graph_captures == 1 and dec.ws["x_in"].shape[0] == 17


# ------------------------------------------------------------------ ChatPool
QUESTIONS = [("Is there a defect?", "Where is it?"), ("Describe the image.", "Is the object damaged?"),
             ("What do you see?", "Is there an anomaly?")]
MAX_NEW = 8


def _open(chat, samples, i):
    conv, imgs = CONV_VISION.copy(), []
    assert chat.upload_img(samples["image"][i:i + 1], conv, imgs, anomaly_maps=samples["anomaly_maps"][i:i + 1])[0] == "Received."
    return conv, imgs


def _context(chat, conv, imgs):
    c = conv.copy()
    c.append_message(c.roles[1], None)
    return chat.get_context_emb(c, imgs)[0]


def test_chat_pool_answers_three_conversations_like_three_solo_chats(model, fx):
    model.eval()
    try:
        samples = _batch(4, train=False, seed=5)
        pool = ChatPool(model, slots=3, capacity=1024)
        solos = [Chat(model, device=DEV) for _ in range(3)]
        convs = [_open(pool, samples, i) for i in range(3)]
        twins = [_open(solos[i], samples, i) for i in range(3)]
        compared = 0
        for t in range(2):
            embs = []
            for i in range(3):
                pool.ask(QUESTIONS[i][t], convs[i][0])
                solos[i].ask(QUESTIONS[i][t], twins[i][0])
                embs.append(_context(pool, *convs[i]))
            out = pool.answer_many(convs, max_new_tokens=MAX_NEW, do_sample=False, prefill_batch=3)
            assert len(out) == 3 and len(pool.last_stats) == 3
            for i in range(3):
                text, _ = solos[i].answer(*twins[i], max_new_tokens=MAX_NEW, do_sample=False)
                ids, ref = pool.last_token_ids[i], solos[i].last_token_ids[0].cpu()
                with torch.no_grad():
                    _, o_mar, o_sc = R.greedy_generate(fx["sd"], embs[i].cpu(), 32, max_new_tokens=MAX_NEW, stop_ids=STOP_WORDS,
                                                       eos_id=2, min_length=1, return_margins=True, return_scales=True)
                horizon = F.two_ulp_horizon(o_mar, o_sc)
                n = min(horizon, ids.shape[0], ref.shape[0])
                assert torch.equal(ids[:n], ref[:n]), (t, i, ids, ref)
                compared += n
                if horizon >= o_mar.shape[1]:
                    assert torch.equal(ids, ref) and out[i][0] == text == convs[i][0].messages[-1][1]
                st = pool.last_stats[i]
                assert st["context_tokens"] == embs[i].shape[1] == st["reused_tokens"] + st["prefilled_tokens"]
                assert (st["reused_tokens"] > 0 and st["full_reprefill_reason"] is None) if t else \
                    (st["reused_tokens"] == 0 and st["full_reprefill_reason"] == "empty cache")
                twins[i][0].messages[-1][1] = convs[i][0].messages[-1][1]      # both go on from the pool's answer
        assert compared > 0 and pool.last_stats[0]["graph_captures"] == 1
        # a fourth conversation needs a slot: refused until one is closed
        conv4 = _open(pool, samples, 3)
        pool.ask("Is there a defect?", conv4[0])
        with pytest.raises(ValueError, match="close"):
            pool.answer_many([conv4], max_new_tokens=MAX_NEW, do_sample=False)
        assert conv4[0].messages[-1][0] == "Human"                   # refused before the conversation was touched
        n_msgs = len(convs[0][0].messages)
        with pytest.raises(ValueError, match="one turn per conversation"):
            pool.answer_many([convs[0], convs[0]], max_new_tokens=MAX_NEW, do_sample=False)
        assert len(convs[0][0].messages) == n_msgs                   # likewise
        pool.close(convs[1][0])
        (text, ids), = pool.answer_many([conv4], max_new_tokens=MAX_NEW, do_sample=False)
        assert isinstance(text, str) and conv4[0].messages[-1] == ["Assistant", text]
        assert pool.decoder.sessions.slot_of(conv4[0]) == 1 and pool.last_stats[0]["full_reprefill_reason"] == "empty cache"
        with pytest.raises(NotImplementedError, match="beam"):
            pool.answer_many([conv4], num_beams=2)
    finally:
        model.train()


def test_a_device_sampled_answer_does_not_depend_on_the_neighbours(model):
    """The same conversation with its own seed, alone in a 3-slot pool and next to two others, two turns each.  prefill_batch = 1:
    a packed pass's row count chooses the GEMM plans, so only the solo prefill gives the conversation the same bits either way;
    the token step's rows are independent."""
    samples = _batch(3, train=False, seed=11)
    model.eval()
    prev = model.llama.device_sampling
    model.llama.device_sampling = True
    try:
        runs = []
        for others in (0, 2):
            pool = ChatPool(model, slots=3, capacity=1024)
            convs = [_open(pool, samples, i) for i in range(1 + others)]
            got = []
            for t in range(2):
                for i, (conv, _) in enumerate(convs):
                    pool.ask(QUESTIONS[i][t], conv)
                pool.answer_many(convs, max_new_tokens=10, do_sample=True, top_p=0.9, temperature=1.0, prefill_batch=1,
                                 seeds=[77 + t, 5, 6][:1 + others])
                got.append(pool.last_token_ids[0])
            assert pool.last_stats[0]["reused_tokens"] > 0
            assert pool.decoder.last_stats["device_sampled_rows"] > 0
            runs.append(got)
        for a, b in zip(*runs):
            assert torch.equal(a, b), (a, b)
    finally:
        model.llama.device_sampling = prev
        model.train()
