"""Token scores through the decode loops on the tiny golden LLaMA: greedy_generate / DecodeSession / SlotDecoder with
return_scores leave the ids alone, report the log-softmax of the logits the pick was made from (within the derived bound of
tests/token_scores_ref.py), agree bit for bit across slot counts and refill settings, and replay their own captured step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd.decode import DecodeSession  # noqa: E402
from myriad_amd.llama import LlamaHIP  # noqa: E402
from tests import token_scores_ref as T  # noqa: E402
from tests.test_decode_slots_gpu import _requests  # noqa: E402
from tests.test_sampling_gpu import _tiny  # noqa: E402

DEV = "cuda:0"
FREE = dict(stop_ids=(), eos_id=-5, min_length=0)                       # no row ever finishes: every column is a real pick
CONFIGS = {                                                              # name -> (device_sampling, keyword arguments)
    "greedy": (False, dict()),
    "host_draw": (False, dict(do_sample=True, top_p=0.9, temperature=3.0)),
    "device_penalty": (True, dict(do_sample=True, top_p=0.9, repetition_penalty=1.3)),
}


@pytest.fixture(scope="module")
def tiny():
    gd, sd, heads = _tiny()
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    return lm, gd["emb"][:2, :7].to(DEV)


def _gen(lm, emb, name, seed=5, **kw):
    lm.device_sampling, ckw = CONFIGS[name]
    return lm.greedy_generate(emb, generator=torch.Generator().manual_seed(seed), **dict(FREE, **ckw, **kw))


def _scores_ws(lm):
    (ws,) = [w for k, w in lm._decode_ws.items() if k[-1] == "scores"]
    return ws


def _check_column(logits, ids_col, watch, tok_lp, watch_lp, what):
    """One step's scores [B] / [B, W] against the float64 log-softmax of the f32 logits [B, V] they were computed from."""
    x = logits.detach().float().cpu().numpy()
    for b in range(x.shape[0]):
        E = T.bound(T.row_X(x[b]), x.shape[1])
        _, lp = T.ref64(x[b], [int(ids_col[b])] + list(watch))
        got = np.concatenate([[float(tok_lp[b])], watch_lp[b].numpy().astype(np.float64)])
        assert T.within(got, lp, E), (what, b, got, lp, E)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_ids_are_bit_equal_with_scores_on(tiny, name):
    lm, emb = tiny
    off = _gen(lm, emb, name, max_new_tokens=8)
    st_off = dict(lm.last_generate_stats)
    ids, sc = _gen(lm, emb, name, max_new_tokens=8, return_scores=True, watch_ids=[3, 1, 4])
    assert torch.equal(ids, off)
    assert sc["token_logprobs"].shape == (2, 8) and sc["token_logprobs"].dtype == torch.float32
    assert sc["watch_logprobs"].shape == (2, 8, 3) and bool((sc["token_logprobs"] < 0).all())
    st = lm.last_generate_stats
    assert (st["host_sampled_rows"], st["device_sampled_rows"]) == (st_off["host_sampled_rows"], st_off["device_sampled_rows"])
    if name == "host_draw":
        assert st["host_sampled_rows"] > 0                               # the path under test did run
    if name == "device_penalty":
        assert st["device_sampled_rows"] > 0 and st["host_sampled_rows"] == 0
    ids2, mar, sc2 = _gen(lm, emb, name, max_new_tokens=8, return_scores=True, return_margins=True)
    assert torch.equal(ids2, off) and mar.shape == (2, 8) and sc2["watch_logprobs"].shape == (2, 8, 0)
    assert torch.equal(sc2["token_logprobs"], sc["token_logprobs"])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_last_column_is_the_log_softmax_of_the_logits_the_pick_was_made_from(tiny, name):
    lm, emb = tiny
    watch = [0, 7, lm.V - 1]
    lm._decode_ws.clear()                                                # one scores workspace in sight: this configuration's
    for n in range(1, 6):
        ids, sc = _gen(lm, emb, name, max_new_tokens=n, return_scores=True, watch_ids=watch)
        assert ids.shape[1] == n
        ws = _scores_ws(lm)
        # the last pick's logits: the prefill's for n = 1, else the step's buffer -- the penalised row with the penalty on
        logits = lm._prefill(emb, ws["caches"]) if n == 1 else ws["logits"]
        _check_column(logits, ids[:, -1], watch, sc["token_logprobs"][:, -1], sc["watch_logprobs"][:, -1], (name, n))
        if n > 1:                                                        # column 0 against the prefill's logits
            _check_column(lm._prefill(emb, ws["caches"]), ids[:, 0], watch, sc["token_logprobs"][:, 0], sc["watch_logprobs"][:, 0],
                          (name, n, "prefill"))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_a_watched_pick_has_its_watch_log_prob(tiny, name):
    lm, emb = tiny
    ids = _gen(lm, emb, name, max_new_tokens=8)
    watch = list(dict.fromkeys(ids.reshape(-1).tolist()))[:8]
    ids2, sc = _gen(lm, emb, name, max_new_tokens=8, return_scores=True, watch_ids=watch)
    assert torch.equal(ids, ids2)
    hits = 0
    for b in range(ids.shape[0]):
        for t in range(ids.shape[1]):
            if int(ids[b, t]) in watch:
                a, w = sc["token_logprobs"][b, t], sc["watch_logprobs"][b, t, watch.index(int(ids[b, t]))]
                if name == "host_draw":                                  # x[id] - lse on the host: the same f32 subtraction
                    assert abs(float(a) - float(w)) <= T.bound(40.0, lm.V), (b, t, a, w)
                else:
                    assert torch.equal(a, w), (b, t, a, w)
                hits += 1
    assert hits >= 8


def test_finished_rows_are_padded_with_zeros(tiny):
    lm, emb = tiny
    lm.device_sampling = False
    free = lm.greedy_generate(emb, max_new_tokens=6, **FREE)
    eos = int(free[1, 2])                                                # row 1 ends at its third token; row 0 goes on (no stop ids)
    assert eos not in free[0].tolist() and eos not in free[1, :2].tolist()    # the fixture's ids: row 1 alone meets it, at t = 2
    ids, sc = lm.greedy_generate(emb, max_new_tokens=6, stop_ids=(), eos_id=eos, min_length=0, return_scores=True, watch_ids=[eos])
    assert ids[1].tolist() == free[1, :3].tolist() + [eos] * 3
    assert bool((sc["token_logprobs"][1, 3:] == 0).all()) and bool((sc["watch_logprobs"][1, 3:] == 0).all())
    assert bool((sc["token_logprobs"][1, :3] < 0).all()) and bool((sc["token_logprobs"][0] < 0).all())
    assert torch.equal(sc["token_logprobs"][1, 2], sc["watch_logprobs"][1, 2, 0])


def test_the_chat_session_passes_the_scores_through(tiny):
    lm, emb = tiny
    lm.device_sampling = False
    want_ids, want = lm.greedy_generate(emb, max_new_tokens=6, return_scores=True, watch_ids=[2, 9], **FREE)
    sess = DecodeSession(lm, 64)
    keys = [[("e", b, p) for p in range(emb.shape[1])] for b in range(emb.shape[0])]
    plain = sess.generate(emb, keys, max_new_tokens=6, **FREE)
    caps = sess.graph_captures
    ids, sc = sess.generate(emb, keys, reset_reason="again", max_new_tokens=6, return_scores=True, watch_ids=[2, 9], **FREE)
    assert torch.equal(plain, want_ids) and torch.equal(ids, want_ids)
    assert torch.equal(sc["token_logprobs"], want["token_logprobs"]) and torch.equal(sc["watch_logprobs"], want["watch_logprobs"])
    assert sess.graph_captures == caps + 1                               # a view and a graph of its own
    sess.generate(emb, keys, reset_reason="again", max_new_tokens=6, **FREE)
    assert sess.graph_captures == caps + 1 and sess.last_stats["graph_replays"] == 5      # the plain view's graph is still there


# ------------------------------------------------------------------------------------------------ slots
def _run(dec, reqs, **kw):
    out = {}
    for i, ids, mar, sc in dec.run(reqs, return_scores=True, **kw):
        assert sc["token_logprobs"].shape == (len(ids),) and sc["watch_logprobs"].shape[0] == len(ids)
        out[i] = (ids, sc["token_logprobs"], sc["watch_logprobs"])
    return out


def _same(a, b):
    return a.keys() == b.keys() and all(all(torch.equal(x, y) for x, y in zip(a[i], b[i])) for i in a)


@pytest.mark.parametrize("sampled", [False, True])
def test_slot_scores_are_bit_equal_across_settings_and_to_batch_1(tiny, sampled):
    lm, _ = tiny
    lm.device_sampling = sampled
    reqs = _requests([3, 9, 5, 7, 4], lm.D, 21)                          # ragged prompts, more requests than slots
    watch = [0, 5, lm.V - 1]
    kw = dict(max_new_tokens=6, stop_ids=(), watch_ids=watch, **(dict(do_sample=True, top_p=0.9) if sampled else {}))
    # per-request seeds: the i-th draw from a generator is request i's seed in a slot run and, with one generator across the
    # calls, the seed greedy_generate draws for request i alone
    skw = (lambda: dict(generator=torch.Generator().manual_seed(5))) if sampled else dict
    g, alone = skw().get("generator"), {}
    for i, x in enumerate(reqs):
        ids, sc = lm.greedy_generate(x[None].to(DEV), generator=g, return_scores=True, **kw)
        alone[i] = (ids[0], sc["token_logprobs"][0], sc["watch_logprobs"][0])
    runs = {}
    for slots, extra in ((2, {}), (3, {}), (2, dict(prefill_batch=2)), (3, dict(prefill_batch=2, refill_min=2))):
        dec = lm.slot_decoder(slots, 64)
        runs[(slots, tuple(extra))] = _run(dec, reqs, **kw, **skw(), **extra)
        if extra:
            assert dec.last_stats["prefill_passes"] < dec.last_stats["prefills"] == len(reqs)       # some pass was packed
        if sampled:
            assert dec.last_stats["host_sampled_rows"] == 0 and dec.last_stats["device_sampled_rows"] > 0
    for key, got in runs.items():
        for i in alone:
            for x, y, what in zip(got[i], alone[i], ("ids", "token_logprobs", "watch_logprobs")):
                assert torch.equal(x, y), (key, i, what, x, y)
    assert all(_same(got, runs[(2, ())]) for got in runs.values())
    lm.device_sampling = False


def test_slot_host_draws_take_their_log_prob_from_the_row_the_host_read(tiny):
    lm, _ = tiny
    lm.device_sampling = False
    reqs = _requests([4, 6, 5], lm.D, 22)
    kw = dict(max_new_tokens=6, stop_ids=(), do_sample=True, top_p=0.9, temperature=3.0)
    dec = lm.slot_decoder(2, 64)
    off = {i: ids for i, ids, _ in dec.run(reqs, generator=torch.Generator().manual_seed(4), **kw)}
    drawn = dec.last_stats["host_sampled_rows"]
    ids0 = [t for v in off.values() for t in v.tolist()]
    watch = list(dict.fromkeys(ids0))[:8]
    on = _run(dec, reqs, generator=torch.Generator().manual_seed(4), watch_ids=watch, **kw)
    assert drawn > 0 and dec.last_stats["host_sampled_rows"] == drawn
    hits = 0
    for i in off:
        assert torch.equal(on[i][0], off[i])
        for t, tok in enumerate(off[i].tolist()):
            if tok in watch:
                assert abs(float(on[i][1][t]) - float(on[i][2][t, watch.index(tok)])) <= T.bound(40.0, lm.V)
                hits += 1
    assert hits >= 8


def test_a_scores_run_replays_its_own_graph_and_leaves_the_others_alone(tiny):
    lm, emb = tiny
    lm.device_sampling = False
    reqs = _requests([4, 7, 5, 6, 3], lm.D, 23)
    kw = dict(max_new_tokens=8, stop_ids=(), eos_id=-5, min_length=0)
    dec = lm.slot_decoder(2, 64)
    off = {i: ids for i, ids, _ in dec.run(reqs, **kw)}
    assert dec.graph_captures == 1 and dec.last_stats["graph_replays"] == dec.last_stats["steps"] - 2
    on = _run(dec, reqs, watch_ids=[1], **kw)
    assert dec.graph_captures == 2 and dec.last_stats["graph_replays"] == dec.last_stats["steps"] - 2 > 0
    assert all(torch.equal(on[i][0], off[i]) for i in off)
    again = {i: ids for i, ids, _ in dec.run(reqs, **kw)}
    assert dec.graph_captures == 2 and dec.last_stats["graph_replays"] == dec.last_stats["steps"]      # the plain view's graph
    assert all(torch.equal(again[i], off[i]) for i in off)
    _run(dec, reqs, watch_ids=[3, 4, 5], **kw)                           # another watch set: the same graph
    assert dec.graph_captures == 2 and dec.last_stats["graph_replays"] == dec.last_stats["steps"]
    # greedy_generate: a workspace of its own, the plain one untouched
    lm._decode_ws.clear()
    a = lm.greedy_generate(emb, max_new_tokens=8, **FREE)
    (plain,) = lm._decode_ws.values()
    graph = plain["graph"]
    assert graph is not None and plain["rec"].shape[0] == 4
    ids, _ = lm.greedy_generate(emb, max_new_tokens=8, return_scores=True, **FREE)
    assert lm.last_generate_stats["graph_replays"] == lm.last_generate_stats["steps"] - 3 > 0           # prefill, warm-up, capture
    ids, _ = lm.greedy_generate(emb, max_new_tokens=8, return_scores=True, watch_ids=[5], **FREE)
    assert lm.last_generate_stats["graph_replays"] == lm.last_generate_stats["steps"] - 1
    assert len(lm._decode_ws) == 2 and plain["graph"] is graph and torch.equal(ids, a)
    b = lm.greedy_generate(emb, max_new_tokens=8, **FREE)
    assert lm.last_generate_stats["graph_replays"] == 7 and plain["graph"] is graph and torch.equal(a, b)


def test_watch_id_refusals(tiny):
    lm, emb = tiny
    dec = lm.slot_decoder(2, 64)
    for bad in (list(range(9)), [lm.V], [-1], [1.5]):
        with pytest.raises(ValueError, match="watch_ids"):
            lm.greedy_generate(emb, max_new_tokens=2, return_scores=True, watch_ids=bad)
        with pytest.raises(ValueError, match="watch_ids"):
            list(dec.run([emb[0].cpu()], max_new_tokens=2, return_scores=True, watch_ids=bad))
