"""The host side of draft decoding under the device sampler, the penalty and min_length, without a device: DraftLoop's kept rule,
predict_draft_run / replay_slot_run with the positions the host drew, each against a token-by-token walk; the restatements of
tests/draft_sample_ref.py against a naive one-token-at-a-time penalty + pick loop; eval_aqa.parse_args with the switch on and off."""
import numpy as np
import pytest

from myriad_amd.decode_host import DraftLoop, NgramDrafter, predict_draft_run, replay_slot_run, run_draft_loop
from tests import draft_sample_ref as ref


def _corpus(chain, bad):
    c = list(chain)
    for i in bad:
        c[i] = 9000 + i
    return c


def _walk(chain, drafter, k, min_length, host):
    """One answer, a token at a time: the step counts of the solo loop (fillers count as guesses; a host-drawn row ends its window)."""
    st, n = dict(verify_steps=0, plain_steps=0, draft_proposed=0, draft_accepted=0), 1
    while n < len(chain):
        prop = [] if k < 2 or n < min_length else list(drafter.propose(chain[:n], k - 1))[:k - 1]
        if not prop:
            st["plain_steps"] += 1
            n += 1
            continue
        fed = prop + [0] * (k - 1 - len(prop))
        st["verify_steps"] += 1
        st["draft_proposed"] += len(prop)
        j = 0
        while True:                                                            # row j emits token n + j
            last = j == k - 1 or n + j + 1 >= len(chain) or (n + j) in host or fed[j] != chain[n + j]
            if last:
                break
            j += 1
        st["draft_accepted"] += j
        n += j + 1
    return st


CHAIN = [11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 2]


@pytest.mark.parametrize("host", [(), (3,), (4, 5, 11), (1, 2, 3, 18, 19)])
@pytest.mark.parametrize("min_length", [1, 4])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_the_loop_and_the_predictor_follow_the_walk_with_host_drawn_rows_and_a_ban(k, min_length, host):
    d = NgramDrafter([_corpus(CHAIN, (7, 13))])
    want = _walk(CHAIN, d, k, min_length, set(host))
    assert predict_draft_run(d, CHAIN, k, min_length, host_drawn=host) == want
    assert predict_draft_run(d, CHAIN, k, min_length) == _walk(CHAIN, d, k, min_length, set())      # the argument is optional
    loop = DraftLoop(d, k, 90, stop_ids=(), eos_id=2, min_length=min_length, do_sample=True, top_p=0.9)

    def record(n, rows, guesses):
        """What the device records for rows fed [last token] + guesses at token index n: the true token while every earlier guess
        was right (a host-drawn row shows its arg-max, 7777, and kept -1), garbage behind a wrong guess; n_out by the kept rule."""
        ids, kept, ok, n_out = [], [], True, 1
        for j in range(rows):
            t = n + j
            drawn = t in host
            ids.append((7777 if drawn else CHAIN[t]) if ok and t < len(CHAIN) else 8888)
            kept.append(-1 if drawn else 3)
            ok = ok and j < len(guesses) and t < len(CHAIN) and guesses[j] == CHAIN[t]
        for j in range(rows - 1):
            if kept[j] < 0 or ids[j] != guesses[j]:
                break
            n_out += 1
        return ids, [0.5] * rows, [0.99] * rows, n_out, (lambda j: CHAIN[n + j]), False, kept

    def unpack(r):
        return dict(ids=r[0], margins=r[1], pmax=r[2], n_out=r[3], draw=r[4], first=r[5], kept=r[6])

    loop.take(**dict(unpack(record(0, 1, [])), first=True))
    while not loop.done:
        g = loop.guesses()
        assert loop.fed is None or loop.fed == loop.ids[-1]
        assert not g or len(loop.ids) >= min_length                            # no verify step while the ban is on
        loop.take(**unpack(record(len(loop.ids), 1 + len(g), g)))
    assert loop.ids == CHAIN
    st = loop.stats
    assert {k_: st[k_] for k_ in want} == want, (st, want)
    assert st["host_sampled_rows"] == len(host) and st["device_sampled_rows"] == len(CHAIN) - len(host) and st["sampled_rows"] == 0
    assert st["steps"] == len(CHAIN)


def test_take_without_kept_is_the_p_max_rule_and_a_host_row_inside_a_window_is_an_error():
    loop = DraftLoop(NgramDrafter(), 4, 90, do_sample=True, top_p=0.9)
    loop.take([5], [0.1], [0.5], 1, draw=lambda j: 6, first=True)              # p_max < top_p: the host draws
    assert loop.ids == [6] and loop.fed == 6 and loop.stats["host_sampled_rows"] == loop.stats["sampled_rows"] == 1
    loop.take([7, 8], [0.1, 0.1], [0.5, 0.99], 2, draw=lambda j: 9, kept=[4, 4])   # kept given: p_max decides nothing
    assert loop.ids == [6, 7, 8] and loop.stats["host_sampled_rows"] == 1 and loop.stats["device_sampled_rows"] == 2
    with pytest.raises(ValueError, match="end its window"):
        loop.take([7, 8], [0.1, 0.1], [0.99, 0.99], 2, draw=lambda j: 9, kept=[-1, 4])
    assert run_draft_loop.__name__ == "run_draft_loop"                         # the greedy loop's driver is still there


def _slot_walk(chains, drafter, k, max_new, host):
    """One slot, the requests one after the other, a token at a time: the slot rule (real guesses only, never past max_new)."""
    st = dict(verify_steps=0, plain_steps=0, draft_proposed=0, draft_accepted=0, steps=0)
    for i, chain in enumerate(chains):
        n = 1
        while n < len(chain):
            room = min(k - 1, max_new - n - 1)
            g = [int(t) for t in drafter.propose(chain[:n], room)][:room] if room > 0 else []
            st["steps"] += 1
            if not g:
                st["plain_steps"] += 1
                n += 1
                continue
            st["verify_steps"] += 1
            st["draft_proposed"] += len(g)
            j = 0
            while not (j == len(g) or n + j + 1 >= len(chain) or (n + j) in host[i] or g[j] != chain[n + j]):
                j += 1
            st["draft_accepted"] += j
            n += j + 1
    return st


@pytest.mark.parametrize("k", [2, 4, 8])
def test_replay_slot_run_takes_the_host_drawn_positions(k):
    chains = [CHAIN, [31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 2], [51, 52, 53, 2]]
    d = NgramDrafter([_corpus(chains[0], (9,)), chains[1], chains[2]])
    for host in ([(), (), ()], [(3, 4, 10), (2,), (1,)], [(1, 2, 3, 4, 5, 6), (), (2,)]):
        want = _slot_walk(chains, d, k, 20, [set(h) for h in host])
        got = replay_slot_run([5, 6, 7], chains, 1, 20, stop_ids=(), draft=d, draft_k=k, host_drawn=host)
        assert {n: got[n] for n in want} == want, (k, host, got, want)
    none = replay_slot_run([5, 6, 7], chains, 1, 20, stop_ids=(), draft=d, draft_k=k, host_drawn=[(), (), ()])
    assert replay_slot_run([5, 6, 7], chains, 1, 20, stop_ids=(), draft=d, draft_k=k) == none       # the argument is optional
    # two slots: the host-drawn rows only ever cost steps
    a = replay_slot_run([5, 6, 7], chains, 2, 20, stop_ids=(), draft=d, draft_k=k)
    b = replay_slot_run([5, 6, 7], chains, 2, 20, stop_ids=(), draft=d, draft_k=k, host_drawn=[(3, 4, 10), (2,), (1,)])
    assert b["steps"] >= a["steps"] and b["draft_accepted"] <= a["draft_accepted"] and b["emitted"] == a["emitted"]


# ------------------------------------------------------------------------------------------------ the kernel restatements
def _naive_rows(logits, seen, fed, gen, min_length, eos, pen):
    """The plain loop on one request: token by token, the fed id joins the seen set, every seen id is penalised by scalar
    arithmetic, EOS is banned while the token index is below min_length, the pick is the first arg-max."""
    seen, rows, picks = set(seen), [], []
    for j, t in enumerate(fed):
        seen.add(int(t))
        x = np.array(logits[j], dtype=np.float32)
        for i in seen:
            x[i] = np.float32(x[i] * np.float32(pen)) if x[i] < 0 else np.float32(x[i] / np.float32(pen))
        rows.append(x)
        y = x.copy()
        if gen + j < min_length:
            y[eos] = -np.inf
        best = 0
        for i in range(1, len(y)):
            if y[i] > y[best]:
                best = i
        picks.append(best)
    return rows, picks


@pytest.mark.parametrize("G,K", [(1, 1), (1, 4), (3, 2), (3, 8)])
def test_the_penalty_and_pick_restatements_equal_the_token_by_token_loop(G, K):
    V, eos, min_length, pen = 41, 5, 4, 1.3
    rng = np.random.default_rng(10 * G + K)
    logits = rng.standard_normal((G * K, V)).astype(np.float32) * 3
    logits[:, eos] = 30.0                                                      # the ban decides the pick
    logits[:, 3] = 0.0
    live, nrow, gen = [1, 0, 1][:G], [K, K, max(1, K // 2)][:G], [1, 2, 3][:G]
    seen = [set(rng.integers(0, V, 5).tolist()) | {3} for _ in range(G)]
    ids_k = rng.integers(0, V, G * K)
    for g in range(G):
        ids_k[g * K] = sorted(seen[g])[0]                                      # an extra that is in the bitmap ...
        if K > 2:
            ids_k[g * K + 2] = ids_k[g * K + 1]                                # ... and two equal extras
    pen_rows = ref.penalty_draft_ref(logits, seen, ids_k, nrow, live, K, pen)
    picks = ref.pick_draft_ref(pen_rows, gen, nrow, live, K, min_length, eos)
    for g in range(G):
        sl = slice(g * K, g * K + nrow[g])
        if not live[g]:
            assert np.array_equal(pen_rows[g * K:(g + 1) * K], logits[g * K:(g + 1) * K]) and picks[g * K:(g + 1) * K] == [-1] * K
            continue
        rows, want = _naive_rows(logits[sl], seen[g], ids_k[sl], gen[g], min_length, eos, pen)
        assert np.array_equal(pen_rows[sl].view(np.int32), np.stack(rows).view(np.int32)), (G, K, g)
        assert picks[sl] == want and picks[g * K + nrow[g]:(g + 1) * K] == [-1] * (K - nrow[g])
        assert np.array_equal(pen_rows[g * K + nrow[g]:(g + 1) * K], logits[g * K + nrow[g]:(g + 1) * K])
        assert any(p != eos for p in want[:max(0, min_length - gen[g])]) or min_length <= gen[g]
    assert ref.bitmap_ids(ref.bitmap_of({0, 31, 32, V - 1}, V), V) == {0, 31, 32, V - 1}


def test_the_accept_restatement_is_the_plain_loops_bookkeeping():
    K, V = 4, 100
    nxt, ids = [10, 11, 12, 13], [5, 10, 11, 99]
    base = dict(mar=[0.1] * K, pmx=[0.9] * K, top_p=0.5, pos=7, kv=3, nid=55, gen=2, K=K, V=V)
    # three rows stand (two confirmed guesses + the token behind them): the plain loop would have fed 5, 10, 11 and now feeds 12
    rec, id0, nid, pos, kv, gen, seen = ref.accept_sampled_ref(nxt, kept=[3, 3, 3, 3], ids=ids, nguess=3, live=1, seen_set={1}, **base)
    assert (rec[-1], id0, nid, pos, kv, gen, seen) == (3.0, 12, 12, 10, 11, 5, {1, 5, 10, 11}) and rec[3 * K:4 * K] == [3.0] * K
    # a row the host must draw ends the chain even where the guess behind it is right
    rec, id0, _, pos, _, gen, seen = ref.accept_sampled_ref(nxt, kept=[3, -1, 3, 3], ids=ids, nguess=3, live=1, seen_set={1}, **base)
    assert (rec[-1], id0, pos, gen, seen) == (2.0, 11, 9, 4, {1, 5, 10})
    # without kept the p_max rule; a filler is never confirmed; an idle group keeps everything
    rec = ref.accept_sampled_ref(nxt, kept=None, ids=ids, nguess=1, live=1, seen_set=None, **base)
    assert rec[0][-1] == 2.0 and rec[0][3 * K:4 * K] == [0.0] * K and rec[6] is None
    rec = ref.accept_sampled_ref(nxt, kept=None, ids=ids, nguess=3, live=1, seen_set=None, **dict(base, pmx=[0.9, 0.4, 0.9, 0.9]))
    assert rec[0][-1] == 2.0
    rec = ref.accept_sampled_ref(nxt, kept=[3] * K, ids=ids, nguess=3, live=0, seen_set={1}, **base)
    assert rec == ([-1.0] * K + [0.0] * (3 * K + 1), 5, 55, 7, 3, 2, {1})


def test_eval_aqa_takes_llm_score_with_draft_k_behind_the_switch(monkeypatch):
    import eval_aqa
    base = ["--cfg-path", "x.yaml", "--draft-k", "4", "--llm-score"]
    monkeypatch.setenv("MYRIAD_SLOT_DRAFT", "1")
    monkeypatch.delenv("MYRIAD_DRAFT_SAMPLING", raising=False)
    for extra in ([], ["--slots", "4"]):
        with pytest.raises(SystemExit):                                        # off by default: refused as before
            eval_aqa.parse_args(base + extra)
    monkeypatch.setenv("MYRIAD_DRAFT_SAMPLING", "1")
    a, b = eval_aqa.parse_args(base), eval_aqa.parse_args(base + ["--slots", "4", "--bs", "2"])
    assert a.llm_score and a.draft_k == 4 and b.llm_score and (b.slots, b.draft_k) == (4, 4)
    for bad in (["--num-beams", "2"], ["--slots", "17"], ["--bs", "2"]):       # what the switch does not lift
        with pytest.raises(SystemExit):
            eval_aqa.parse_args(base + bad)
    monkeypatch.setenv("MYRIAD_DRAFT_SAMPLING", "0")
    with pytest.raises(SystemExit):
        eval_aqa.parse_args(base)
