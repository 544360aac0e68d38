"""Draft-and-verify greedy decoding, the host side (myriad_amd/decode_host.py; no GPU): the n-gram drafter, the predictor of a run's
step counts on hand-worked chains, and the loop's window cutting driven by a scripted step that plays the device's part -- it
knows the true chain and answers a K-row verify step the way mh_draft_accept would."""
import json

import pytest

from myriad_amd.decode_host import DraftLoop, NgramDrafter, load_draft_corpus, predict_draft_run, run_draft_loop


# ------------------------------------------------------------------------------------------------ the drafter
def test_an_empty_table_proposes_nothing():
    d = NgramDrafter()
    assert d.propose([], 4) == [] and d.propose([5, 6, 7], 4) == [] and d.propose([5], 0) == []


def test_the_longest_known_suffix_wins_over_a_more_frequent_shorter_one():
    d = NgramDrafter(corpus=[[1, 2, 3, 9], [7, 3, 8], [6, 3, 8]], max_order=4)
    assert d.propose([4, 3], 1) == [8]                # only the 1-gram (3,) is known: 8 twice, 9 once
    assert d.propose([2, 3], 1) == [9]                # (2, 3) is known and says 9, whatever the 1-gram counts say
    assert d.propose([1, 2, 3], 1) == [9]
    assert d.propose([], 1) == [1]                    # the start sentinel is a context: three answers, 1 was seen first


def test_ties_go_to_the_successor_observed_first():
    assert NgramDrafter(corpus=[[5, 1], [5, 2]]).propose([5], 1) == [1]
    assert NgramDrafter(corpus=[[5, 2], [5, 1]]).propose([5], 1) == [2]
    d = NgramDrafter(corpus=[[5, 2], [5, 1]])
    d.observe([5, 1])                                 # 1 now leads by count
    assert d.propose([5], 1) == [1]


def test_a_proposal_extends_on_itself_up_to_k_and_ends_where_the_table_does():
    d = NgramDrafter(corpus=[[10, 11, 12, 13, 2]])
    assert d.propose([10], 3) == [11, 12, 13]
    assert d.propose([10], 8) == [11, 12, 13, 2]      # nothing was ever seen after the last id
    assert d.propose([], 2) == [10, 11]
    assert d.propose([99], 2) == []                   # an unknown id right behind the sentinel: no suffix is known


def test_max_order_bounds_the_context():
    chains = [[1, 2, 3, 4], [9, 2, 3, 5], [9, 2, 3, 5]]
    assert NgramDrafter(chains, max_order=3).propose([1, 2, 3], 1) == [4]
    assert NgramDrafter(chains, max_order=2).propose([1, 2, 3], 1) == [5]
    with pytest.raises(ValueError):
        NgramDrafter(max_order=0)


def test_the_drafter_is_deterministic_and_observe_teaches_it():
    a, b = NgramDrafter(), NgramDrafter()
    for d in (a, b):
        d.observe([3, 4, 5])
        d.observe([3, 4, 6])
    hist = [3, 4]
    assert a.propose(hist, 3) == b.propose(hist, 3) == a.propose(hist, 3) == [5]
    assert hist == [3, 4]                             # the history is the caller's
    assert NgramDrafter([[3, 4, 5], [3, 4, 6]]).table == a.table


def test_corpus_files(tmp_path):
    p = tmp_path / "ids.json"
    p.write_text(json.dumps([[1, 2, 3], [4, 5]]))
    assert load_draft_corpus(str(p)) == [[1, 2, 3], [4, 5]]
    q = tmp_path / "results.jsonl"
    q.write_text("\n".join(json.dumps(dict(output=t, other=1)) for t in ("ab", "c")) + "\n")
    assert load_draft_corpus(str(q), tokenize=lambda s: [ord(c) for c in s]) == [[97, 98], [99]]
    with pytest.raises(ValueError):
        load_draft_corpus(str(q))


# ------------------------------------------------------------------------------------------------ the predictor
CHAIN = list(range(100, 111))                         # 11 ids: the prefill's pick and ten more


def test_predictor_with_a_perfect_drafter():
    d = NgramDrafter([CHAIN])
    # K = 4: ten tokens after the prefill's, windows of 4, 4, 2 (the last one cut by the chain's end: one accepted guess)
    assert predict_draft_run(d, CHAIN, 4) == dict(verify_steps=3, plain_steps=0, draft_proposed=8, draft_accepted=7)
    # (nothing is known to follow 110, so the last window's proposals are 109, 110; the chain's end cuts it after one guess)
    assert predict_draft_run(d, CHAIN, 2) == dict(verify_steps=5, plain_steps=0, draft_proposed=5, draft_accepted=5)
    assert predict_draft_run(d, CHAIN, 1) == dict(verify_steps=0, plain_steps=10, draft_proposed=0, draft_accepted=0)
    assert predict_draft_run(d, CHAIN, 8) == dict(verify_steps=2, plain_steps=0, draft_proposed=9, draft_accepted=8)


def test_predictor_with_an_empty_and_a_wrong_drafter():
    assert predict_draft_run(NgramDrafter(), CHAIN, 4) == dict(verify_steps=0, plain_steps=10, draft_proposed=0, draft_accepted=0)

    class Wrong:
        def propose(self, history, k):
            return [7] * k

    assert predict_draft_run(Wrong(), CHAIN, 4) == dict(verify_steps=10, plain_steps=0, draft_proposed=30, draft_accepted=0)


def test_predictor_with_a_corrupted_corpus_and_a_minimum_length():
    bad = list(CHAIN)
    bad[3] = 999                                      # the drafter believes 102 -> 999 -> 104
    d = NgramDrafter([bad])
    # after 100: guesses 101, 102, 999 -> 101, 102 stand and the step's own pick is 103      (emitted 4)
    # after 103: (102, 103) is unknown, so is (103,): nothing proposed, a plain step -> 104   (emitted 5)
    # after 104: (999, 104) unknown, (104,) -> 105, 106, 107: all three stand, pick 108      (emitted 9)
    # after 108: 109, 110 proposed (nothing follows 110); 109 stands, 110 is the pick that ends the chain (emitted 11)
    assert predict_draft_run(d, CHAIN, 4) == dict(verify_steps=3, plain_steps=1, draft_proposed=8, draft_accepted=6)
    good = NgramDrafter([CHAIN])
    # min_length = 3: the steps that pick tokens 1 and 2 run plain with the EOS ban, then windows of 4 and 4
    assert predict_draft_run(good, CHAIN, 4, min_length=3) == dict(verify_steps=2, plain_steps=2, draft_proposed=6, draft_accepted=6)


# ------------------------------------------------------------------------------------------------ the loop, on a scripted device
class ScriptedDevice:
    """Plays the device for DraftLoop: `chain[i]` is the true greedy token i and `pmax[i]` its p_max; a verify step answers what
    mh_argmax_pmax_rows + mh_draft_accept would.  Past the chain's end the picks are id 1.  Keeps the cache position, to check the
    loop never feeds a token the device did not see."""

    def __init__(self, chain, K, top_p=0.0, pmax=None, drawn=None):
        self.chain, self.K, self.top_p = list(chain), K, top_p
        self.pmax = list(pmax) if pmax is not None else [1.0] * len(chain)
        self.drawn = dict(drawn or {})                # token index -> the id the host draw returns there
        self.n = 1                                    # tokens picked so far = index of the next pick
        self.log = []

    def pick(self, i):
        return (self.chain[i], 0.5 + i, self.pmax[i]) if i < len(self.chain) else (1, 0.0, 1.0)

    def first(self):
        t, m, p = self.pick(0)
        return [t], [m], [p], 1, lambda j: self.drawn[0]

    def plain(self, ban, fed):
        self.log.append(("plain", ban, fed))
        i = self.n
        self.n += 1
        t, m, p = self.pick(i)
        return [t], [m], [p], 1, lambda j: self.drawn[i]

    def verify(self, guesses, fed):
        assert len(guesses) == self.K - 1
        self.log.append(("verify", tuple(guesses), fed))
        i0 = self.n
        fed_ids = [None] + list(guesses)
        picks, valid = [], True
        for j in range(self.K):
            # row j's input is right iff every earlier guess was: only then is its pick the true token
            valid = valid and (j == 0 or fed_ids[j] == self.chain_at(i0 + j - 1))
            picks.append(self.pick(i0 + j) if valid else (3, 0.0, 1.0))
        n_out = 1
        for j in range(self.K - 1):
            if picks[j][0] == fed_ids[j + 1] and (self.top_p <= 0 or picks[j][2] >= self.top_p):
                n_out += 1
            else:
                break
        self.n += n_out
        ids, mar, pm = zip(*picks)
        return list(ids), list(mar), list(pm), n_out, lambda j: self.drawn[i0 + j]

    def chain_at(self, i):
        return self.chain[i] if i < len(self.chain) else 1


def drive(chain, drafter, K, **kw):
    dev_kw = {k: kw.pop(k) for k in ("pmax", "drawn") if k in kw}
    if kw.get("do_sample"):
        dev_kw["top_p"] = kw["top_p"]
    dev = ScriptedDevice(chain, K, **dev_kw)
    loop = DraftLoop(drafter, K, **kw)
    run_draft_loop(loop, dev.first(), dev.plain, dev.verify)
    return loop, dev


def test_loop_emits_the_chain_and_counts_what_the_predictor_counts():
    chain = CHAIN + [2]
    for K in (1, 2, 4, 8):
        for corpus in ([chain], [], [[100, 101, 7, 103, 104, 105, 2]]):
            d = NgramDrafter(corpus)
            loop, dev = drive(chain, d, K, max_new_tokens=90, stop_ids=(), eos_id=2)
            assert loop.ids == chain and loop.margins == [0.5 + i for i in range(len(chain))]
            want = predict_draft_run(d, chain, K)
            assert {k: loop.stats[k] for k in want} == want, (K, corpus)
            assert loop.stats["steps"] == len(chain)
            assert all(e[2] is None for e in dev.log)             # no host draw: the device feeds itself


def test_a_stop_sequence_ending_inside_a_window_cuts_it():
    chain = [50, 51, 2277, 29937, 60, 61, 62, 63]                   # the device would go on past the stop
    loop, dev = drive(chain, NgramDrafter([chain]), 8, max_new_tokens=90, stop_ids=((835,), (2277, 29937)), eos_id=2)
    assert loop.ids == [50, 51, 2277, 29937] and loop.done
    assert [e[0] for e in dev.log] == ["verify"] and loop.stats["verify_steps"] == 1
    assert loop.stats["draft_accepted"] == 2 and len(loop.margins) == 4     # 51, 2277 were confirmed guesses; 29937 the pick
    # the stop's first half at the end of one window, the second at the start of the next
    loop, _ = drive(chain, NgramDrafter([chain]), 2, max_new_tokens=90, stop_ids=((2277, 29937),), eos_id=2)
    assert loop.ids == [50, 51, 2277, 29937] and loop.stats["verify_steps"] == 2


def test_eos_inside_a_window_cuts_it():
    chain = [300, 301, 302, 2, 9, 9, 9]
    loop, dev = drive(chain, NgramDrafter([chain]), 8, max_new_tokens=90, stop_ids=(), eos_id=2)
    assert loop.ids == [300, 301, 302, 2] and loop.stats["draft_accepted"] == 2 and loop.stats["verify_steps"] == 1


def test_max_new_tokens_reached_inside_a_window_cuts_it():
    chain = list(range(200, 230))
    loop, dev = drive(chain, NgramDrafter([chain]), 4, max_new_tokens=7, stop_ids=(), eos_id=2)
    assert loop.ids == chain[:7] and loop.stats["verify_steps"] == 2        # 1 + 4 + (2 of 4)
    assert loop.stats["draft_accepted"] == 3 + 1 and loop.stats["steps"] == 7
    loop, dev = drive(chain, NgramDrafter([chain]), 4, max_new_tokens=1, stop_ids=(), eos_id=2)
    assert loop.ids == chain[:1] and dev.log == []                          # the prefill's pick was all


def test_the_eos_ban_keeps_its_steps_plain():
    chain = list(range(200, 211)) + [2]
    loop, dev = drive(chain, NgramDrafter([chain]), 4, max_new_tokens=90, stop_ids=(), eos_id=2, min_length=3)
    assert loop.ids == chain
    assert [(e[0], e[1]) for e in dev.log[:2]] == [("plain", 2), ("plain", 2)] and dev.log[2][0] == "verify"


def test_a_row_that_needs_a_host_draw_ends_its_window_and_is_fed_back():
    # token 3's p_max is below top_p: the device ends the window there, the host draws 777 in its place and feeds it
    chain = [10, 11, 12, 13, 14, 15, 16, 17]
    pmax = [1.0, 1.0, 1.0, 0.2, 1.0, 1.0, 1.0, 1.0]
    d = NgramDrafter([chain, [777, 14]])
    loop, dev = drive(chain, d, 8, max_new_tokens=6, stop_ids=(), eos_id=2, do_sample=True, top_p=0.9, pmax=pmax, drawn={3: 777})
    # the scripted device keeps its own chain after the draw (its pick after 777 is chain[4]): what matters is the window
    assert loop.ids[:4] == [10, 11, 12, 777]
    assert dev.log[0][0] == "verify" and dev.log[1][2] == 777               # the next step was fed the drawn id
    assert loop.stats["sampled_rows"] == 1 and loop.stats["host_sampled_rows"] == 1 and loop.stats["min_pmax"] == pytest.approx(0.2)
    assert loop.margins[3] == 3.5                                           # the arg-max row's margin, as the plain loop records it
    # the prefill's pick can need a draw too
    loop, dev = drive(chain, NgramDrafter(), 4, max_new_tokens=3, stop_ids=(), eos_id=2, do_sample=True, top_p=0.9,
                      pmax=[0.1] + [1.0] * 7, drawn={0: 55})
    assert loop.ids[0] == 55 and dev.log[0] == ("plain", -1, 55)


def test_take_refuses_a_record_that_breaks_the_rule():
    loop = DraftLoop(NgramDrafter(), 4, 90, do_sample=True, top_p=0.9)
    with pytest.raises(ValueError):
        loop.take([1, 2, 3, 4], [0.0] * 4, [1.0, 0.1, 1.0, 1.0], 3, draw=lambda j: 9)    # a draw row inside the window
    with pytest.raises(ValueError):
        loop.take([1, 2], [0.0] * 2, [1.0] * 2, 3)
