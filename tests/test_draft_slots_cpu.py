"""The host side of draft-and-verify decoding in the decode slots, no device in sight: SlotScheduler.step_windows (a window of tokens
per slot per step, cut at that request's own stop), decode_host.slot_guesses (the clamp at the end of a request), the predictor
replay_slot_run(draft=, draft_k=) against a hand-worked run, and the argument refusals that need no device."""
import types

import pytest

from myriad_amd import ops
from myriad_amd.decode import SlotDecoder
from myriad_amd.decode_host import NgramDrafter, SlotScheduler, f32_at_least, replay_slot_run, slot_guesses

STOPS = ((835,), (2277, 29937))


def _sched(slots=2, max_new=10, ordered=False):
    return SlotScheduler(slots, max_new, STOPS, eos_id=2, ordered=ordered)


def test_a_window_is_cut_at_eos_and_the_tokens_past_it_never_appear():
    s = _sched()
    assert s.admit(0, 5, 0.5) and s.admit(1, 6, 0.6)
    fin = s.step_windows({0: ([7, 2, 9, 9], [.1, .2, .3, .4]), 1: ([8], [.7])})
    assert fin == [0] and s.taken == {0: 2, 1: 1} and s.emitted == 3 and s.steps == 1 and s.live_row_steps == 2
    assert s.pop() == [(0, [5, 7, 2], [0.5, 0.1, 0.2])] and s.live() == [1] and s.rows[1][1] == [6, 8]


def test_a_window_is_cut_at_a_two_id_stop_ending_inside_it_and_at_one_that_began_before_it():
    s = _sched()
    s.admit(0, 5, 0.0), s.admit(1, 2277, 0.0)
    fin = s.step_windows({0: ([7, 2277, 29937, 11], [.1, .2, .3, .4]), 1: ([29937, 12, 13], [.5, .6, .7])})
    assert fin == [0, 1] and s.taken == {0: 3, 1: 1} and s.emitted == 4
    assert s.pop() == [(0, [5, 7, 2277, 29937], [0.0, .1, .2, .3]), (1, [2277, 29937], [0.0, .5])]
    s.admit(0, 5, 0.0)
    assert s.step_windows({0: ([835, 1], [.1, .2])}) == [0] and s.pop() == [(2, [5, 835], [0.0, .1])]


def test_a_window_is_cut_at_max_new_tokens():
    s = _sched(slots=1, max_new=4)
    s.admit(0, 5, 0.0)
    assert s.step_windows({0: ([6, 7], [.1, .2])}) == [] and s.taken == {0: 2}
    assert s.step_windows({0: ([8, 9, 10], [.3, .4, .5])}) == [0] and s.taken == {0: 1} and s.emitted == 3
    assert s.pop() == [(0, [5, 6, 7, 8], [0.0, .1, .2, .3])] and s.steps == 2 and s.live_row_steps == 2


def test_a_live_slot_without_a_window_is_an_error():
    s = _sched()
    s.admit(0, 5, 0.0), s.admit(1, 6, 0.0)
    for bad in ({0: ([7], [.1])}, {0: ([7], [.1]), 1: ([], [])}, {0: ([7], [.1]), 1: ([8, 9], [.1])}):
        with pytest.raises(ValueError):
            s.step_windows(bad)
    assert s.steps == 0 and s.emitted == 0 and s.rows[0][1] == [5]


def test_windows_of_one_token_are_step_on_the_same_picks():
    picks = [[7, 8], [2277, 9], [29937, 2], [3, 4], [2, 2]]
    a, b = _sched(), _sched()
    for sc in (a, b):
        sc.admit(0, 5, 0.5), sc.admit(1, 6, 0.6)
    out_a, out_b = [], []
    for t, p in enumerate(picks):
        if not a.live():
            break
        live = a.live()
        assert live == b.live()
        fa = a.step(p, [0.1 * t] * 2)
        fb = b.step_windows({s: ([p[s]], [0.1 * t]) for s in live})
        assert fa == fb and a.taken == b.taken
        out_a += a.pop()
        out_b += b.pop()
    assert out_a == out_b and len(out_a) == 2
    assert (a.steps, a.live_row_steps, a.emitted, a.occupancy) == (b.steps, b.live_row_steps, b.emitted, b.occupancy)


def test_ordered_output_waits_for_every_earlier_request():
    s = _sched(ordered=True)
    s.admit(0, 5, 0.0), s.admit(1, 6, 0.0)
    assert s.step_windows({0: ([7, 8], [.1, .2]), 1: ([9, 2, 4], [.3, .4, .5])}) == [1]
    assert s.pop() == []                                                       # request 1 is done, request 0 is not
    s.admit(1, 3, 0.0)
    assert s.step_windows({0: ([2], [.6]), 1: ([2, 7], [.7, .8])}) == [0, 1]
    assert [r[0] for r in s.pop()] == [0, 1, 2]
    u = _sched()
    u.admit(0, 5, 0.0), u.admit(1, 6, 0.0)
    u.step_windows({0: ([7, 8], [.1, .2]), 1: ([9, 2, 4], [.3, .4, .5])})
    assert [r[0] for r in u.pop()] == [1]                                      # unordered: as it finishes


class Echo:
    """Proposes k times the id 50: as many guesses as it is asked for."""

    def propose(self, history, k):
        return [50] * k


def test_the_guesses_are_clamped_at_the_end_of_a_request():
    s = SlotScheduler(3, 6, (), eos_id=2)
    s.admit(0, 5, 0.0), s.admit(1, 5, 0.0), s.admit(2, 5, 0.0)
    s.step_windows({0: ([6], [0.0]), 1: ([6, 7, 8], [0.0] * 3), 2: ([6, 7, 8, 9], [0.0] * 4)})
    # 2, 4 and 5 of at most 6 tokens: the request can emit 4, 2 and 1 more, of which the fed token's pick is one
    assert slot_guesses(s, Echo(), 4) == {0: [50, 50, 50], 1: [50], 2: []}
    assert slot_guesses(s, Echo(), 8) == {0: [50, 50, 50], 1: [50], 2: []}
    assert slot_guesses(s, Echo(), 2) == {0: [50], 1: [50], 2: []} and slot_guesses(s, Echo(), 1) == {0: [], 1: [], 2: []}
    assert slot_guesses(s, NgramDrafter(), 4) == {0: [], 1: [], 2: []}         # a drafter with nothing: plain steps
    # a window of 1 + guesses tokens then ends the request exactly at max_new_tokens
    s.step_windows({0: ([7, 8, 9, 10], [0.0] * 4), 1: ([9, 10], [0.0] * 2), 2: ([10], [0.0])})
    assert s.live() == [] and all(len(r[1]) == 6 for r in s.pop())


def test_the_predictor_on_a_hand_worked_run_of_three_requests_in_two_slots():
    """K = 4, the drafter knows answer A only.  Step 1 (verify): A's slot is guessed 11 12 13, all right -> 4 tokens; B's slot has
    no guess -> 1.  Step 2 (verify): A is guessed its EOS (1 guess, the window's own pick ends it: nothing accepted), B ends.
    Request C takes slot 0.  Step 3 (verify): guessed 11 12 13, the third is wrong -> 3 tokens, 2 accepted.  Step 4: nothing
    known after 99 -> the plain step, which ends C."""
    A, B, C = [10, 11, 12, 13, 14, 2], [20, 21, 2], [10, 11, 12, 99, 2]
    got = replay_slot_run([5, 7, 6], [A, B, C], slots=2, max_new_tokens=20, stop_ids=(), eos_id=2, draft=NgramDrafter([A]), draft_k=4)
    assert got == dict(prefills=3, prefill_passes=3, packed_rows=18, steps=4, live_row_steps=6, occupancy=0.75, emitted=11,
                       verify_steps=3, plain_steps=1, draft_proposed=7, draft_accepted=5)
    # K = 1 and an untaught drafter: the run without a drafter, every step plain
    plain = replay_slot_run([5, 7, 6], [A, B, C], slots=2, max_new_tokens=20, stop_ids=(), eos_id=2)
    for kw in (dict(draft=NgramDrafter([A]), draft_k=1), dict(draft=NgramDrafter(), draft_k=4)):
        got = replay_slot_run([5, 7, 6], [A, B, C], slots=2, max_new_tokens=20, stop_ids=(), eos_id=2, **kw)
        assert {k: got[k] for k in plain} == plain and got["verify_steps"] == 0
        assert got["plain_steps"] == plain["steps"] == 6                      # A: 5 steps in slot 0; B: 2, then C: 4, in slot 1
        assert got["draft_proposed"] == 0 and got["emitted"] == 11


def test_the_refusals_that_need_no_device():
    on = types.SimpleNamespace(slot_draft=True)
    dec = SlotDecoder(on, 8, 128)
    free = dict(dev_sample=False, penalty=False, min_length=1, scores=False, turns=None)
    assert dec._draft_args(4, **free) == 4 and dec._draft_args(8, **free) == 8 and dec._draft_args(1, **free) == 1
    for k in (0, 9, -1):
        with pytest.raises(ValueError, match="draft_k"):
            dec._draft_args(k, **free)
    with pytest.raises(ValueError, match="rows"):
        SlotDecoder(on, 16, 128)._draft_args(8, **free)   # 128 rows
    assert SlotDecoder(on, 16, 128)._draft_args(4, **free) == 4 and ops.GEMV_WIDE_MAX_ROWS == 64
    for kw, what in ((dict(dev_sample=True), "device sampling"), (dict(penalty=True), "repetition_penalty"),
                     (dict(min_length=2), "min_length"), (dict(scores=True), "return_scores"), (dict(turns=[]), "run_turns")):
        with pytest.raises(NotImplementedError, match=what):
            dec._draft_args(4, **dict(free, **kw))
    with pytest.raises(NotImplementedError, match="num_beams"):
        next(dec.run([], draft=NgramDrafter(), num_beams=2))
    for off in (types.SimpleNamespace(slot_draft=False), types.SimpleNamespace()):     # the switch is off by default
        with pytest.raises(NotImplementedError, match="MYRIAD_SLOT_DRAFT"):
            SlotDecoder(off, 8, 128)._draft_args(4, **free)
    with pytest.raises(NotImplementedError, match="run_turns"):
        dec.run_turns([], draft=NgramDrafter())


def test_eval_aqa_takes_slots_with_draft_k_up_to_64_rows_behind_the_switch(monkeypatch):
    import eval_aqa
    base = ["--cfg-path", "x.yaml"]
    monkeypatch.delenv("MYRIAD_SLOT_DRAFT", raising=False)
    with pytest.raises(SystemExit):                                            # off by default: refused as before
        eval_aqa.parse_args(base + ["--slots", "8", "--draft-k", "4"])
    assert eval_aqa.parse_args(base + ["--draft-k", "4"]).draft_k == 4         # the batch-1 loop needs no switch
    monkeypatch.setenv("MYRIAD_SLOT_DRAFT", "1")
    a = eval_aqa.parse_args(base + ["--slots", "8", "--draft-k", "4", "--bs", "4"])
    assert (a.slots, a.draft_k) == (8, 4) and eval_aqa.parse_args(base + ["--slots", "16", "--draft-k", "4"]).draft_k == 4
    for bad in (["--slots", "16", "--draft-k", "8"], ["--slots", "9", "--draft-k", "8"], ["--draft-k", "4", "--bs", "2"],
                ["--slots", "4", "--draft-k", "4", "--num-beams", "2"], ["--slots", "4", "--draft-k", "4", "--llm-score"],
                ["--slots", "4", "--draft-k", "4", "--num-beams", "2", "--beam-sample"],
                ["--slots", "4", "--draft-k", "4", "--num-beams", "2", "--repetition-penalty", "1.2"]):
        with pytest.raises(SystemExit):
            eval_aqa.parse_args(base + bad)


def test_the_device_threshold_decides_what_the_hosts_double_comparison_decides():
    """The device keeps a row with p_max >= *top_p in f32, the host draws where p_max < top_p with top_p a double: with the smallest
    f32 >= top_p on the device the two agree for every f32 p_max, also where the f32 nearest top_p lies below it (0.9, 0.01)."""
    import numpy as np
    for tp in (0.9, 0.01, 0.5, 0.1, 0.95, 1.0, 0.7):
        t = f32_at_least(tp)
        assert t.dtype == np.float32 and float(t) >= tp and float(np.nextafter(t, np.float32(-np.inf))) < tp
        for p in (np.float32(tp), t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))):
            assert (p >= t) == (not float(p) < tp), (tp, p)
    assert float(np.float32(0.9)) < 0.9 and f32_at_least(0.9) > np.float32(0.9)     # the case round-to-nearest gets wrong


def test_the_engine_loop_runs_without_grad_and_the_argument_check_is_plain():
    assert hasattr(SlotDecoder._run, "__wrapped__") and hasattr(SlotDecoder.run, "__wrapped__")      # torch.no_grad() wraps them
    assert not hasattr(SlotDecoder._draft_args, "__wrapped__")
