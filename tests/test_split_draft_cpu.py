"""Draft decoding in SlotDecoder.run_turns, without a device: the scheduling of `_run` for turns with a drafter, driven by scripted
picks -- windows cut at each turn's own stop, the step counts replay_slot_run predicts, no row fed past context + max_new_tokens -
1, and after a turn the session's key list holds only the tokens that stood -- and the `draft_split` switch against `slot_draft`
and `draft_sampling`."""
import itertools
import types

import pytest

from myriad_amd.decode import SlotDecoder
from myriad_amd.decode_host import NgramDrafter, SessionTable, SlotScheduler, TurnPlanner, replay_slot_run, slot_guesses

STOPS, EOS, MAX_NEW = ((835,), (77, 78)), 2, 12
COUNTS = ("steps", "verify_steps", "plain_steps", "draft_proposed", "draft_accepted", "emitted", "prefills", "prefill_passes",
          "packed_rows", "live_row_steps")


def _call(table, turns, scripts, drafter, K, slots, prefill_batch=1):
    """One run_turns call as SlotDecoder._run schedules it.  turns = [(session, keys)], scripts[i] = the picks the device makes for
    turn i at token 0, 1, ... while every earlier token was fed (they run on past the turn's stop: the device knows no stop rule).
    Returns ({session: ids}, counters, the (first, last) position fed per step and slot)."""
    begun = table.plan([(s, list(k)) for s, k in turns], ("v", 0, None))
    plan = TurnPlanner([(slot, (i, len(turns[i][1]) - past)) for i, (slot, past, _) in enumerate(begun)], prefill_batch, 2048,
                       length=lambda q: q[1])
    sched = SlotScheduler(slots, MAX_NEW, STOPS, EOS)
    st = dict(verify_steps=0, plain_steps=0, draft_proposed=0, draft_accepted=0, prefills=0)
    owner, out, fed = {}, {}, []

    def results():
        for index, ids, _ in sched.pop():
            table.end(turns[index][0], turns[index][1], ids)
            out[turns[index][0]] = list(ids)

    while True:
        group = plan.next_pass()
        while group:
            for slot, (i, _) in group:
                st["prefills"] += 1
                if sched.admit(slot, scripts[i][0], 0.0):
                    owner[slot] = i
            group = plan.next_pass()
        results()
        live = sched.live()
        if not live:
            break
        guesses = slot_guesses(sched, drafter, K) if K > 1 else {s: [] for s in live}
        verify = any(guesses[s] for s in live)
        windows = {}
        for s in live:
            script, n, ctx = scripts[owner[s]], len(sched.rows[s][1]), len(turns[owner[s]][1])
            take = 1                                                         # the device's rule: the leading guesses the picks confirm
            while take <= len(guesses[s]) and n + take < len(script) and guesses[s][take - 1] == script[n + take - 1]:
                take += 1
            windows[s] = (script[n:n + take], [0.0] * take)
            fed.append((ctx + n - 1, ctx + n - 1 + len(guesses[s]), ctx))
        sched.step_windows(windows)
        st["verify_steps" if verify else "plain_steps"] += 1
        if verify:
            st["draft_proposed"] += sum(len(guesses[s]) for s in live)
            st["draft_accepted"] += sum(sched.taken[s] - 1 for s in live)
        results()
    st.update(steps=sched.steps, emitted=sched.emitted, prefill_passes=plan.passes, packed_rows=plan.packed_rows,
              live_row_steps=sched.live_row_steps)
    return out, st, fed, begun


def _answer(script):
    """Where the stop rule ends a script."""
    s = SlotScheduler(1, MAX_NEW, STOPS, EOS)
    for n in range(1, len(script) + 1):
        if s._ended(script[:n]):
            return script[:n]
    raise AssertionError("the script never ends")


@pytest.mark.parametrize("K", [2, 4, 8])
@pytest.mark.parametrize("prefill_batch", [1, 3])
def test_turns_with_a_drafter_cut_windows_at_their_own_stop_and_record_only_what_stood(K, prefill_batch):
    # three conversations: a one-id stop, EOS, a two-id stop ending inside a window, and one that runs to max_new_tokens; every
    # script goes on past its end with ids the drafter knows, so a window reaches past the stop
    first = {"a": [10, 11, 12, 835, 13, 14, 15, 16], "b": [20, 21, 22, 23, 24, 2, 25, 26, 27], "c": [30, 77, 78, 31, 32, 33, 34]}
    second = {"a": [40 + j for j in range(MAX_NEW + 6)], "b": [50, 51, 77, 99, 78, 52, 2, 53], "c": [60, 2, 61, 62]}
    drafter = NgramDrafter(list(first.values()) + list(second.values()))
    table = SessionTable(3)
    keys = {s: [("r", s, 0, j) for j in range(5 + 3 * i)] for i, s in enumerate("abc")}
    for k, scripts in enumerate((first, second)):
        turns = [(s, keys[s]) for s in "abc"]
        out, st, fed, begun = _call(table, turns, [scripts[s] for s in "abc"], drafter, K, 3, prefill_batch)
        begun_past = {s: past for s, (_, past, _) in zip("abc", begun)}
        answers = [_answer(scripts[s]) for s in "abc"]
        assert [out[s] for s in "abc"] == answers                             # cut at each turn's own stop, nothing past it
        lens = [len(keys[s]) - begun_past[s] for s in "abc"]
        want = replay_slot_run(lens, answers, 3, MAX_NEW, stop_ids=STOPS, eos_id=EOS, prefill_batch=prefill_batch, draft=drafter, draft_k=K)
        assert {c: st[c] for c in COUNTS} == {c: want[c] for c in COUNTS}, (st, want)
        assert st["verify_steps"] > 0 and st["draft_accepted"] > 0
        assert all(first_ <= last <= ctx + MAX_NEW - 1 for first_, last, ctx in fed)      # no row past context + max_new_tokens - 1
        assert any(last > first_ for first_, last, _ in fed)
        for s, ids in zip("abc", answers):                                    # the recorded keys: the context and the ids that stood
            assert table.keys_of(s) == keys[s] + [("t", t) for t in ids[:-1]]
            if k == 0:
                assert begun_past[s] == 0
                keys[s] = keys[s] + [("t", t) for t in ids] + [("r", s, 1, j) for j in range(4)]
            else:                                                              # turn 2 reuses the context and every id but the last
                assert begun_past[s] == len(keys[s]) - 4 - 1
    assert len(second["a"]) > MAX_NEW and len(_answer(second["a"])) == MAX_NEW


def test_a_wrong_drafter_costs_rows_never_a_step_and_leaves_the_keys_alone():
    class Wrong:
        def propose(self, history, k):
            return [7] * k

    scripts = [[10, 11, 12, 835], [20, 21, 2]]
    table, keys = SessionTable(2), [[("r", 0, j) for j in range(6)], [("r", 1, j) for j in range(9)]]
    out, st, _, _ = _call(table, [("a", keys[0]), ("b", keys[1])], scripts, Wrong(), 4, 2)
    plain = replay_slot_run([6, 9], scripts, 2, MAX_NEW, stop_ids=STOPS, eos_id=EOS)
    assert out == {"a": scripts[0], "b": scripts[1]} and st["steps"] == plain["steps"] == st["verify_steps"] and st["draft_accepted"] == 0
    assert table.keys_of("a") == keys[0] + [("t", 10), ("t", 11), ("t", 12)] and table.keys_of("b") == keys[1] + [("t", 20), ("t", 21)]


def test_the_switch_against_slot_draft_and_draft_sampling():
    free = dict(dev_sample=False, penalty=False, min_length=1, scores=False)
    tails = (dict(dev_sample=True), dict(penalty=True), dict(min_length=2), dict(scores=True))
    d = NgramDrafter()
    for slot_draft, draft_split, draft_sampling in itertools.product((False, True), repeat=3):
        L = types.SimpleNamespace(slot_draft=slot_draft, draft_split=draft_split, draft_sampling=draft_sampling)
        dec = SlotDecoder(L, 4, 128)
        for turns in (None, [("s", None, [])]):
            ok = slot_draft and (turns is None or draft_split)
            if ok:
                assert dec._draft_args(4, turns=turns, **free) == 4
            else:
                with pytest.raises(NotImplementedError, match="run_turns" if slot_draft else "MYRIAD_SLOT_DRAFT"):
                    dec._draft_args(4, turns=turns, **free)
            for kw in tails:                                                   # the tails stay behind draft_sampling, turns or not
                if ok and draft_sampling:
                    assert dec._draft_args(4, turns=turns, **dict(free, **kw)) == 4
                else:
                    with pytest.raises(NotImplementedError):
                        dec._draft_args(4, turns=turns, **dict(free, **kw))
        if draft_split:                                                        # run_turns hands `draft` on to the engine (a generator)
            assert hasattr(dec.run_turns([], draft=d, draft_k=4), "__next__")
        else:
            with pytest.raises(NotImplementedError, match="MYRIAD_DRAFT_SPLIT"):
                dec.run_turns([], draft=d)
        with pytest.raises(NotImplementedError, match="beam"):
            dec.run_turns([], draft=d if draft_split else None, num_beams=2)
