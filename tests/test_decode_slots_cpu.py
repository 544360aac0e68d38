"""The decode-slot scheduler (myriad_amd.llama.SlotScheduler) under a scripted step -- no device anywhere -- and the evaluation
entry point's --slots switch."""
import pytest

from myriad_amd.llama import SlotScheduler

EOS = 2


def _drive(slots, max_new, stops, scripts, ordered=False):
    """Run the scheduler as the engine does, the model replaced by `scripts` (request i emits scripts[i] token by token).
    Returns (results in the order they left, admissions as (request, slot or None), live slots per step, the scheduler)."""
    sched = SlotScheduler(slots, max_new, stops, EOS, ordered=ordered)
    nxt, cur, out, admissions, live_log = 0, {}, [], [], []
    while True:
        for s in sched.free():
            while nxt < len(scripts) and sched.rows[s] is None:
                went_on = sched.admit(s, scripts[nxt][0], 0.5 + nxt)
                admissions.append((nxt, s if went_on else None))
                if went_on:
                    cur[s] = [nxt, 1]
                nxt += 1
        out += sched.pop()
        live = sched.live()
        if not live:
            return out, admissions, live_log, sched
        live_log.append(list(live))
        ids, mar = [-7] * slots, [9.0] * slots                       # idle slots carry junk the scheduler must ignore
        for s in live:
            i, t = cur[s]
            ids[s], mar[s] = scripts[i][t], i + t / 100.0
            cur[s][1] += 1
        sched.step(ids, mar)
        out += sched.pop()


def test_refill_order_stops_eos_and_the_length_limit():
    scripts = [
        [10, 11, 12, 13, 14, 15, 16],       # 0: runs to the limit of 6
        [20, 7, 8, 99],                     # 1: the two-token stop (7, 8) at its third token
        [30, EOS, 99],                      # 2: EOS at its second token
        [40, 41, 5, 99],                    # 3: the one-token stop (5,)
        [8, 50, 7, 51, 7, 8, 99],           # 4: 8 first and 7 later do not stop it: the sequence must be ITS OWN last two ids
    ]
    out, adm, live_log, sched = _drive(2, 6, ((5,), (7, 8)), scripts)
    got = {i: ids for i, ids, _ in out}
    assert got == {0: [10, 11, 12, 13, 14, 15], 1: [20, 7, 8], 2: [30, EOS], 3: [40, 41, 5], 4: [8, 50, 7, 51, 7, 8]}
    # slot 1 frees after step 2 (request 1), takes 2, frees after step 3, takes 3, frees after step 5 with slot 0: 4 goes to slot 0
    assert adm == [(0, 0), (1, 1), (2, 1), (3, 1), (4, 0)]
    assert [i for i, _, _ in out] == [1, 2, 0, 3, 4]                 # completion order
    assert {i: m for i, _, m in out}[1] == [1.5, 1.01, 1.02]         # the admit margin, then each step's own slot's margin
    assert live_log[:5] == [[0, 1]] * 5 and live_log[5:] == [[0]] * 5
    assert sched.steps == 10 and sched.live_row_steps == 15 and sched.occupancy == 15 / 20


def test_a_stop_does_not_straddle_two_requests_in_one_slot():
    # request 0 ends with 7 (at the limit); the slot's next request starts with 8: (7, 8) must not fire across them
    out, _, _, _ = _drive(1, 3, ((7, 8),), [[11, 12, 7, 99], [8, 13, 14, 99]])
    assert [ids for _, ids, _ in out] == [[11, 12, 7], [8, 13, 14]]


def test_a_request_that_ends_on_its_prefill_pick_never_occupies_a_step():
    out, adm, live_log, sched = _drive(2, 4, ((5,),), [[5, 99], [EOS, 99], [60, 61, 5], [70, EOS]])
    assert adm == [(0, None), (1, None), (2, 0), (3, 1)]
    assert [(i, ids) for i, ids, _ in out] == [(0, [5]), (1, [EOS]), (3, [70, EOS]), (2, [60, 61, 5])]
    assert live_log == [[0, 1], [0]] and sched.occupancy == 3 / 4
    out, adm, live_log, sched = _drive(3, 1, (), [[9, 99], [8, 99]])  # max_new_tokens = 1: nothing ever steps
    assert [ids for _, ids, _ in out] == [[9], [8]] and sched.steps == 0 and sched.occupancy == 0.0


def test_ordered_output_waits_for_earlier_requests():
    scripts = [[10, 11, 12, 13, 14], [20, EOS], [30, EOS], [40, 41, EOS]]
    done, _, _, _ = _drive(2, 5, (), scripts)
    assert [i for i, _, _ in done] == [1, 2, 0, 3]                   # out of order as they finish
    out, _, _, _ = _drive(2, 5, (), scripts, ordered=True)
    assert [i for i, _, _ in out] == [0, 1, 2, 3]
    assert sorted(done) == sorted(out)


def test_more_slots_than_requests():
    out, adm, live_log, sched = _drive(4, 3, (), [[11, 12, 13], [14, EOS]])
    assert adm == [(0, 0), (1, 1)] and live_log == [[0, 1], [0]]
    assert sched.free() == [0, 1, 2, 3] and sched.occupancy == 3 / 8
    assert [(i, ids) for i, ids, _ in out] == [(1, [14, EOS]), (0, [11, 12, 13])]
    with pytest.raises(ValueError):
        SlotScheduler(0, 3)
    sched = SlotScheduler(1, 3)
    assert sched.admit(0, 1, 0.0)
    with pytest.raises(ValueError):
        sched.admit(0, 1, 0.0)


def test_eval_entry_point_takes_slots():
    import eval_aqa
    assert eval_aqa.parse_args(["--cfg-path", "x.yaml"]).slots == 0
    assert eval_aqa.parse_args(["--cfg-path", "x.yaml", "--slots", "8"]).slots == 8
