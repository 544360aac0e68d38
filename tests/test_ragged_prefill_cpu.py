"""The packed-prefill refill logic (myriad_amd.llama.RefillPlanner next to SlotScheduler) under a scripted step -- no device
anywhere: which waiting requests share a prefill pass and when, the row cap, refill_min and its releases, the counters against the
one-request scheduler's, replay_slot_run, the evaluation entry point's switches, and the condition the GPU suite's fp64 kernel
test puts on its inputs."""
import pytest
import torch

from myriad_amd.llama import RefillPlanner, SlotScheduler, replay_slot_run
from tests import fp64_bounds as fb
from tests.ragged_case import H, ragged_inputs

EOS = 2


def _drive(slots, max_new, stops, scripts, lengths=None, ordered=False, **plan_kw):
    """Run scheduler and planner as the engine does, the model replaced by `scripts` (request i emits scripts[i] token by token).
    Returns (results in the order they left, the passes as [(request, slot), ...] with the step each ran after, live slots per
    step, the scheduler, the planner)."""
    lengths = lengths or [4] * len(scripts)
    sched = SlotScheduler(slots, max_new, stops, EOS, ordered=ordered)
    plan = RefillPlanner(sched, range(len(scripts)), length=lambda i: lengths[i], **plan_kw)
    cur, out, passes, live_log = {}, [], [], []
    while True:
        group = plan.next_pass()
        while group:
            passes.append((sched.steps, [(i, s) for s, i in group]))
            for s, i in group:
                if sched.admit(s, scripts[i][0], 0.5 + i):
                    cur[s] = [i, 1]
            group = plan.next_pass()
        out += sched.pop()
        live = sched.live()
        if not live:
            return out, passes, live_log, sched, plan
        live_log.append(list(live))
        ids, mar = [-7] * slots, [9.0] * slots                       # idle slots carry junk the scheduler must ignore
        for s in live:
            i, t = cur[s]
            ids[s], mar[s] = scripts[i][t], i + t / 100.0
            cur[s][1] += 1
        sched.step(ids, mar)
        out += sched.pop()


def _drive_one_by_one(slots, max_new, stops, scripts):
    """The engine's loop before there was a planner (tests/test_decode_slots_cpu.py::_drive): the counters to reproduce."""
    sched = SlotScheduler(slots, max_new, stops, EOS)
    nxt, cur, adm = 0, {}, []
    while True:
        for s in sched.free():
            while nxt < len(scripts) and sched.rows[s] is None:
                if sched.admit(s, scripts[nxt][0], 0.0):
                    cur[s] = [nxt, 1]
                adm.append((sched.steps, [(nxt, s)]))
                nxt += 1
        live = sched.live()
        if not live:
            return sched, adm
        ids = [0] * slots
        for s in live:
            ids[s] = scripts[cur[s][0]][cur[s][1]]
            cur[s][1] += 1
        sched.step(ids, [0.0] * slots)


SCRIPTS = [
    [10, 11, 12, 13, 14, 15, 16],       # 0: runs to the limit of 6
    [20, 7, 8, 99],                     # 1: the two-token stop (7, 8) at its third token
    [30, EOS, 99],                      # 2: EOS at its second token
    [40, 41, 5, 99],                    # 3: the one-token stop (5,)
    [8, 50, 7, 51, 7, 8, 99],           # 4: its own last two ids must be (7, 8)
    [5, 99],                            # 5: ends on its prefill pick
    [60, 61, 62, 5],                    # 6
]
STOPS = ((5,), (7, 8))
WANT = {0: [10, 11, 12, 13, 14, 15], 1: [20, 7, 8], 2: [30, EOS], 3: [40, 41, 5], 4: [8, 50, 7, 51, 7, 8], 5: [5], 6: [60, 61, 62, 5]}


def test_requests_are_admitted_in_input_order_up_to_prefill_batch_per_pass():
    out, passes, _, sched, plan = _drive(3, 6, STOPS, SCRIPTS, prefill_batch=2)
    assert {i: ids for i, ids, _ in out} == WANT
    # three free slots, two requests per pass at most: [0, 1] then [2]; later passes take what is free, lowest slot first
    assert passes[0] == (0, [(0, 0), (1, 1)]) and passes[1] == (0, [(2, 2)])
    order = [i for _, grp in passes for i, _ in grp]
    assert order == list(range(7))                                   # input order, over all passes
    assert all(len(grp) <= 2 for _, grp in passes)
    assert plan.passes == len(passes) and plan.packed_rows == 4 * 7
    out3, passes3, _, _, plan3 = _drive(3, 6, STOPS, SCRIPTS, prefill_batch=3)
    assert passes3[0] == (0, [(0, 0), (1, 1), (2, 2)]) and plan3.passes < plan.passes
    assert {i: ids for i, ids, _ in out3} == WANT


def test_the_row_cap_splits_a_pass_and_a_long_request_goes_alone():
    scripts = [[10, 11, 12]] * 4
    # 40 + 30 = 70 -> 128 rows fits the cap of 128; + 100 would be 192: the third request opens the next pass, 100 + 10 -> 128 fits
    _, passes, _, _, plan = _drive(4, 3, (), scripts, lengths=[40, 30, 100, 10], prefill_batch=4, prefill_rows=128)
    assert [grp for _, grp in passes] == [[(0, 0), (1, 1)], [(2, 2), (3, 3)]]
    assert plan.packed_rows == 180
    # a request longer than the cap still goes, in a pass of its own
    _, passes, _, _, _ = _drive(4, 3, (), scripts[:3], lengths=[300, 10, 20], prefill_batch=4, prefill_rows=128)
    assert [grp for _, grp in passes] == [[(0, 0)], [(1, 1), (2, 2)]]
    _, passes, _, _, _ = _drive(4, 3, (), scripts[:3], lengths=[10, 300, 20], prefill_batch=4, prefill_rows=128)
    assert [grp for _, grp in passes] == [[(0, 0)], [(1, 1)], [(2, 2)]]
    with pytest.raises(ValueError):
        RefillPlanner(SlotScheduler(2, 3), [], prefill_batch=0)


def test_refill_min_waits_for_free_slots_until_nothing_is_live():
    scripts = [[10, EOS], [20, 21, 22, EOS], [30, EOS], [40, EOS], [50, EOS], [60, EOS]]
    _, passes, live_log, _, _ = _drive(2, 6, (), scripts, prefill_batch=2, refill_min=2)
    # request 0 ends after step 1: one free slot < 2 and request 1 is live, so the refill waits; after step 3 nothing is live
    assert passes == [(0, [(0, 0), (1, 1)]), (3, [(2, 0), (3, 1)]), (4, [(4, 0), (5, 1)])]
    assert live_log == [[0, 1], [1], [1], [0, 1], [0, 1]]
    # without the hold the freed slot is refilled at once, one request per pass
    _, passes1, _, _, _ = _drive(2, 6, (), scripts, prefill_batch=2, refill_min=1)
    assert passes1[:2] == [(0, [(0, 0), (1, 1)]), (1, [(2, 0)])]
    # refill_min above the slot count is the slot count
    _, passes9, _, _, _ = _drive(2, 6, (), scripts, prefill_batch=2, refill_min=9)
    assert passes9 == passes


def test_refill_min_lets_go_when_the_requests_have_run_out():
    scripts = [[10, EOS], [20, 21, 22, 23, EOS], [30, 31, EOS]]
    _, passes, live_log, _, _ = _drive(2, 6, (), scripts, prefill_batch=2, refill_min=2)
    # after step 1 one slot is free and request 1 is live, but request 2 is the last: it does not wait
    assert passes == [(0, [(0, 0), (1, 1)]), (1, [(2, 0)])]
    assert live_log == [[0, 1], [0, 1], [0, 1], [1]]


def test_a_first_pick_finish_leaves_its_slot_for_the_next_round():
    out, passes, live_log, sched, _ = _drive(2, 4, ((5,),), [[5, 99], [EOS, 99], [60, 61, 5], [70, EOS]], prefill_batch=2)
    assert passes == [(0, [(0, 0), (1, 1)]), (0, [(2, 0), (3, 1)])]  # both slots stayed free: the next pass takes them again
    assert [(i, ids) for i, ids, _ in out] == [(0, [5]), (1, [EOS]), (3, [70, EOS]), (2, [60, 61, 5])]
    assert live_log == [[0, 1], [0]] and sched.occupancy == 3 / 4
    # one of two ends at once: the next pass holds one request, for that slot
    _, passes, _, _, _ = _drive(2, 4, ((5,),), [[60, 61, 5], [5, 99], [70, EOS]], prefill_batch=2)
    assert passes == [(0, [(0, 0), (1, 1)]), (0, [(2, 1)])]


def test_ordered_output_with_packed_passes():
    scripts = [[10, 11, 12, 13, 14], [20, EOS], [30, EOS], [40, 41, EOS]]
    done, _, _, _, _ = _drive(2, 5, (), scripts, prefill_batch=2)
    assert [i for i, _, _ in done] == [1, 2, 0, 3]
    out, _, _, _, _ = _drive(2, 5, (), scripts, ordered=True, prefill_batch=2)
    assert [i for i, _, _ in out] == [0, 1, 2, 3] and sorted(done) == sorted(out)


@pytest.mark.parametrize("slots", [1, 2, 3, 8])
def test_one_request_per_pass_reproduces_the_present_scheduler(slots):
    for scripts, stops, max_new in ((SCRIPTS, STOPS, 6), ([[5, 99], [EOS, 99], [60, 61, 5], [70, EOS]], ((5,),), 4),
                                    ([[9, 99], [8, 99]], (), 1)):
        old, adm = _drive_one_by_one(slots, max_new, stops, scripts)
        out, passes, _, sched, plan = _drive(slots, max_new, stops, scripts, prefill_batch=1, refill_min=1)
        assert passes == adm                                         # the same request into the same slot after the same step
        assert (sched.steps, sched.live_row_steps, sched.occupancy) == (old.steps, old.live_row_steps, old.occupancy)
        assert plan.passes == len(scripts)
        ids = {i: got for i, got, _ in out}
        r = replay_slot_run([4] * len(scripts), [ids[i] for i in range(len(scripts))], slots, max_new, stops, EOS)
        assert (r["steps"], r["live_row_steps"], r["prefill_passes"], r["prefills"]) == (old.steps, old.live_row_steps,
                                                                                         len(scripts), len(scripts))


def test_replay_equals_the_driven_run():
    for kw in (dict(prefill_batch=3), dict(prefill_batch=3, refill_min=2), dict(prefill_batch=2, refill_min=3, prefill_rows=64)):
        lengths = [5, 23, 9, 14, 7, 18, 11]
        _, _, _, sched, plan = _drive(3, 6, STOPS, SCRIPTS, lengths=lengths, **kw)
        r = replay_slot_run(lengths, [WANT[i] for i in range(7)], 3, 6, STOPS, EOS, **kw)
        assert r == dict(prefills=7, prefill_passes=plan.passes, packed_rows=plan.packed_rows, steps=sched.steps,
                         live_row_steps=sched.live_row_steps, occupancy=sched.occupancy)
        assert r["packed_rows"] == sum(lengths)


def test_eval_entry_point_takes_the_packed_prefill_switches(monkeypatch, tmp_path):
    import eval_aqa
    a = eval_aqa.parse_args(["--cfg-path", "x.yaml", "--slots", "8"])
    assert (a.prefill_batch, a.refill_min) == (1, 1)
    a = eval_aqa.parse_args(["--cfg-path", "x.yaml", "--slots", "8", "--prefill-batch", "4", "--refill-min", "2"])
    assert (a.slots, a.prefill_batch, a.refill_min) == (8, 4, 2)
    seen = {}

    class Model:
        last_generate_stats = {}

        def generate_stream(self, batches, **kw):
            seen.update(kw)
            return iter(())

    monkeypatch.setattr(torch.cuda, "synchronize", lambda *x: None)
    monkeypatch.setattr(torch.cuda, "max_memory_allocated", lambda *x: 0)
    assert eval_aqa._run_slots(a, Model(), [], {"max_new_tokens": 3}, str(tmp_path / "r.jsonl")) == []
    assert seen == dict(slots=8, prefill_batch=4, refill_min=2, max_new_tokens=3)


def _heads(t, n, D):
    return t.reshape(1, n, H, D).transpose(1, 2)


def test_rope_exempt_share_of_the_ragged_kernel_case():
    """The condition of the GPU suite's fp64 kernel test, which needs no device: its segments and positions leave at most 1 % of
    the rotated elements ambiguous and no whole row."""
    for D in (16, 128):
        qkv, seg, _, pos = ragged_inputs(D, "cpu")
        cos, sin = fb.rope_tables(D)
        W = H * D
        for r0, n, _ in seg:
            if n == 1:
                continue
            for i in (0, 1):
                x = _heads(qkv[r0:r0 + n, i * W:(i + 1) * W].float(), n, D)
                fb.assert_rope_exempt_share(fb.rope_bf16(x, pos[r0:r0 + n].long()[None], cos, sin)[1], f"D={D} len={n} {'qk'[i]}")
