"""The host side of ranking candidate answers by log-likelihood -- no device anywhere: the condition the GPU suite's fp64 test of
mh_attn_prefill_ragged_shared puts on its inputs (tests/shared_prefix_case.py), decode_host.ScorePlan (which rows a scoring pass
packs, what each row's logits score) and eval_protocol.answer_anomaly_score."""
import math

import pytest
import torch

from myriad_amd import eval_protocol as EP
from myriad_amd.decode_host import ScorePlan
from tests import fp64_bounds as fb
from tests import ragged_past_case as pc
from tests.shared_prefix_case import (H, ONE_ROW_SHARED_SLOTS, SHARED_SLOTS, T_CAP, one_row_shared_inputs, shared_inputs)


def test_the_shared_case_is_the_past_case_with_repeating_slots():
    for D in (16, 128):
        for mine, theirs, slots in ((shared_inputs, pc.past_inputs, SHARED_SLOTS),
                                    (one_row_shared_inputs, pc.one_row_inputs, ONE_ROW_SHARED_SLOTS)):
            qkv, prefix, seg, M, pos = mine(D, "cpu")
            qkv0, _, seg0, M0, pos0 = theirs(D, "cpu")
            assert torch.equal(qkv.view(torch.int16), qkv0.view(torch.int16)) and M == M0 and torch.equal(pos, pos0)
            assert [(r, n, p) for r, n, _, p in seg] == [(r, n, p) for r, n, _, p in seg0] and [s[2] for s in seg] == slots
            assert len(set(slots)) < len(slots)
            for s, pre in prefix.items():
                assert pre.shape == (max(p for _, _, slot, p in seg if slot == s), 2 * H * D)
    assert [(p, n) for (_, n, _, p) in shared_inputs(16, "cpu")[2]] == [(0, 17), (1, 64), (63, 2), (64, 65), (65, 1), (130, 100),
                                                                       (192, 64)]
    assert [(p, n) for (_, n, _, p) in one_row_shared_inputs(16, "cpu")[2]] == [(112, 1), (128, 1), (200, 1), (255, 1)]


def test_rope_exempt_share_of_the_shared_kernel_case():
    """tests/test_ragged_past_cpu.py's condition, on this module's output: every segment of at least 16 rows leaves at most 1 %
    of the rotated elements ambiguous and no whole row; a shorter segment no wholly ambiguous row."""
    for D, inputs in [(D, f) for D in (16, 128) for f in (shared_inputs, one_row_shared_inputs)]:
        qkv, _, seg, _, pos = inputs(D, "cpu")
        assert max(p + n for _, n, _, p in seg) == T_CAP
        cos, sin = fb.rope_tables(D)
        W = H * D
        for r0, n, _, past in seg:
            for i in (0, 1):
                x = qkv[r0:r0 + n, i * W:(i + 1) * W].float().reshape(1, n, H, D).transpose(1, 2)
                unc = fb.rope_bf16(x, pos[r0:r0 + n].long()[None], cos, sin)[1]
                what = f"D={D} past={past} len={n} {'qk'[i]}"
                if n >= 16:
                    fb.assert_rope_exempt_share(unc, what)
                else:
                    assert not bool((unc > 0).all(-1).any()), f"{what}: a whole row is ambiguous"


# ------------------------------------------------------------------------------------------------ the planner
V, MAX_POS = 100, 512
LENS = [7, 150, 30]
CANDS = [[[5], [6, 7], [8, 9, 10, 11, 12]],
         [[1, 2, 3], [4]],
         [list(range(20, 60)), list(range(60, 70)), [99]]]


def _check_plan(plan, lens, cands, slots_cap, rows_cap):
    """Every rule of the plan that does not depend on where the passes were cut."""
    scored = {}
    assert sorted(i for g in plan.groups for i in g["prompts"]) == list(range(len(lens)))
    for g in plan.groups:
        assert len(g["prompts"]) <= slots_cap and g["slots"] == list(range(len(g["prompts"])))
        assert len(g["prompts"]) == 1 or ((sum(lens[i] for i in g["prompts"]) + 63) // 64) * 64 <= rows_cap
        slot_of = dict(zip(g["prompts"], g["slots"]))
        # first tokens: the prompt's last prefill row, replicated once per candidate
        assert [(i, c) for i, c, _ in g["first_map"]] == [(i, c) for i in g["prompts"] for c in range(len(cands[i]))]
        for row, tgt, (i, c, j) in zip(g["first_rows"], g["first_targets"], g["first_map"]):
            assert j == 0 and row == slot_of[i] and tgt == cands[i][c][0]
            assert scored.setdefault((i, c, 0), "first") == "first"
        assert len(g["first_rows"]) == len(g["first_targets"]) == len(g["first_map"])
        seen = set()
        for ps in g["passes"]:
            n = len(ps["ids"])
            assert ps["M"] % 64 == 0 and n <= ps["M"] < n + 64 and ps["seg"]
            assert len(ps["seg"]) == 1 or ps["M"] <= rows_cap          # the caps; the first of a pass always goes
            assert n == len(ps["pos"]) == len(ps["targets"]) == len(ps["map"])
            row = 0
            for r0, ln, slot, past in ps["seg"]:
                assert r0 == row and ln >= 1 and r0 + ln <= ps["M"]    # disjoint, back to back, inside the frame
                i, c, j0 = ps["map"][r0]
                assert j0 == 1 and slot == slot_of[i] and past == lens[i] and ln == len(cands[i][c]) - 1   # never split
                assert (i, c) not in seen
                seen.add((i, c))
                for k in range(ln):
                    assert ps["map"][r0 + k] == (i, c, k + 1)
                    assert ps["ids"][r0 + k] == cands[i][c][k] and ps["targets"][r0 + k] == cands[i][c][k + 1]
                    assert ps["pos"][r0 + k] == lens[i] + k
                    assert scored.setdefault((i, c, k + 1), "row") == "row"
                row += ln
            assert row == n
        # one-token candidates produce no segment
        assert seen == {(i, c) for i in g["prompts"] for c, ids in enumerate(cands[i]) if len(ids) > 1}
    # every token of every candidate is scored exactly once
    assert set(scored) == {(i, c, j) for i, cs in enumerate(cands) for c, ids in enumerate(cs) for j in range(len(ids))}
    assert plan.passes == sum(1 + len(g["passes"]) for g in plan.groups)
    assert plan.segments == sum(len(ps["seg"]) for g in plan.groups for ps in g["passes"])
    assert plan.packed_rows == sum(lens) + sum(len(ids) - 1 for cs in cands for ids in cs)


def test_plan_of_one_group_is_two_passes():
    plan = ScorePlan(LENS, CANDS, V, MAX_POS)
    _check_plan(plan, LENS, CANDS, 8, 2048)
    assert plan.passes == 2 and len(plan.groups) == 1
    g = plan.groups[0]
    assert g["first_rows"] == [0, 0, 0, 1, 1, 2, 2, 2] and g["first_targets"] == [5, 6, 8, 1, 4, 20, 60, 99]
    assert g["passes"][0]["seg"] == [(0, 1, 0, 7), (1, 4, 0, 7), (5, 2, 1, 150), (7, 39, 2, 30), (46, 9, 2, 30)]
    assert g["passes"][0]["M"] == 64 and g["passes"][0]["pos"][:5] == [7, 7, 8, 9, 10]
    assert (plan.segments, plan.packed_rows) == (5, 187 + 55)


@pytest.mark.parametrize("slots_cap,rows_cap", [(1, 2048), (2, 2048), (8, 64), (2, 64), (8, 128), (8, 192)])
def test_caps_are_honoured_and_no_candidate_is_split(slots_cap, rows_cap):
    _check_plan(ScorePlan(LENS, CANDS, V, MAX_POS, slots_cap, rows_cap), LENS, CANDS, slots_cap, rows_cap)


def test_an_overflowing_prompt_is_revisited_with_the_same_slot_and_past():
    cands = [[list(range(40)) for _ in range(4)], [[1, 2]]]          # 4 x 39 rows against a cap of 64: one candidate per pass
    plan = ScorePlan([10, 20], cands, V, MAX_POS, 8, 64)
    _check_plan(plan, [10, 20], cands, 8, 64)
    (g,) = plan.groups
    assert [ps["seg"] for ps in g["passes"]] == [[(0, 39, 0, 10)]] * 3 + [[(0, 39, 0, 10), (39, 1, 1, 20)]]
    assert plan.passes == 1 + 4                                      # ONE prompt prefill: the prompt stays cached
    # a candidate longer than the cap goes alone, whole
    long_ = ScorePlan([10], [[list(range(90)), [3, 4]]], V, MAX_POS, 8, 64)
    assert [ps["seg"] for ps in long_.groups[0]["passes"]] == [[(0, 89, 0, 10)], [(0, 1, 0, 10)]]
    assert long_.groups[0]["passes"][0]["M"] == 128


def test_plan_refusals():
    for lens, cands, why in [([5], [[[]]], "empty"),                               # an empty candidate
                             ([5], [[]], "empty candidate list"),
                             ([5], [[[1, V]]], "outside"),                         # an id outside [0, V)
                             ([5], [[[-1]]], "outside"),
                             ([5], [[[1] * (MAX_POS - 3)]], "rotary"),             # S + n - 1 = MAX_POS + 1
                             ([5, 6], [[[1]]], "per prompt"),
                             ([], [], "per prompt"),
                             ([0], [[[1]]], "no rows")]:
        with pytest.raises(ValueError, match=why):
            ScorePlan(lens, cands, V, MAX_POS)
    ScorePlan([5], [[[1] * (MAX_POS - 4)]], V, MAX_POS)              # S + n - 1 = MAX_POS: the last fed position is MAX_POS - 1
    with pytest.raises(ValueError):
        ScorePlan([5], [[[1]]], V, MAX_POS, slots=0)


# ------------------------------------------------------------------------------------------------ the anomaly score
def test_answer_anomaly_score_known_values():
    assert EP.answer_anomaly_score([-3.0, -3.0]) == 0.5              # two equal log-probs
    assert EP.answer_anomaly_score([math.log(0.3), math.log(0.1)]) == pytest.approx(0.75, rel=1e-12)
    assert EP.answer_anomaly_score([math.log(0.1), math.log(0.3), math.log(0.6)]) == pytest.approx(0.1, rel=1e-12)
    assert EP.answer_anomaly_score(torch.tensor([-40.0, -41.0], dtype=torch.float64)) == pytest.approx(1 / (1 + math.exp(-1)),
                                                                                                      rel=1e-12)
    assert EP.answer_anomaly_score([-2.0]) == 1.0


def test_answer_anomaly_score_without_nan_at_the_extremes():
    inf = float("inf")
    assert EP.answer_anomaly_score([-inf, -1.0]) == 0.0 and EP.answer_anomaly_score([-1.0, -inf]) == 1.0
    assert EP.answer_anomaly_score([-inf, -inf]) == 0.5
    assert EP.answer_anomaly_score([-1e30, -1.0]) == 0.0 and EP.answer_anomaly_score([-1.0, -1e30]) == 1.0
    assert EP.answer_anomaly_score([-5000.0, -5001.0]) == pytest.approx(1 / (1 + math.exp(-1)), rel=1e-12)   # exp underflows alone


def test_answer_anomaly_score_is_invariant_under_a_constant():
    row = [-12.5, -14.0, -13.25]
    for shift in (0.0, 3.0, -700.0, 1e4):
        assert EP.answer_anomaly_score([v + shift for v in row]) == pytest.approx(EP.answer_anomaly_score(row), rel=1e-9)


def test_add_answer_ranking_writes_the_files_format():
    rec = EP.add_answer_ranking({"image_id": 1}, [math.log(0.3), math.log(0.1)], "Yes")
    assert rec == {"image_id": 1, "llm_answer_score": "0.75", "ranked_output": "Yes"}
