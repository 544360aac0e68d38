"""Token scores without a device: the bound of tests/token_scores_ref.py holds a plain f32 restatement and rejects the plausible
mistakes; the evaluation protocol's llm_anomaly_score additions; generate()'s argument refusals."""
import inspect
from types import SimpleNamespace

import numpy as np
import pytest

from myriad_amd import eval_protocol as EP
from myriad_amd import ops
from myriad_amd.decode import SlotDecoder
from myriad_amd.llama import LlamaHIP
from myriad_amd.myriad import MyriadHIP
from tests import token_scores_ref as T


def _entries(fn, row, ids):
    lse, lp = fn(row, ids)
    return np.concatenate([[lse], lp])


@pytest.mark.parametrize("V", T.GRID_V)
def test_f32_restatement_stays_inside_the_bound_on_the_kernel_tests_grid(V):
    buf, _, ids = T.make_case(V)
    for r in range(T.R):
        if not T.LIVE[r] or ids[r] < 0:
            continue
        want = [ids[r]] + [w for w in T.watch_sets(V)[2] if w >= 0]
        E = T.bound(T.row_X(buf[r, :V]), V)
        got, ref = _entries(T.restate_f32, buf[r, :V], want), _entries(T.ref64, buf[r, :V], want)
        fin = np.isfinite(ref)
        print(f"V={V} row {r}: E {E:.3e}, restatement max err {np.abs(got[fin] - ref[fin]).max():.3e}")
        assert T.within(got, ref, E)
    assert T.bound(80.0, 32000) < 4e-5 and T.bound(12.0, 1000) < 1e-5          # the bound is tight enough to tell a token apart


def test_plausible_mistakes_land_outside_the_bound():
    V = 1000
    buf, _, ids = T.make_case(V)
    want = [int(ids[0]), 0, V - 1]
    row, E = buf[0, :V], T.bound(T.row_X(buf[0, :V]), V)
    ref = _entries(T.ref64, row, want)
    assert T.within(_entries(T.restate_f32, row, want), ref, E)
    # the EOS ban applied to the normaliser: the banned token's mass leaves lse.  The pick (the arg-max) as EOS: the first step's case
    assert not T.within(_entries(lambda x, i: T.mistake_ban_in_normaliser(x, i, int(ids[0])), row, want), ref, E)
    # ... and at the tenth most likely token of the row, whose mass is still far above E
    eos = int(np.argsort(row)[-10])
    p_eos = float(np.exp(T.ref64(row, [eos])[1][0]))
    assert p_eos > 10 * E
    assert not T.within(_entries(lambda x, i: T.mistake_ban_in_normaliser(x, i, eos), row, want), ref, E)
    for inv_temp in (1.0 / 3.0, 1.0 / 0.7):
        assert not T.within(_entries(lambda x, i: T.mistake_temperature(x, i, inv_temp), row, want), ref, E)
    # NaN border columns read: NaN is never within a bound
    assert not T.within(_entries(lambda x, i: T.mistake_border(buf[0], V, i), row, want), ref, E)
    # the neighbouring row's normaliser
    rows = [buf[r, :V] for r in range(T.R)]
    assert not T.within(_entries(lambda x, i: T.mistake_neighbour_lse(rows, 0, i), row, want), ref, E)
    # the maximum not subtracted at X = 80: a row whose mass sits near its maximum overflows f32 (V e^80 > 3.4e38 from V = 6200 up)
    V = 32000
    hot = (np.float32(80.0) - np.random.default_rng(3).random(V).astype(np.float32)).astype(np.float32)
    hot[0] = 80.0
    want, E = [0, V - 1], T.bound(80.0, V)
    ref = _entries(T.ref64, hot, want)
    assert T.within(_entries(T.restate_f32, hot, want), ref, E)
    assert not T.within(_entries(T.mistake_no_max, hot, want), ref, E)
    # and on the grid's own X = 80 row (a few entries near 80: no overflow) it still loses the small terms' bits
    buf, _, ids = T.make_case(V)
    row = buf[T.X80_ROW, :V]
    got, ref = _entries(T.mistake_no_max, row, [0]), _entries(T.ref64, row, [0])
    print("no-max on the grid's X = 80 row: err", float(np.abs(got - ref).max()), "E", T.bound(80.0, V))


def test_auroc_by_score_key_on_hand_made_records():
    recs = []
    for i, (anom, expert, llm) in enumerate([(1, 0.2, 0.9), (1, 0.3, 0.8), (0, 0.6, 0.1), (0, 0.7, 0.3), (1, 0.9, 0.7), (0, 0.1, 0.2)]):
        r = EP.make_ad_record(i, f"a/b/scene{i % 2}/x/{i}.png", bool(anom), "Yes, broken" if anom else "No, fine", expert * 255.0, llm)
        r["scene"] = "s"
        recs.append(r)
    acc, auc, th = EP.scene_performance(recs)
    acc2, auc_llm, th_llm = EP.scene_performance(recs, score_key="llm_anomaly_score")
    assert acc == acc2 == 1.0
    assert auc == EP.auroc([1, 1, 0, 0, 1, 0], [0.2, 0.3, 0.6, 0.7, 0.9, 0.1]) and auc < 0.6
    assert auc_llm == 1.0 and th_llm == 1.0 and th < 1.0                       # the llm column separates the classes, the expert's not
    assert EP.scene_performance(recs, None, None) == (acc, auc, th)
    assert "score_key" in inspect.signature(EP.scene_performance).parameters


def test_record_keys_with_and_without_llm_score():
    base = EP.make_ad_record(3, "a/b/c/d/e/f.png", True, "Yes", 128.0)
    assert set(base) == {"image_id", "image_path", "is_anomaly", "error", "output", "anomaly_score"}        # today's key set
    with_llm = EP.make_ad_record(3, "a/b/c/d/e/f.png", True, "Yes", 128.0, llm_score=0.123456)
    assert set(with_llm) == set(base) | {"llm_anomaly_score"} and with_llm["llm_anomaly_score"] == "0.1235"
    assert {k: with_llm[k] for k in base} == base
    assert EP.make_ad_record(3, "a/b/c/d/e/f.png", True, "Yes", 128.0, llm_score=None) == base
    # p_yes / (p_yes + p_no) from the two log-probs, the ends included
    assert EP.llm_anomaly_score([np.log(0.3), np.log(0.1)]) == pytest.approx(0.75, abs=1e-12)
    assert EP.llm_anomaly_score([-np.inf, -1.0]) == 0.0 and EP.llm_anomaly_score([-1.0, -np.inf]) == 1.0
    assert EP.llm_anomaly_score([-np.inf, -np.inf]) == 0.5 and EP.llm_anomaly_score([-2000.0, -1.0]) == 0.0


def test_generate_argument_refusals_without_a_device():
    stub = SimpleNamespace(pad_id=2, llama=SimpleNamespace(device_sampling=False, V=100))
    args = lambda **kw: MyriadHIP._generate_args(stub, kw)                      # noqa: E731
    a = args(max_new_tokens=4)
    assert a["output_scores"] is False and a["watch_ids"] == ()
    a = args(max_new_tokens=4, output_scores=True, watch_ids=[3, np.int64(99)])
    assert a["output_scores"] is True and a["watch_ids"] == (3, 99)
    assert args(output_scores=True)["watch_ids"] == ()
    for bad in ([0] * 9, [100], [-1], [1.5], ["7"], [True]):
        with pytest.raises(ValueError, match="watch_ids"):
            args(output_scores=True, watch_ids=bad)
    with pytest.raises(ValueError, match="watch_ids"):
        args(watch_ids=[3])                                                     # ids without the flag: nothing would return them
    with pytest.raises(NotImplementedError, match="output_scores"):
        args(output_scores=True, num_beams=2)
    assert args(num_beams=2)["num_beams"] == 2                                  # beams alone are what they were
    with pytest.raises(TypeError):
        args(output_logits=True)
    # the decode loops' own check and the table the kernel reads
    assert ops.SCORE_WATCH_MAX == 8 and ops.SCORE_ROWS == 10
    assert ops.score_watch_table([5, 7], 10).tolist() == [5, 7, -1, -1, -1, -1, -1, -1]
    for bad in (range(9), [10], [2.0]):
        with pytest.raises(ValueError):
            ops.score_watch_ids(bad, 10)
    for fn in (LlamaHIP.greedy_generate, SlotDecoder.run):
        p = inspect.signature(fn).parameters
        assert p["return_scores"].default is False and p["watch_ids"].default == ()


def test_a_scores_view_has_a_key_of_its_own_and_every_other_key_is_unchanged():
    key = SlotDecoder._view_key
    for args in ((1.0, None), (0.5, (False, True)), (0.5, (True, False))):
        for split in (False, True):
            assert key(*args, split) == key(*args, split, False)
            assert key(*args, split, True) != key(*args, split, False)
        assert key(*args, True, True) == ("split", ("scores", key(*args)))
    assert key(1.0) == 1.0 and key(1.0, None, False, True) == ("scores", 1.0)
