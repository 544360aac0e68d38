"""CPU checks of the beam-sampling rule: tests/beam_sample_ref.py's processed scores against transformers' own logits processors
on the log-probs, the decode loop's host rule (decode_host.beam_sample_select) against the reference on the shared grid, the
Gumbel top-K draw against the exact Plackett-Luce probabilities, and the condition the GPU test relies on: few grid items hold a
row whose top-p cut is too close to call."""
import numpy as np
import pytest
import torch

from myriad_amd.decode_host import beam_sample_select
from tests import beam_sample_ref as BR

NAMES = [c.name for c in BR.CASES]


def _tol(ref):
    return BR.TOL * np.maximum(1.0, np.abs(np.asarray(ref, dtype=np.float64)))


@pytest.mark.parametrize("name", [c.name for c in BR.CASES if not c.first])
def test_processed_scores_match_transformers_processors(name):
    lp_mod = pytest.importorskip("transformers.generation.logits_process")
    c = next(c for c in BR.CASES if c.name == name)
    inp = c.inputs()
    R, V = inp["logits"].shape
    lp = torch.log_softmax(inp["logits"].float(), -1)
    longest = max(1, max(len(s) for s in inp["seen"]))
    # the generated ids as HF's input_ids; a shorter row repeats one of its own ids (each id is penalised once)
    ids = torch.tensor([(list(s) + [s[0]] * (longest - len(s))) if s else [0] * longest for s in inp["seen"]], dtype=torch.long)
    want = lp.clone()
    rows_with_ids = [r for r, s in enumerate(inp["seen"]) if s]
    if c.penalty != 1.0 and rows_with_ids:
        rp = lp_mod.RepetitionPenaltyLogitsProcessor(c.penalty)
        want[rows_with_ids] = rp(ids[rows_with_ids], lp[rows_with_ids].clone())
    if c.ban >= 0:                                          # MinLength: input_ids shorter than min_length bans EOS
        want = lp_mod.MinLengthLogitsProcessor(longest + 1, c.ban)(ids, want)
    want = want * torch.tensor(np.float32(c.inv_temp))      # TemperatureLogitsWarper divides by T: the kernel multiplies by fp32(1 / T)
    want = lp_mod.TopKLogitsWarper(max(c.top_k, 1), min_tokens_to_keep=2)(ids, want)
    if c.top_p < 1.0:
        want = lp_mod.TopPLogitsWarper(c.top_p, min_tokens_to_keep=2)(ids, want)
    checked = 0
    for r in range(R):
        got, near = BR.processed(inp["logits"][r], inp["seen"][r], c.penalty, c.ban, c.inv_temp, c.top_k, c.top_p)
        if near:
            continue
        checked += 1
        assert torch.equal(torch.isinf(got), torch.isinf(want[r])), (name, r)
        fin = torch.isfinite(got)
        assert float((got[fin] - want[r][fin]).abs().max()) <= 1e-6, (name, r)
    assert checked >= R - 1


def test_temperature_as_a_multiplication_stays_within_the_tolerance():
    """HF divides by T, the kernel multiplies by fp32(1 / T): one rounding apart, far inside the kernel's tolerance."""
    lp = torch.log_softmax(torch.randn(4096, generator=torch.Generator().manual_seed(3)) * 3.0, -1)
    for T in (0.7, 3.0):
        a, b = lp / T, lp * torch.tensor(np.float32(1.0 / T))
        assert float(((a - b).abs() / a.abs().clamp_min(1.0)).max()) <= 3e-7


@pytest.mark.parametrize("name", NAMES)
def test_host_select_equals_the_reference(name):
    c = next(c for c in BR.CASES if c.name == name)
    inp, ref = c.inputs(), c.ref()
    for b, it in enumerate(ref):
        if it.near:
            continue
        lo = b * c.nb
        acc, flat, key = beam_sample_select(inp["logits"][lo:lo + c.nb].numpy(), inp["scores"][lo:lo + c.nb].numpy(),
                                            inp["seen"][lo:lo + c.nb], c.ban, c.inv_temp, c.top_k, c.top_p, c.penalty, inp["seed"],
                                            0 if c.first else c.t, b)
        assert flat.tolist() == it.sel_flat, (name, b)
        assert np.all(np.abs(acc - np.array(it.sel_acc)) <= _tol(it.sel_acc)), (name, b)
        assert np.all(np.abs(key - np.array(it.sel_key)) <= _tol(it.sel_key)), (name, b)


def test_host_select_without_the_draw_is_penalised_beam_search():
    c = next(c for c in BR.CASES if c.penalty != 1.0 and c.V == 4100)
    inp = c.inputs()
    ref = BR.step(inp["logits"], inp["scores"], inp["seen"], c.B, c.nb, c.ban, 1.0, 50, 1.0, c.penalty, 0, 0, draw=False)
    for b, it in enumerate(ref):
        lo = b * c.nb
        acc, flat, key = beam_sample_select(inp["logits"][lo:lo + c.nb].numpy(), inp["scores"][lo:lo + c.nb].numpy(),
                                            inp["seen"][lo:lo + c.nb], c.ban, 1.0, 50, 1.0, c.penalty, 0, 0, b, draw=False)
        assert flat.tolist() == it.sel_flat and np.array_equal(acc, key)
        assert np.all(np.abs(acc - np.array(it.sel_acc)) <= _tol(it.sel_acc))


def test_first_step_pins_the_parked_beams_to_the_lower_flat_index():
    """t = 0: the -1e9 rows' keys collapse to one fp32 value, so what they contribute comes in ascending flat order."""
    c = next(c for c in BR.CASES if c.name == "first_V36_nb8_k1")
    for it in c.ref():
        parked = [(f, k) for f, k in zip(it.sel_flat, it.sel_key) if f >= c.V]
        assert len(parked) == 2 * c.nb - 2                  # top_k = 1 keeps two candidates a row: 14 of the 16 come from parked rows
        assert all(k == np.float32(-1.0e9) for _, k in parked)
        assert [f for f, _ in parked] == sorted(f for f, _ in parked)


def test_gumbel_top_k_is_plackett_luce():
    """N = 4096 draws of the reference (8 steps of 512 items): first-draw and ordered first-pair counts against the exact values."""
    d = BR.DIST
    x = BR.dist_logits().repeat(d["items"], 1)
    sc = torch.tensor(d["scores"]).repeat(d["items"])
    firsts, pairs = [], []
    for t in range(d["steps"]):
        for it in BR.step(x, sc, [[]] * (2 * d["items"]), d["items"], d["nb"], -1, 1.0, 50, 1.0, 1.0, d["seed"], t):
            firsts.append(it.sel_flat[0])
            pairs.append((it.sel_flat[0], it.sel_flat[1]))
    worst = BR.check_counts(firsts, pairs)
    print(f"worst z: first draws {worst['first'][0]:.2f} over {worst['first'][1]} outcomes, "
          f"pairs {worst['pair'][0]:.2f} over {worst['pair'][1]}")
    assert worst["first"][1] >= 8 and worst["pair"][1] >= 30


def test_few_grid_items_are_near_a_top_p_cut():
    """A condition of the grid, from the reference alone: the GPU test skips near items, so they must be rare (<= 2 %)."""
    items = [it for c in BR.CASES for it in c.ref()]
    near = sum(it.near for it in items)
    print(f"{near} of {len(items)} grid items hold a near row")
    assert len(items) >= 50 and near <= 0.02 * len(items)
