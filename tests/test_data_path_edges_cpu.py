"""The data-path edge cases, CPU side (no GPU needed): the helpers of tests/data_path_ref.py are themselves held to the
references the project trusts, and the cases the GPU module runs are shown to discriminate.

  * `label_ref` == `apply_numpy`'s label, bit for bit, on every golden case.
  * The constructed windows hold what they claim: exactly 40 / 41 non-zeros in the disk, exactly 12 / 13 votes.
  * A numpy emulation of the label kernels meets every section-3 case; each named mutant (H and W swapped, a clamp to H - 2,
    majority > 13, threshold >=, median position 39 / 41, nz > 41, the masked sum for the intensity, the unmasked sum for the
    vote) fails at least one.  The same for the blend's index arithmetic and the front-end's crop offset.
  * The Poisson cases: the pre-truncation solution by scipy's DST and by the dense sine products agree to 1e-10, no unclipped
    pixel is within 1e-9 of the truncation's discontinuity, and both truncate to the same bytes -- so bit equality may be
    demanded of the device on every pixel."""
import importlib.util
import os

import numpy as np
import pytest

from myriad_amd import self_sup as P
from tests import data_path_ref as R

_spec = importlib.util.spec_from_file_location("mk_selfsup_edges", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools",
                                                                               "make_golden_selfsup.py"))
MK = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MK)

_MODES = {"binary": 0, "continuous": 1, "intensity": 2, "logistic-intensity": 3}


@pytest.mark.parametrize("name,seed,kw", MK.CASES, ids=[c[0] for c in MK.CASES])
def test_label_ref_is_apply_numpys_label(name, seed, kw):
    dest, src = MK.test_image(10 + seed), MK.test_image(40 + seed)
    np.random.seed(1000 + seed)
    ops, factor = P.plan(dest, src, **{k: v for k, v in kw.items() if k != "intensity_logistic_params"})
    s = dest if kw.get("same") else src
    ilp = kw.get("intensity_logistic_params", (1 / 6, 20))
    union = R.union_ref(dest.shape[:2], ops)
    for label_mode, mode in _MODES.items():                     # the case's own mode and the other three
        for tol in ((1, 0) if label_mode == kw.get("label_mode", "binary") else (1,)):
            out, label, _ = P.apply_numpy(dest, s, ops, factor, label_mode, tol, ilp)
            got = R.label_ref(dest, out, union, mode, tol, factor, ilp[0], ilp[1])
            want = np.asarray(label, np.float64)[..., 0]
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, label_mode, tol)


def test_constructed_windows_hold_the_stated_counts():
    cases = {c[0]: c for c in R.label_cases()}
    seen = set()
    for name, b, (cy, cx), kind, count, tol in R.CONSTRUCTED:
        _, dest, out, union = cases[name]
        H, W = union.shape[1:]
        if kind == "median":
            assert R.disk_nonzeros(dest[b], out[b], union[b], tol, cy, cx) == count, (name, b)
        else:
            assert R.vote_count(dest[b], out[b], union[b], tol, cy, cx) == count, (name, b)
            lm = R.label_ref(dest[b], out[b], union[b], 0, tol, 1.0, 0, 0)
            assert lm[cy, cx] == (1.0 if count >= 13 else 0.0)
        seen.add((kind, count, "corner" if (cy, cx) in ((0, 0), (H - 1, W - 1)) else "interior", H > W))
    assert len(seen) == 16                                      # 2 kinds x 2 counts x {interior, corner} x 2 orientations
    # the threshold blocks: sums of exactly 3 tol stay out, 3 tol + 1 go in, for tol = 0, 1, 85
    for tag in ("37x53", "53x37"):
        _, dest, out, union = cases["thresholds_" + tag]
        s = R.channel_sums(dest[0], out[0])
        assert set(np.unique(s).tolist()) == {0, 1, 3, 4, 255, 256}
        for tol in R.LABEL_TOLS:
            lm = R.label_ref(dest[0], out[0], union[0], 0, tol, 1.0, 0, 0)
            assert lm[s == 3 * tol].sum() == 0 and lm[s == 3 * tol + 1].sum() >= 9
    # the dense cases run the selection (> 40 non-zeros), the sparse ones the shortcut, with ties present
    _, dest, out, union = cases["dense_ties_2x37x53"]
    assert R.disk_nonzeros(dest[0], out[0], union[0], 0, 18, 26) > 40 and len(np.unique(R.channel_sums(dest[0], out[0]))) <= 7
    _, dest, out, union = cases["sparse_2x37x53"]
    lm = R.label_ref(dest[0], out[0], union[0], 0, 1, 1.0, 0, 0)
    assert 0 < lm.sum() < lm.size // 2
    # union_holes: holes inside the blurred mask where out != dest, and a changed region the union leaves out
    _, dest, out, union = cases["union_holes_2x37x53"]
    lm = R.label_ref(dest[0], out[0], union[0], 0, 1, 1.0, 0, 0)
    s = R.channel_sums(dest[0], out[0])
    assert ((union[0] == 0) & (lm == 1) & (s > 0)).sum() > 20 and ((union[0] == 0) & (lm == 0) & (s > 3)).sum() > 100


@pytest.mark.parametrize("case", R.label_cases(), ids=[c[0] for c in R.label_cases()])
def test_label_emulation_meets_every_case(case):
    assert R.label_case_passes(case)


@pytest.mark.parametrize("mutant", R.LABEL_MUTANTS)
def test_label_mutant_fails_a_case(mutant):
    failed = [c[0] for c in R.label_cases() if not R.label_case_passes(c, mutant)]
    assert failed, mutant
    if mutant == "hw_swap":                                     # invisible on square crops, caught by both orientations
        assert any("37x53" in n for n in failed) and any("53x37" in n for n in failed)
    if mutant in ("median_pos39", "median_pos41", "nz_gt41"):
        assert any(n.startswith("median_windows") for n in failed), failed
    if mutant == "majority_gt13":
        assert any(n.startswith("vote_windows") for n in failed), failed
    if mutant == "threshold_ge":
        assert any(n.startswith("thresholds") for n in failed), failed
    if mutant in ("value_masked", "vote_unmasked"):
        assert any(n.startswith("union_holes") for n in failed), failed


def test_label_mutants_are_invisible_where_the_old_suite_looked():
    """What the golden cases could not see: on a square crop the H / W swap computes the same label."""
    r = np.random.RandomState(0)
    dest = r.randint(0, 256, (1, 24, 24, 3)).astype(np.uint8)
    out = r.randint(0, 256, (1, 24, 24, 3)).astype(np.uint8)
    union = np.ones((1, 24, 24), np.uint8)
    for mode in (0, 2):
        assert np.array_equal(R.emu_label(dest, out, union, mode, 1, [1.0], 0, 0), R.emu_label(dest, out, union, mode, 1, [1.0], 0, 0, "hw_swap"))


# ------------------------------------------------------------------------------------------------ blend
@pytest.mark.parametrize("sc", R.blend_scenarios(), ids=[s[0] for s in R.blend_scenarios()])
def test_blend_emulation_is_apply_numpy_and_the_swap_mutant_is_not(sc):
    name, dest, src, plans = sc
    want, wu = R.blend_ref(dest, src, plans)
    got, gu = R.emu_blend(dest, src, plans)
    assert np.array_equal(got, want) and np.array_equal(gu, wu)
    assert np.array_equal(want[1], dest[1]) and not wu[1].any()               # no operation on image 1
    mg, mu = R.emu_blend(dest, src, plans, "hw_swap")
    assert not np.array_equal(mg, want) or not np.array_equal(mu, wu)
    assert not np.array_equal(want[0], dest[0]) or name == "factors_0_1"      # the scenario changes pixels


def test_blend_scenarios_reach_what_they_claim():
    sc = {s[0]: s for s in R.blend_scenarios()}
    exact, under = R.integer_pairs(0.3)
    assert len(exact) > 100 and len(under) >= 10              # 6206 and 34 of the 65536 byte pairs
    x, s = under[0]
    v = float(x)
    v -= 0.3 * 1 * x
    v += 0.3 * 1 * s
    assert (7 * int(x) + 3 * int(s)) % 10 == 0 and np.floor(v) == (7 * int(x) + 3 * int(s)) // 10 - 1
    _, d2, s2, _ = sc["integer_landing"]
    pairs = set(map(tuple, np.stack([d2[0].reshape(-1), s2[0].reshape(-1)], 1).tolist()))
    assert pairs & set(map(tuple, exact.tolist())) and pairs & set(map(tuple, under.tolist()))
    # overlap: the second operation sees the first's pixels -- applying them in the other order gives another image
    _, dest, src, plans = sc["overlap"]
    for b in (0, 2):
        ops, f = plans[b]
        a, _, _ = P.apply_numpy(dest[b], src[b], ops, f)
        rev, _, _ = P.apply_numpy(dest[b], src[b], ops[::-1], f)
        assert not np.array_equal(a, rev)
    # factor 0 changes nothing, factor 1 pastes the source
    _, dest, src, plans = sc["factors_0_1"]
    want, _ = R.blend_ref(dest, src, plans)
    assert np.array_equal(want[0], dest[0]) and not np.array_equal(want[2], dest[2])
    assert any(op.resized for op in sc["pooled"][3][0][0]) and any(not op.resized for op in sc["pooled"][3][0][0])


# ------------------------------------------------------------------------------------------------ front-end crop offset
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_front_end_emulation_meets_the_sizes(mode):
    for (H, W) in R.FRONT_SIZES:
        img = R.noise_image(H, W)
        assert np.array_equal(R.emu_front_end(img, R.FRONT_SIZE, mode), R.front_ref(img, R.FRONT_SIZE, mode)[0]), (H, W)


@pytest.mark.parametrize("rounding,caught", [("floor", (35, 16)), ("ceil", (17, 16)), ("ceil", (16, 17)), ("ceil", (33, 16))])
def test_front_end_crop_offset_mutant_fails(rounding, caught):
    assert caught in R.FRONT_SIZES
    img = R.noise_image(*caught)
    assert not np.array_equal(R.emu_front_end(img, R.FRONT_SIZE, "train", rounding), R.front_ref(img, R.FRONT_SIZE, "train")[0])


# ------------------------------------------------------------------------------------------------ Poisson
@pytest.mark.parametrize("case", R.poisson_cases(), ids=[c[0] for c in R.poisson_cases()])
def test_poisson_truncation_cannot_hide_a_difference(case):
    """(a) dense and FFT solutions agree to 1e-10; (b) no unclipped pixel has u + 1e-6 within 1e-9 of an integer; (c) their
    truncations are equal -- and equal poisson_clone_numpy's bytes, which holds the restated lines to the reference."""
    name, dest, image, steps = case
    out = dest.copy()
    worst, nearest = 0.0, 1.0
    for patch, pms, roi, mixed in steps:
        u_fft, u_dense = R.poisson_u(out[image], patch, pms, roi, mixed)
        worst = max(worst, float(np.abs(u_fft - u_dense).max()))
        assert np.abs(u_fft - u_dense).max() <= 1e-10, name                                             # (a)
        for u in (u_fft, u_dense):
            free = (u > 0.0) & (u < 255.0)
            t = u[free] + P.TRUNC_EPS
            dist = np.abs(t - np.rint(t))
            nearest = min(nearest, float(dist.min()) if dist.size else 1.0)
            assert not (dist <= 1e-9).any(), name                                                       # (b)
        assert np.array_equal(R.truncate(u_fft), R.truncate(u_dense)), name                             # (c)
        y0s, x0s, dy0, dx0, h, w = roi
        before = out.copy()
        P.poisson_clone_numpy(out[image], patch, pms, roi, mixed=mixed)
        assert np.array_equal(out[image, dy0 + 1:dy0 + h - 1, dx0 + 1:dx0 + w - 1], R.truncate(u_fft)), name
        before[image, dy0 + 1:dy0 + h - 1, dx0 + 1:dx0 + w - 1] = out[image, dy0 + 1:dy0 + h - 1, dx0 + 1:dx0 + w - 1]
        assert np.array_equal(before, out)                      # nothing outside the ROI's interior moves
    assert np.array_equal(out, R.poisson_apply_ref(dest, image, steps))
    print(f"{name}: dense vs FFT {worst:.2e}, nearest integer {nearest:.2e}")
