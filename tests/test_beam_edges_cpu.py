"""The reference the beam-search edge tests hold the kernels to (tests/beam_topk_ref.py), checked on the host: against
beam_ref's stable top-K where nothing ties, against hand-written answers where something does, torch's own fp32 arithmetic
inside the bound the kernel is held to, and every random case decisive -- so the GPU tests may ask for exact indices."""
import numpy as np
import pytest
import torch

from tests import beam_ref
from tests import beam_topk_ref as BR


def _torch_f32_scores(c):
    """scores + log_softmax as torch forms it in fp32, the ban after it, a NaN score mapped to -inf (the kernel's rule)."""
    s = c.scores[:, None] + torch.log_softmax(c.logits, -1)
    if 0 <= c.ban < c.V:
        s[:, c.ban] = BR.NINF
    s = torch.where(torch.isnan(s), torch.full_like(s, BR.NINF), s)
    return s.view(c.B, c.rpi * c.V)


@pytest.mark.parametrize("name", [c.name for c in BR.cases() if c.decisive and bool(torch.isfinite(c.logits).all())])
def test_topk_ref_is_the_stable_topk_of_log_softmax_where_nothing_ties(name):
    c, r = BR.case(name), BR.ref(name)
    lp = torch.log_softmax(c.logits.double(), -1)
    if 0 <= c.ban < c.V:
        lp[:, c.ban] = BR.NINF
    acc = (lp + c.scores.double()[:, None]).view(c.B, c.rpi * c.V)
    assert torch.equal(beam_ref._topk_stable(acc, c.K), r.idx)
    assert float((acc - r.s64)[r.s64 > BR.NINF].abs().max()) < 1e-12


@pytest.mark.parametrize("name", [c.name for c in BR.cases() if c.want is not None])
def test_topk_ref_gives_the_hand_written_answers(name):
    c, r = BR.case(name), BR.ref(name)
    assert np.array_equal(r.idx.numpy(), c.want), (r.idx, c.want)
    for b, k0, k1 in c.bit_equal:                                       # a tie is a tie in the reference's keys too
        s = r.s64[b][r.idx[b, k0:k1]]
        assert bool((s == s[0]).all())
    if c.exact_s is not None:                                           # the hand-derived fp32 scores lie within the bound
        sel = torch.gather(r.s64, 1, r.idx), torch.gather(r.bound, 1, r.idx)
        assert bool(((torch.from_numpy(c.exact_s).double() - sel[0]).abs() <= sel[1]).all())


def test_known_answers_spelled_out():
    """A few of the answers once more as literals, so that no helper stands between the contract and the expectation."""
    assert BR.ref("const-nb3-ban-1").idx.tolist() == [[0, 1, 2, 3, 4, 5]]
    assert BR.ref("const-nb3-ban0").idx.tolist() == [[1, 2, 3, 4, 5, 6]]
    assert BR.ref("const-nb3-ban3").idx.tolist() == [[0, 1, 2, 4, 5, 6]]
    assert BR.ref("const-nb1-ban3").idx.tolist() == [[0, 1]]
    assert BR.ref("tie-pairs-nb3").idx.tolist() == [[2 * 2500 + t for t in (0, 5, 7, 69, 133, 300)], [0, 5, 7, 69, 133, 300]]
    assert BR.ref("tie-pairs-nb8").idx[1].tolist() == [0, 5, 7, 69, 133, 300, 301, 302, 1023, 1024, 1029, 1031, 1093, 1500, 2047, 2048]
    assert BR.ref("tie-two-groups-nb3").idx[1].tolist() == [0, 1024, 2499, 5, 7, 69]
    assert BR.ref("tie-one-thread-nb3").idx[1].tolist() == [64, 1088, 2112, 3136, 4160, 5184]
    assert BR.ref("tie-every-wave-nb8").idx[1].tolist() == [3 + 64 * w for w in range(16)]
    assert BR.ref("rows-const-ulp-nb3").idx[0].tolist() == [2050, 2051, 2052, 2053, 2054, 2055]
    assert BR.ref("rows-same-equal-nb3").idx[0].tolist() == [700, 1725, 2750, 64, 1089, 2114]
    assert BR.ref("rows-same-ulp-nb3").idx[0].tolist() == [2750, 700, 1725, 2114, 64, 1089]
    assert BR.ref("rows-parked-one-nb3").idx[0].tolist() == [2050, 2051, 2052, 2053, 2054, 2055]
    r = BR.ref("few-finite-nb5")
    assert r.idx.tolist() == [[700, 1024, 3, 64, 0, 1, 2, 4, 5, 6]]
    assert torch.isinf(r.s64[0][r.idx[0, 4:]]).all() and torch.isfinite(r.s64[0][r.idx[0, :4]]).all()
    assert bool((r.bound[0][r.idx[0, 4:]] == 0).all())


@pytest.mark.parametrize("name", [c.name for c in BR.cases() if c.twin is not None])
def test_a_non_finite_row_ranks_like_a_row_whose_score_is_minus_infinity(name):
    c, r, t = BR.case(name), BR.ref(name), BR.ref(BR.case(name).twin)
    assert torch.equal(r.idx, t.idx)
    assert torch.equal(torch.gather(r.s64, 1, r.idx), torch.gather(t.s64, 1, t.idx))
    if c.kind == "nonfinite":
        assert bool(torch.isinf(r.s64.view(c.B, c.rpi, c.V)[:, 1]).all())           # row 1 of every item is all -inf
        assert not bool(torch.isnan(r.s64).any())


@pytest.mark.parametrize("name", BR.names())
def test_torch_fp32_arithmetic_stays_within_the_bound(name):
    c, r = BR.case(name), BR.ref(name)
    BR.check_scores(_torch_f32_scores(c), r.s64, r.bound, name)


def test_check_scores_fails_what_it_should():
    c, r = BR.case("rand-nb3-B1-rpi3-V1025"), BR.ref("rand-nb3-B1-rpi3-V1025")
    good = _torch_f32_scores(c)
    k = int(r.idx[0, 0])
    for wrong in (good[0, k] + 4 * float(r.bound[0, k]) + 1e-6, float("nan"), BR.NINF):
        bad = good.clone()
        bad[0, k] = wrong
        with pytest.raises(AssertionError):
            BR.check_scores(bad, r.s64, r.bound)
    bad = good.clone()
    bad[0, 2] = -1e30                                                   # the banned token: -inf, not merely very small
    with pytest.raises(AssertionError):
        BR.check_scores(bad, r.s64, r.bound)


def test_every_random_case_is_decisive():
    """Each gap among the first K + 1 ranks exceeds twice the larger of the two bounds: the exact indices are demanded of the
    kernel with no exempt share.  A case that fails here gets another seed through beam_topk_ref.SEED_BUMP."""
    weak = {c.name: BR.decisive(BR.ref(c.name)) for c in BR.cases() if c.decisive}
    assert len(weak) >= 100
    bad = {n: v for n, v in weak.items() if not v > 1.0}
    assert not bad, bad
    print(f"least decisive case: {min(weak, key=weak.get)} at {min(weak.values()):.1f} x (2 bound); seeds SEED0 = {BR.SEED0} + name "
          f"checksum, bumps {BR.SEED_BUMP}")


def test_reorder_ref_clamps_and_ignores_foreign_parents():
    B, nb, T, C = 2, 2, 5, 3
    c = torch.arange(B * nb * T * C, dtype=torch.float32).view(B * nb, T, C)
    new, = BR.reorder_ref([c], [1, 0, 2, 2], -3, 2, B, nb)                # swap in item 0, row 3 from row 2, lo clamps to 0
    assert torch.equal(new[0, :2], c[1, :2]) and torch.equal(new[1, :2], c[0, :2]) and torch.equal(new[3, :2], c[2, :2])
    assert torch.equal(new[:, 2:], c[:, 2:]) and torch.equal(new[2], c[2])
    new, = BR.reorder_ref([c], [2, -1, 4, 0], 3, 99, B, nb)               # another item's row, negative, past the end: ignored
    assert torch.equal(new, c)
    new, = BR.reorder_ref([c], [1, 1, 3, 3], 4, 4, B, nb)                 # an empty window
    assert torch.equal(new, c)
    new, = BR.reorder_ref([c], [1, 1, 3, 3], 4, 99, B, nb)                # hi clamps to T_cap
    assert torch.equal(new[0, 4], c[1, 4]) and torch.equal(new[2, 4], c[3, 4]) and torch.equal(new[:, :4], c[:, :4])
