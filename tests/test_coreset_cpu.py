"""CPU checks of the coreset reference (tests/coreset_ref.py): the known answer of the rule, that the replay checker accepts a
correct fp32 selector and rejects each plausible kernel mistake -- an fp32 emulation of csrc/coreset.hip with the mistake built in
-- and the device-free host logic (BankIndex.resize, the keep -> rows rule)."""
import math

import pytest
import torch

from myriad_amd.expert_bank import BankIndex, keep_rows
from tests import coreset_ref as cr

BF16 = torch.bfloat16


def emulated_select(taps, n, start=0, *, rows=None, agg="min", drop_tap=False, tie="low", mark=True):
    """csrc/coreset.hip in fp32 on the host (dist2 = the fp64 sum rounded to fp32: inside the bound), with switches for the
    mistakes: `agg` "max", `drop_tap` (the last tap is left out), `tie` "high", `mark` False (a chosen row keeps its 0), and
    `rows` larger than the class (the loop runs over the neighbour's rows too)."""
    x = cr.as64(taps[:-1] if drop_tap and len(taps) > 1 else taps)
    rows = x[0].shape[0] if rows is None else rows
    x = [t[:rows] for t in x]
    mind = torch.full((rows,), math.inf, dtype=torch.float32)
    sel, radius2 = [start], [math.inf]
    for j in range(n):
        d = cr.dist2_to(x, sel[j]).float()
        mind = torch.minimum(mind, d) if agg == "min" or j == 0 else torch.maximum(mind, d)
        if mark:
            mind[sel[j]] = -1.0
        if j + 1 < n:
            top = mind.max()
            hits = (mind == top).nonzero()
            sel.append(int(hits[0] if tie == "low" else hits[-1]))
            radius2.append(float(top))
    return sel, torch.tensor(radius2), mind, float(mind.max())


def test_known_answer():
    taps = [torch.tensor(cr.KNOWN_ROWS, dtype=torch.float32).to(BF16)]
    ref = cr.select_ref(taps, 6, start=0, checkpoints=(2, 6))
    assert ref["sel"] == cr.KNOWN_SEL == [0, 2, 4, 1, 3, 5]
    assert ref["radius2"].tolist() == cr.KNOWN_RADIUS2 == [math.inf, 5.0, 5.0, 0.0, 0.0, 0.0]
    assert ref["cover2"] == -1.0 and ref["mind"].tolist() == [-1.0] * 6
    assert ref["at"][2][0].tolist() == [-1.0, 0.0, -1.0, 0.0, 5.0, 0.0] and ref["at"][2][1] == 5.0
    assert ref["at"][6][1] == -1.0
    short = cr.select_ref(taps, 3, start=0)                                   # nesting: a prefix, and the cover of what is left
    assert short["sel"] == cr.KNOWN_SEL[:3] and short["cover2"] == 0.0
    cr.replay_check(taps, ref["sel"], ref["radius2"], start=0, mind=ref["mind"], cover2=ref["cover2"], exact=True)
    other = cr.select_ref(taps, 6, start=5)
    assert other["sel"] == [5, 2, 4, 0, 1, 3]


def random_case():
    """40 unit rows in two taps and copies of the first eight behind them: 48 rows, eight exact ties."""
    taps = cr.unit_case(40, 32, 2, seed=11)
    return [torch.cat([t, t[:8]]) for t in taps]


def test_gamma_is_the_documented_expression():
    k = (96 * 2 + 3) * 2.0 ** -24
    assert cr.gamma(96, 2) == k / (1 - k)


def test_checker_accepts_the_correct_selector():
    taps = random_case()
    for n, start in ((48, 0), (48, 47), (17, 5), (1, 0)):
        sel, r2, mind, cover2 = emulated_select(taps, n, start)
        worst = cr.replay_check(taps, sel, r2, start=start, mind=mind, cover2=cover2, what=f"n={n}")
        assert worst <= 1.0
        assert sorted(sel) == sorted(set(sel)) and (n < 48 or sorted(sel) == list(range(48)))
    ints = cr.int_case(30, 8, 2, seed=3)
    sel, r2, mind, cover2 = emulated_select(ints, 30)
    cr.replay_check(ints, sel, r2, start=0, mind=mind, cover2=cover2, exact=True)
    ref = cr.select_ref(ints, 30)
    assert sel == ref["sel"] and torch.equal(r2.double(), ref["radius2"]) and cover2 == ref["cover2"] == -1.0


@pytest.mark.parametrize("mistake", [dict(agg="max"), dict(drop_tap=True), dict(mark=False)])
def test_checker_rejects_a_wrong_selector(mistake):
    taps = random_case()
    sel, r2, mind, cover2 = emulated_select(taps, 48, 0, **mistake)
    with pytest.raises(AssertionError):
        cr.replay_check(taps, sel, r2, start=0, mind=mind, cover2=cover2, what=str(mistake))


def test_checker_rejects_ties_broken_to_the_highest_index():
    ints = cr.int_case(30, 8, 2, seed=3)
    sel, r2, mind, cover2 = emulated_select(ints, 30, tie="high")
    with pytest.raises(AssertionError, match="lower"):
        cr.replay_check(ints, sel, r2, start=0, what="tie high")              # the identical-row rule alone
    with pytest.raises(AssertionError):
        cr.replay_check(ints, sel, r2, start=0, exact=True, what="tie high, exact")


def test_checker_rejects_a_selector_that_reads_past_the_class():
    taps = random_case()
    far = [-t.double().mean(dim=0, keepdim=True) for t in taps]               # the neighbour's first row: far from every row
    bank = [torch.cat([t, (f / f.norm()).to(BF16)]) for t, f in zip(taps, far)]
    sel, r2, mind, cover2 = emulated_select(bank, 10, 0, rows=49)
    assert 48 in sel
    with pytest.raises(AssertionError, match="outside"):
        cr.replay_check(taps, sel, r2, start=0, what="one row past the class")


def test_checker_rejects_a_wrong_mind_and_cover():
    taps = random_case()
    sel, r2, mind, cover2 = emulated_select(taps, 12, 0)
    bad = mind.clone()
    free = int((mind > 0).nonzero()[0])
    bad[free] *= 1.001
    with pytest.raises(AssertionError):
        cr.replay_check(taps, sel, r2, mind=bad, cover2=float(bad.max()))
    with pytest.raises(AssertionError):
        cr.replay_check(taps, sel, r2, mind=mind, cover2=cover2 * 1.001)
    bad = mind.clone()
    bad[sel[3]] = 0.0
    with pytest.raises(AssertionError, match="-1"):
        cr.replay_check(taps, sel, r2, mind=bad)


def test_coverage_case_on_the_fp64_rule():
    """Six clusters of 900 / 40 / 30 / 20 / 7 / 3 rows, the big one first: six centres are one row of every cluster (the first
    six ROWS are all cluster 0), the radii are distances between clusters (about 4 = 2 per tap between unrelated unit rows) and
    the cover is a distance inside a cluster."""
    taps, label = cr.sized_clusters(cr.COVER_SIZES, 96, 2, seed=5)
    ref = cr.select_ref(taps, 6)
    assert sorted(int(label[s]) for s in ref["sel"]) == [0, 1, 2, 3, 4, 5] and set(label[:6].tolist()) == {0}
    assert ref["sel"] == cr.COVER_SEL
    r2 = ref["radius2"][1:]
    print("coverage case: radius2", [float(v) for v in r2], "cover2", ref["cover2"])
    # the recorded fp64 values (4.2209, 3.9995, 3.9239, 3.7654, 3.7438 and 0.19204); 1e-9 is room for the order of a host sum
    assert bool((r2 - torch.tensor(cr.COVER_RADIUS2, dtype=torch.float64)).abs().max() <= 1e-9)
    assert abs(ref["cover2"] - cr.COVER_COVER2) <= 1e-9
    assert bool((r2[:-1] >= r2[1:]).all())


# ------------------------------------------------------------------------------------------------------------ host logic
def test_bank_index_resize():
    ix = BankIndex()
    for name, rows in (("a", 512), ("b", 300), ("c", 7)):
        ix.append(name, rows)
    assert ix.resize("b", 30) == (512, 300)
    assert ix.names() == ["a", "b", "c"] and ix.total == 549
    assert [ix.lookup(n) for n in "abc"] == [(0, 512), (512, 30), (542, 7)]
    assert ix.resize("b", 30) == (512, 30)                                    # keeping everything is allowed
    for bad in (0, 31, -1):
        with pytest.raises(ValueError, match="'b'"):
            ix.resize("b", bad)
    with pytest.raises(KeyError, match="zipper"):
        ix.resize("zipper", 1)
    assert ix.remove("b") == (512, 30) and ix.lookup("c") == (512, 7)


def test_keep_to_rows_rule():
    assert keep_rows(1, 512) == 1 and keep_rows(512, 512) == 512 and keep_rows(37, 512) == 37
    assert keep_rows(1.0, 512) == 512 and keep_rows(0.25, 512) == 128 and keep_rows(0.1, 512) == 52
    assert keep_rows(0.01, 51200) == 512 and keep_rows(1e-9, 512) == 1 and keep_rows(0.5, 1) == 1
    assert keep_rows(0.1, 51201) == 5121                                      # the ceiling
    for bad in (0, 513, -3, 0.0, 1.5, -0.1, True, "all", None, float("nan")):
        with pytest.raises(ValueError):
            keep_rows(bad, 512)
