"""No GPU: the rows of tests/sampling_edge_cases.py discriminate.  HF's warper chain, restated apart from tests/sampling_ref.py,
keeps the set sample_row keeps; six mis-statements of the rule (what a kernel could plausibly compute instead) each disagree with
sample_row on a row the GPU file compares; the NaN / +inf rules of the reference have the contract's answers."""
import numpy as np
import pytest
import torch

from tests import sampling_edge_cases as C
from tests import sampling_ref as S

TIE_COUNTS = (1059, 8, 181)                 # compared, near, overflow rows of the tie grid (test_sampling_edges_gpu.py asserts the same)


def _hf_kept(x, top_k, top_p, inv_temp, ban):
    """transformers' TemperatureLogitsWarper -> TopKLogitsWarper (`scores < kth` go) -> TopPLogitsWarper (ascending sort, `cum <=
    1 - top_p` go, the last stays) on one finite row, as myriad_amd.decode_host._host_draw runs them; the masses in float64.  HF
    leaves the order inside a tie to torch.sort; the contract's (logit desc, id asc) is the flipped row sorted stably ascending."""
    y = x.clone().float()
    if ban >= 0:
        y[ban] = C.NINF
    y = y * torch.tensor(np.float32(inv_temp))
    V = y.numel()
    kth = torch.topk(y, min(max(top_k, 1), V)).values[-1]
    y = y.masked_fill(y < kth, C.NINF)
    if top_p < 1.0:
        srt, idx = torch.sort(y.flip(0), descending=False, stable=True)
        idx = V - 1 - idx
        remove = srt.double().softmax(-1).cumsum(-1) <= 1.0 - top_p
        remove[-1:] = False
        y[idx[remove]] = C.NINF
    return set(torch.nonzero(torch.isfinite(y)).flatten().tolist())


def _key(y):
    """The order-preserving u32 key of the radix select without the zero rule: +0 above -0."""
    b = y.numpy().view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)


def _row(x, top_k, top_p, inv_temp, ban, u, mutant=None):
    """(kept, out) by sample_row's rule written out again, with one deliberate error when `mutant` names it."""
    x = x.detach().float().clone()
    V = x.numel()
    if ban >= 0:
        x[ban] = C.NINF
    if mutant != "nan_largest":
        x[torch.isnan(x)] = C.NINF
    top = int(torch.argmax(x))
    if bool((x == C.INF).any()):
        return 1, top
    y = x * torch.tensor(np.float32(inv_temp))
    if bool((y == C.INF).any()):
        return 1, int(torch.nonzero(y == C.INF)[0])
    k = max(int(top_k), 1) if mutant == "k_unclamped" else min(max(int(top_k), 1), V)
    thr = torch.topk(y, k).values[-1]
    if mutant == "bitkey":
        key = _key(y)
        cand = torch.from_numpy(key >= _key(thr.reshape(1))[0]) & torch.isfinite(y)
    else:
        cand = (y >= thr) & torch.isfinite(y)
    ids = torch.nonzero(cand).flatten().numpy()
    if len(ids) == 0 or len(ids) > (1023 if mutant == "cap_1023" else S.CAP):
        return -1, top
    yv = y.numpy()[ids].astype(np.float64)
    if mutant == "bitkey":
        o = np.lexsort((ids, -_key(y)[ids]))
    else:
        o = np.lexsort((-ids if mutant == "id_desc" else ids, -yv))
    ids, yv = ids[o], yv[o]
    p = np.exp(yv - yv[0])
    cum = np.cumsum(p)
    excl = cum - p
    if top_p >= 1.0:
        mk = len(ids)
    elif mutant == "excl_le":
        mk = max(int(np.sum(excl <= top_p * cum[-1])), 1)
    else:
        mk = max(int(np.sum(excl < top_p * cum[-1])), 1)
    return mk, int(ids[min(int(np.sum(cum[:mk] <= u * cum[mk - 1])), mk - 1)])


def _compared_rows():
    """(launch, row, reference) of every row the GPU file holds the kernel to: all of tests 2-5, the tie grid's minus its `near`."""
    for c in C.tie_grid() + C.direct_cases():
        for r, ref in enumerate(c.ref()):
            if c.expect is None and ref["near"]:
                continue
            yield c, r, ref


def test_the_rewritten_rule_is_sample_row():
    n = 0
    for c, r, ref in _compared_rows():
        assert _row(c.x[r], c.top_k, c.top_p, c.inv_temp, c.ban, c.u(r)) == (ref["kept"], ref["out"]), (c.name, r)
        n += 1
    assert n == sum(c.R for c in C.tie_grid() + C.direct_cases()) - TIE_COUNTS[1]


@pytest.mark.parametrize("mutant", ["bitkey", "id_desc", "excl_le", "k_unclamped", "nan_largest", "cap_1023"])
def test_each_mutant_is_caught_by_a_compared_row(mutant):
    """bitkey: the threshold and the order on the bit key, +0 above -0 (the kernel before the zero rule).  id_desc: ties in
    descending id order.  excl_le: a candidate whose exclusive mass equals top_p * total stays.  k_unclamped: top_k past V not
    clamped (an error counts).  nan_largest: NaN ranked above every logit.  cap_1023: 1024 candidates already overflow."""
    caught = []
    for c, r, ref in _compared_rows():
        try:
            got = _row(c.x[r], c.top_k, c.top_p, c.inv_temp, c.ban, c.u(r), mutant)
        except (RuntimeError, IndexError):
            got = None
        if got != (ref["kept"], ref["out"]):
            caught.append(c.name)
    print(mutant, "caught on", len(caught), "rows, first", caught[:3])
    assert caught
    families = dict(bitkey="zero_", id_desc="zero_", excl_le="flat", k_unclamped="pad_k5_V3", nan_largest="nan_", cap_1023="pad_n1024")
    assert any(n.startswith(families[mutant]) for n in caught), caught[:10]


def test_the_bitkey_mutant_is_the_issues_example():
    """x = [1, 0, -0, -0, -1, 0, -2, -3], top_k 2 or 3: the rule keeps ids 0 1 2 3 5 in that order, the bit key keeps 0, 1, 5."""
    x = C.ZERO_ROWS["plus_first"]
    for top_k in (2, 3):
        assert S.sample_row(x, top_k, 1.0, 1.0)["order"].tolist() == [0, 1, 2, 3, 5]
        assert _hf_kept(x, top_k, 1.0, 1.0, -1) == {0, 1, 2, 3, 5}
        key = _key(x)
        assert set(np.nonzero(key >= np.sort(key)[::-1][top_k - 1])[0].tolist()) == {0, 1, 5}


def test_hf_chain_keeps_the_reference_set_on_the_finite_rows():
    """Tests 1 to 3: the tie grid, the sort-padding ramps and the signed zeros; overflow rows have no kept set to compare."""
    n = 0
    for c in C.tie_grid() + C.pad_cases() + C.zero_cases():
        for r, ref in enumerate(c.ref()):
            if ref["near"] or ref["kept"] == -1:
                continue
            assert bool(torch.isfinite(c.x[r]).all())
            assert _hf_kept(c.x[r], c.top_k, c.top_p, c.inv_temp, c.ban) == set(ref["order"][:ref["kept"]].tolist()), (c.name, r)
            n += 1
    assert n >= TIE_COUNTS[0]


def test_tie_grid_counts_and_direct_rows_stay_clear_of_a_boundary():
    rows, near, over = C.tie_grid_counts()
    assert (rows, near, over) == TIE_COUNTS and rows + near + over == len(C.TIE_V) * 4 * 4 * 2 * C.TIE_ROWS == 1248
    assert near <= 0.02 * (rows + near + over)
    for c in C.direct_cases():
        for r, ref in enumerate(c.ref()):
            if c.expect is None:
                assert not ref["near"], c.name
            else:                                                     # the closed-form answer is the reference's too
                assert (ref["kept"], ref["out"]) == tuple(c.expect[r]), (c.name, ref["kept"], ref["out"])


def test_nan_and_inf_rules_of_the_reference():
    seen = set()
    for c in C.nonfinite_cases():
        x, ref = c.x[0], c.ref()[0]
        seen.add(c.name.split("_V")[0])
        assert 0 <= ref["out"] < c.V
        nan_ids = set(torch.nonzero(torch.isnan(x)).flatten().tolist())
        if c.expect is None:                                          # a NaN is -inf: the row with -inf written in its place
            want = S.sample_row(c.clean[0], c.top_k, c.top_p, c.inv_temp, c.ban, u=c.u(0))
            assert (ref["kept"], ref["out"]) == (want["kept"], want["out"]) and ref["order"].tolist() == want["order"].tolist()
            assert ref["kept"] >= 1 and not nan_ids & set(ref["order"].tolist()) and c.ban not in ref["order"].tolist()
        else:
            assert (ref["kept"], ref["out"]) == tuple(c.expect[0]), c.name
    assert len(seen) == 15
    # the same answers, spelled out on one small row
    x = torch.tensor([0.0, 3.0, 1.0, 2.0])
    x[1] = C.nan(False)
    assert S.sample_row(x, 2, 1.0, 1.0, u=0.0)["order"].tolist() == [3, 2]
    x[1] = C.nan(True)
    assert S.sample_row(x, 2, 1.0, 1.0, u=0.999)["out"] == 2
    x[2] = x[0] = C.INF
    assert (lambda r: (r["kept"], r["out"]))(S.sample_row(x, 2, 0.5, 1.0, u=0.999)) == (1, 0)
    assert (lambda r: (r["kept"], r["out"]))(S.sample_row(x, 2, 0.5, 1.0, ban=0, u=0.999)) == (1, 2)
    assert (lambda r: (r["kept"], r["out"]))(S.sample_row(torch.full((5,), C.NINF), 2, 0.5, 1.0, u=0.5)) == (-1, 0)
