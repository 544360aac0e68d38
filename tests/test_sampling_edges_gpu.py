"""The device sampler (mh_sample_rows, its slot form, the repetition penalty) where a wrong pick would go unnoticed: ties at the
k-th value, the two zeros, NaN and infinite logits, the widths at which the launch geometry changes, the candidate counts at which
the sort's padding changes, the knobs' ends and u next to 0 and 1.  The rows come from tests/sampling_edge_cases.py (the CPU file
test_sampling_edges_cpu.py shows that they discriminate); the reference is tests/sampling_ref.py under the contract written at
mh_sample_rows in include/myriad_hip.h.  Every launch writes into poisoned outputs with two spare entries and reads NaN-bordered
logits [R, ldl], ldl = V rounded up to 4 plus 4; u, margin and p_max are compared bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from tests import beam_sample_ref as BR  # noqa: E402
from tests import sampling_edge_cases as C  # noqa: E402
from tests import sampling_ref as S  # noqa: E402
from tests.test_slot_sampling_gpu import POISON, _bitmap, _i32, _out, _poisoned, _prm  # noqa: E402

DEV = "cuda:0"
F32, I32 = torch.float32, torch.int32
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
TIE_COUNTS = (1059, 8, 181)                  # compared, near, overflow rows of the tie grid, by the reference alone


def _bordered(x, border=float("nan"), guard_rows=0):
    """The [R, V] rows of x (CPU, copied bit for bit) inside a [R + guard_rows, ldl] device buffer filled with `border`."""
    R_, V = x.shape
    ldl = (V + 3) // 4 * 4 + 4
    full = torch.full((R_ + guard_rows, ldl), border, dtype=F32)
    full.view(I32)[:R_, :V] = x.contiguous().view(I32)
    full = full.to(DEV)
    return full, full[:R_, :V]


def _same(a, b):
    """torch.equal, a NaN equal to a NaN."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _bits(t):
    return t.detach().cpu().contiguous().view(I32)


def _run(c):
    """One mh_sample_rows launch of `c` with what every case asserts: u is the host Philox, margin and p_max are
    mh_argmax_pmax_rows' on the same view, ban and inv_temp, nothing past row R and nothing of the logits was written, every id
    lies in [0, V).  Returns the outputs and the arg-max on the host."""
    full, x = _bordered(c.x)
    before = _bits(full)
    bf, b = _out(c.R)
    prm = torch.tensor([c.inv_temp, c.top_p, float(c.top_k), 1.0], dtype=F32, device=DEV)
    seed = torch.tensor([c.seed], dtype=torch.long, device=DEV)
    step = _i32([c.t - 1]) if c.t else None                          # t = *step + t_add, or t_add alone
    ops.sample_rows(x, b["out"], b["mar"], b["pmx"], b["kept"], prm, seed, ban_id=c.ban, step=step, t_add=1 if c.t else 0,
                    u_out=b["u"])
    _, am = _out(c.R)
    ops.argmax_pmax_rows(x, am["out"], am["mar"], am["pmx"], ban_id=c.ban, inv_temp=c.inv_temp)
    torch.cuda.synchronize()
    assert _poisoned(bf, c.R), c.name
    assert torch.equal(_bits(full), before), c.name
    got = {k: v.cpu() for k, v in b.items()}
    for r in range(c.R):
        assert float(got["u"][r]) == c.u(r), (c.name, r)
    assert _same(got["mar"], am["mar"].cpu()) and _same(got["pmx"], am["pmx"].cpu()), c.name
    assert bool(((got["out"] >= 0) & (got["out"] < c.V)).all()), (c.name, got["out"])
    return got, am["out"].cpu()


def _check_direct(cases):
    """kept and out of every row against the reference (and the closed-form answer where the case carries one); the rows that
    differ are collected, so that one run names them all."""
    bad = []
    for c in cases:
        got, top = _run(c)
        for r, ref in enumerate(c.ref()):
            assert c.expect is not None or not ref["near"], c.name
            want = (ref["kept"], ref["out"])
            if c.expect is not None:
                assert want == tuple(c.expect[r]), c.name
            if want[0] == -1:
                assert want[1] == int(top[r]), c.name
            if (int(got["kept"][r]), int(got["out"][r])) != want:
                bad.append((c.name, r, (int(got["kept"][r]), int(got["out"][r])), want))
    for row in bad:
        print("differs (case, row, got, want):", *row)
    assert not bad, (len(bad), bad[:20])
    return len(cases)


# ------------------------------------------------------------------------------------------------ 1-5: the uniform entry
def test_tie_grid_equals_the_reference():
    """Quantised logits (steps 1/4 and 1/64) at V = 1 .. 32768, top_k 1 / 2 / 50 / 1024, top_p 0.01 / 0.5 / 0.9 / 1.0, three rows,
    T cycled over (0.7, 1.0, 1.3), the last id banned in every other launch.  Of the 1248 rows the reference compares 1059, marks
    8 `near` (0.6 %, skipped: fp32 summation order may move the cut or the pick) and calls 181 overflow (a tied top-k set past
    1024 candidates, or nothing finite at V = 1 under the ban), which are asserted: kept = -1 and out = the arg-max."""
    rows = near = over = 0
    bad = []
    for c in C.tie_grid():
        got, top = _run(c)
        for r, ref in enumerate(c.ref()):
            pair = (int(got["kept"][r]), int(got["out"][r]))
            if ref["kept"] == -1:
                over += 1
                assert ref["out"] == int(top[r]), (c.name, r)
                if pair != (-1, ref["out"]):
                    bad.append((c.name, r, pair, (-1, ref["out"])))
                continue
            if ref["near"]:
                near += 1
                continue
            rows += 1
            if pair != (ref["kept"], ref["out"]):
                bad.append((c.name, r, pair, (ref["kept"], ref["out"])))
    for row in bad:
        print("differs (case, row, got, want):", *row)
    print("sampler tie grid: compared", rows, "near", near, "overflow", over, "differing", len(bad))
    assert not bad, (len(bad), bad[:20])
    assert (rows, near, over) == TIE_COUNTS and rows + near + over == 1248
    assert near <= 0.02 * (rows + near + over), (near, rows)


def test_sort_padding_and_cap_edges():
    """Distinct logits -i / 256 permuted over V = 2048 ids, top_p = 1, top_k = n for n = 1, 2, 3, 511, 512, 513, 1023, 1024 (each
    side of a power-of-two padding of the bitonic sort, and the cap): kept = n, the pick follows the order at a seed clear of
    every boundary, at u next to 1 (the last candidate) and at u = 0 (the first).  One more value tied at rank 1024 under
    top_k = 1024 is 1025 candidates: kept = -1 and the arg-max.  top_k = 5 at V = 3 keeps 3."""
    cases = C.pad_cases()
    assert [c.ref()[0]["kept"] for c in cases if c.name.startswith("pad_n") and "_u_" not in c.name] == list(C.PAD_N)
    assert next(c for c in cases if c.name == "pad_k5_V3").ref()[0]["kept"] == 3
    assert _check_direct(cases) == 3 * len(C.PAD_N) + 3


def test_signed_zeros_are_one_value():
    """[1, 0, -0, -0, -1, 0, -2, -3] and its sign-swapped twin, alone (V = 8), ending in the one-element last float4 of V = 4097
    and across the boundary of waves 0 and 1 (ids 252..259 of V = 300); top_k 2 and 3.  top_p = 1 keeps ids 0 1 2 3 5 in that
    order, with seeds (host search) whose u lands in the mass of id 2, 3 and 5; top_p = 0.5 keeps ids 0 and 1."""
    assert _check_direct(C.zero_cases()) == 60


def test_nan_and_infinite_rows():
    """V = 37 and 4097, top_k = 5, top_p 0.9 and 1.0.  A NaN of either sign (explicit bit patterns) at id 0, at V - 1, at the
    would-be arg-max and on the banned id: the row draws as with -inf there.  All NaN, all -inf, -inf except the banned id:
    kept = -1, out = 0.  One +inf, two +inf (the lower id), +inf behind a NaN: that id, kept = 1.  +inf on the banned id: an
    ordinary draw among the rest."""
    cases = C.nonfinite_cases()
    for c in cases:                                                   # the NaN survives the upload with its sign
        nan_ids = torch.nonzero(torch.isnan(c.x[0])).flatten()
        assert all(int(_bits(c.x[0])[i]) & 0x7FFFFFFF == C.POS_NAN for i in nan_ids)
    assert _check_direct(cases) == 60


def test_extreme_knobs_and_uniforms_next_to_0_and_1():
    """top_p = 0: kept = 1 and the arg-max (asserted directly: the reference's `near` fires there by construction).  top_p = 1.5
    keeps the whole top-k set.  inv_temp = 20 and 0.05, and inv_temp = 20 on logits of 1e38: the lowest id pushed to +inf.  u = 0, 2^-22, 1 - 2^-24 and 1 - 2^-23 (hard-coded seeds) on a peaked
    row, which every u answers with the arg-max, and on flat rows of 8 and of 1024 equal logits, where every sum is an integer:
    top_p = 1 keeps all and picks id 0 / the last, top_p = 0.5 keeps exactly half and picks id 0 / the last of that half."""
    for s, u in C.LOW_SEEDS + C.HIGH_SEEDS:
        assert S.uniform(s, 0, 0) == u and (u < 2.0 ** -20 or u > 1.0 - 2.0 ** -20)
    assert _check_direct(C.knob_cases()) == 36


# ------------------------------------------------------------------------------------------------ 6: the slot form
def test_slot_form_draws_what_the_uniform_entry_draws_on_the_edge_rows():
    """The rows of the three tests above through mh_sample_rows_slots at odd slots, idle slots in between holding live-looking
    logits, each row with its own (seed, gen): a live row equals mh_sample_rows' row-0 draw at that seed and step (which those
    tests hold to the reference), an idle row writes (-1, 0, 0, 0) and nothing else.  mh_argmax_pmax_rows_slots on the NaN / inf /
    ban rows equals mh_argmax_pmax_rows."""
    for c in C.zero_cases() + C.nonfinite_cases() + C.knob_cases():
        RS = 2 * c.R + 1
        src = [min(s // 2, c.R - 1) for s in range(RS)]
        live_h = [s % 2 for s in range(RS)]
        full, x = _bordered(c.x[src])
        before = _bits(full)
        seed_h = [c.seed + 31 * (s // 2) for s in range(RS)]
        eos, min_length = (c.ban, c.t + 1) if c.ban >= 0 else (2, 0)
        prm = _prm(c.inv_temp, c.top_p, c.top_k, 1.0, min_length, eos)
        gen, live = _i32([c.t] * RS), _i32(live_h)
        bf, b = _out(RS)
        ops.sample_rows_slots(x, b["out"], b["mar"], b["pmx"], b["kept"], prm, torch.tensor(seed_h, dtype=torch.long, device=DEV),
                              gen, live, u_out=b["u"])
        pf, p = _out(RS)
        ops.argmax_pmax_rows_slots(x, p["out"], p["mar"], p["pmx"], prm, gen, live)
        torch.cuda.synchronize()
        assert _poisoned(bf, RS) and torch.equal(_bits(full), before), c.name
        assert bool((pf["out"][RS:] == -77).all() and (pf["mar"][RS:] == POISON).all() and (pf["pmx"][RS:] == POISON).all())
        assert bool((p["kept"] == -99).all() and (p["u"] == POISON).all())            # the greedy form has neither
        for s in range(RS):
            if not live_h[s]:
                assert int(b["out"][s]) == -1 and int(b["kept"][s]) == 0 and float(b["mar"][s]) == 0 and float(b["pmx"][s]) == 0
                assert float(b["u"][s]) == POISON
                assert int(p["out"][s]) == -1 and float(p["mar"][s]) == 0 and float(p["pmx"][s]) == 0
                continue
            _, one = _out(1)
            ops.sample_rows(x[s:s + 1], one["out"], one["mar"], one["pmx"], one["kept"], prm[:4],
                            torch.tensor([seed_h[s]], dtype=torch.long, device=DEV), ban_id=c.ban, t_add=c.t, u_out=one["u"])
            assert float(one["u"][0]) == S.uniform(seed_h[s], c.t, 0)
            for k in ("out", "kept", "u"):
                assert torch.equal(b[k][s:s + 1], one[k]), (c.name, k, s)
            _, am = _out(1)
            ops.argmax_pmax_rows(x[s:s + 1], am["out"], am["mar"], am["pmx"], ban_id=c.ban, inv_temp=c.inv_temp)
            for k in ("mar", "pmx"):
                assert _same(b[k][s:s + 1], one[k]) and _same(p[k][s:s + 1], am[k]) and _same(one[k], am[k]), (c.name, k, s)
            assert torch.equal(p["out"][s:s + 1], am["out"]), (c.name, s)
            assert 0 <= int(b["out"][s]) < c.V
            if s == 1:                                               # slot 1 is the case's own row 0 at its own seed
                ref = c.ref()[0]
                assert (int(b["kept"][s]), int(b["out"][s])) == (ref["kept"], ref["out"]), c.name


# ------------------------------------------------------------------------------------------------ 7: the repetition penalty
GUARD = 123.0           # the border of the penalty tests: finite, so a penalty applied to it shows (NaN / p is the same NaN)


def _marked(words):
    bits = words.cpu().numpy().view(np.uint32)
    return {w * 32 + b for w in range(len(bits)) for b in range(32) if bits[w] >> b & 1}


def _penalty_case(slots, x0, seen0, prev, penalty, in_range):
    """Two launches on fresh logits with the same prev_ids: the bitmap gains prev_ids[r] where it lies in [0, V) and is then
    unchanged by the second; every marked id < V is penalised once, nothing else changes, the border and one guard row behind
    the last row included.  In the slot form the last row is idle: its logits and bitmap stay bit for bit."""
    R_, V = x0.shape
    live_h = [1] * R_
    if slots:
        live_h[-1] = 0
    pen = torch.tensor([penalty], device=DEV)
    prev_d = torch.tensor(prev, dtype=torch.long, device=DEV)
    seen = seen0.clone().to(DEV)
    for launch in range(2):
        full, x = _bordered(x0, border=GUARD, guard_rows=1)
        if slots:
            ops.repetition_penalty_rows_slots(x, seen, prev_d, pen, _i32(live_h))
        else:
            ops.repetition_penalty_rows(x, seen, prev_d, pen)
        torch.cuda.synchronize()
        got = full.cpu()
        assert bool((got[:R_, V:] == GUARD).all()) and bool((got[R_:] == GUARD).all()), launch
        for r in range(R_):
            before = _marked(seen0[r])
            if not live_h[r]:
                assert torch.equal(_bits(got[r, :V]), _bits(x0[r])) and _marked(seen[r]) == before
                continue
            want_marked = before | ({prev[r]} if in_range[r] else set())
            assert _marked(seen[r]) == want_marked, (launch, r)
            want = S.penalize(x0[r], [i for i in want_marked if i < V], penalty)
            assert torch.allclose(got[r, :V], want, rtol=1e-6, atol=0, equal_nan=True), (launch, r)
            fin = ~torch.isnan(want)
            assert torch.equal(torch.signbit(got[r, :V])[fin], torch.signbit(want)[fin]), (launch, r)    # -0 stays -0, -inf -inf
            untouched = torch.ones(V, dtype=torch.bool)
            untouched[[i for i in want_marked if i < V]] = False
            assert torch.equal(_bits(got[r, :V])[untouched], _bits(x0[r])[untouched]), (launch, r)


@pytest.mark.parametrize("penalty", [1.3, 0.5])
@pytest.mark.parametrize("slots", [False, True], ids=["uniform", "slots"])
def test_penalty_at_the_last_id_out_of_range_ids_and_stale_bits(slots, penalty):
    """V = 37 (V % 32 = 5): prev_id = V - 1 is marked; prev_id = V, -1 and 2^31 are ignored, bitmap unchanged.  Every row's last
    bitmap word carries stale bits for ids 37, 40 and 63 (the border of its own row, and element 19 of the next row or of the
    guard row): nothing there moves.  The seen ids' logits are +0, -0, -inf, NaN and ordinary values of both signs."""
    V = 37
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(5, V, generator=g) * 2.0
    x0[:, 3] = torch.cat([C.f32_bits([0x00000000, 0x80000000]), torch.tensor([C.NINF]), C.nan(False)[None], C.f32_bits([0x80000000])])
    seen0 = _bitmap([[3, 20, 31, 32]] * 5, V).cpu()
    seen0[:, 1] |= (1 << 5) | (1 << 8) | (-2 ** 31)                   # ids 37, 40, 63: past V
    _penalty_case(slots, x0, seen0, [V - 1, V, -1, 2 ** 31, V - 1], penalty, [True, False, False, False, True])


@pytest.mark.parametrize("slots", [False, True], ids=["uniform", "slots"])
def test_penalty_over_four_sweeps_of_the_bitmap(slots):
    """V = 32768: 1024 bitmap words, four sweeps of the 256 threads; prev_ids land in words 255, 256 and 1023 (the last word of
    the first sweep, the first of the second, the last of all), earlier ids sit in every sweep."""
    V = 32768
    x0 = torch.randn(4, V, generator=torch.Generator().manual_seed(8)) * 2.0
    seen0 = _bitmap([[5, 8191, 9000, 20000, 32000]] * 4, V).cpu()
    _penalty_case(slots, x0, seen0, [255 * 32 + 7, 256 * 32, 1023 * 32 + 31, 256 * 32 + 1], 1.3, [True] * 4)


# ------------------------------------------------------------------------------------------------ 8: refusals
def test_uniform_entries_refuse_bad_arguments_and_launch_nothing():
    R_, V = 2, 1000
    x = torch.ones((R_, V), device=DEV)
    prm, seed = torch.tensor([1.0, 0.9, 50.0, 1.3], device=DEV), torch.tensor([7], dtype=torch.long, device=DEV)
    bf, b = _out(R_)

    def sample(logits=x, **kw):
        a = dict(out=b["out"], mar=b["mar"], pmx=b["pmx"], kept=b["kept"], prm=prm, seed=seed)
        a.update(kw)
        ops.sample_rows(logits, a["out"], a["mar"], a["pmx"], a["kept"], a["prm"], a["seed"], u_out=b["u"])

    flat = torch.ones(R_ * 32776 + 8, device=DEV)
    wide = flat[:R_ * 32772].view(R_, 32772)[:, :32769]                            # V = 32769
    odd = flat[:R_ * (V + 2)].view(R_, V + 2)[:, :V]                               # ldl % 4 != 0
    off = flat[1:1 + R_ * V].view(R_, V)                                           # rows 4 bytes off a 16-byte boundary
    assert off.data_ptr() % 16 == 4 and off.stride(0) % 4 == 0
    for bad in (wide, odd, off):
        with pytest.raises(_lib.MyriadHipError, match="MH_ERR_UNSUPPORTED"):
            sample(logits=bad)
    short = torch.as_strided(flat, (R_, V), (V - 4, 1))                            # ldl < V
    for bad in (short, x[:, :0]):                                                  # ... and V = 0
        with pytest.raises(_lib.MyriadHipError, match="MH_ERR_ARG"):
            sample(logits=bad)
    for k in ("out", "kept", "prm", "seed"):
        with pytest.raises(_lib.MyriadHipError, match="MH_ERR_ARG"):
            sample(**{k: None})
    args = [ops._p(x), x.stride(0), ops._p(b["out"]), ops._p(b["mar"]), ops._p(b["pmx"]), ops._p(b["kept"]), ops._p(b["u"]), R_, V, -1,
            ops._p(prm), ops._p(seed), None, 0, ops._s()]
    assert ops._L().mh_sample_rows(None, *args[1:]) == ERR_ARG                     # null logits
    args[7] = 0
    assert ops._L().mh_sample_rows(*args) == OK                                    # R = 0: nothing to do
    sample(logits=x[:0])

    seen = torch.zeros((R_, 32), dtype=I32, device=DEV)
    for a in ((x, None, None, prm[3:]), (x, seen, None, None), (short, seen, None, prm[3:]), (x[:, :0], seen, None, prm[3:])):
        with pytest.raises(_lib.MyriadHipError, match="MH_ERR_ARG"):
            ops.repetition_penalty_rows(*a)
    assert ops._L().mh_repetition_penalty_rows(None, x.stride(0), ops._p(seen), None, R_, V, ops._p(prm[3:]), ops._s()) == ERR_ARG
    seen[:] = -1                                                                   # every id marked: a launch would show
    ops.repetition_penalty_rows(x[:0], seen[:0], None, prm[3:])
    torch.cuda.synchronize()
    assert _poisoned(bf) and bool((x == 1.0).all()) and bool((flat == 1.0).all()) and bool((seen == -1).all())


# ------------------------------------------------------------------------------------------------ the beam sampler shares smp_key
def test_beam_sampler_orders_a_zero_tie_by_id():
    """mh_beam_sample_topk at inv_temp = 0 (an infinite temperature): the tempered log-prob of the row's one certain token is +0,
    every other one's is -0, so the k-th value is a tie of the two zeros over the whole row and the top-p cut (0.3 of 16 equal
    masses: exclusive mass 0 .. 4 < 4.8) keeps ids 0 .. 4 of each row in id order -- not the +0 token first.  The seed is chosen
    (host search) so that the +0 token of row 0, which is not kept, has the largest Gumbel key of ids 0 .. 5: a sort that puts
    +0 above -0 selects it.  Against tests/beam_sample_ref.py."""
    from tests.test_beam_sample_gpu import _check_item, _device_logits, _run as _beam_run
    V, nb, t = 16, 2, 3
    logits = torch.randn(nb, V, generator=torch.Generator().manual_seed(16)) * 3.0
    logits[0, 5], logits[1, 9] = 60.0, 60.0
    scores = torch.tensor([0.0, -0.5])
    seed = next(s for s in range(C.SEED, C.SEED + 4096) if int(torch.argmax(BR.gumbel(s, t, range(6), 0))) == 5)
    ref = BR.step(logits, scores, [[], []], 1, nb, -1, 0.0, 2, 0.3, 1.0, seed, t)[0]
    assert not ref.near and sorted(ref.acc) == [0, 1, 2, 3, 4, 16, 17, 18, 19, 20]
    prm = torch.tensor([0.0, 0.3, 2.0, 1.0], dtype=F32, device=DEV)
    acc, flat, key, flag = _beam_run(_device_logits(logits, 4), scores.to(DEV), 1, nb, prm,
                                     torch.tensor([seed], dtype=torch.long, device=DEV), t=t, what="zero tie")
    assert not flag.any()
    _check_item("zero tie", ref, acc[0], flat[0], key[0], V)
