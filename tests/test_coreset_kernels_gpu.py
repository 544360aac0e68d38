"""csrc/coreset.hip (mh_coreset_select, ops.coreset_select) on the GPU against the fp64 rule and the replay checker of
tests/coreset_ref.py (shown to reject the plausible mistakes by tests/test_coreset_cpu.py).  Outputs start as poison inside
poisoned frames; the class's neighbours in a larger bank are poison too."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from tests import coreset_ref as cr  # noqa: E402
from tests import fp64_bounds as fb  # noqa: E402

DEV = "cuda"
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
BORDER = 64
G = cr.GROUP_ROWS
ROWS = [1, 2, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 255, 256, 257, 1000]   # 63 / 64 / 65: the workgroup's edge


def bordered(n, dtype):
    buf = fb.poisoned((n + 2 * BORDER,), dtype, DEV)
    return buf, buf[BORDER:BORDER + n]


def framed_out(n, rows):
    bufs, views = zip(*(bordered(k, dt) for k, dt in ((n, I32), (n, F32), (1, F32), (rows, F32))))
    return bufs, ops.CoresetResult(*views)


def assert_frames(bufs, what):
    for buf, name in zip(bufs, ("sel", "radius2", "cover2", "mind")):
        fb.assert_untouched(buf[:BORDER], f"{what} {name} (before)")
        fb.assert_untouched(buf[-BORDER:], f"{what} {name} (behind)")


def to_dev(taps):
    return [t.to(DEV).contiguous() for t in taps]


def test_group_rows_is_what_the_tests_assume():
    """One 8-byte partial per workgroup: the workspace grows by 8 bytes exactly where a class needs one more workgroup."""
    lib = ops._L()
    assert lib.mh_coreset_ws_bytes(1) == 8 and lib.mh_coreset_ws_bytes(G) == 8 and lib.mh_coreset_ws_bytes(G + 1) == 16
    assert lib.mh_coreset_ws_bytes(0) < 0


# --------------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("last", [False, True], ids=["start0", "startlast"])
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("D", [8, 32, 96, 1280])
def test_exact_cases_bit_for_bit(D, T, last):
    """Small integers, duplicated rows: every fp32 operation is exact and ties are everywhere, so sel, radius2, cover2 and mind
    carry the bits of the fp64 rule.  Every row count of ROWS from start 0 or from start rows - 1, each with n in
    {1, 2, min(rows, 17), rows}; one fp64 run of n = rows per (rows, start) serves its values of n (the selection for n is a
    prefix)."""
    for rows in ROWS:
        host = cr.int_case(rows, D, T, seed=1000 * D + 10 * T + rows)
        taps = to_dev(host)
        start = rows - 1 if last else 0
        ns = sorted({1, min(rows, 2), min(rows, 17), rows})
        ref = cr.select_ref(host, rows, start, checkpoints=ns)
        for n in ns:
            what = f"D={D} T={T} rows={rows} start={start} n={n}"
            bufs, out = framed_out(n, rows)
            got = ops._coreset_select_into(out, taps, n, start=start)
            mind, cover2 = ref["at"][n]
            assert got.sel.tolist() == ref["sel"][:n], what
            assert torch.equal(got.radius2.cpu(), ref["radius2"][:n].float()), what
            assert torch.equal(got.mind.cpu(), mind.float()), what
            assert float(got.cover2) == cover2, what
            assert_frames(bufs, what)


def test_known_answer_on_the_device():
    rows = torch.tensor(cr.KNOWN_ROWS, dtype=F32)
    x = torch.zeros(6, 8)
    x[:, :4] = rows
    got = ops.coreset_select([x.to(BF16).to(DEV)], 6)
    assert got.sel.tolist() == cr.KNOWN_SEL and got.radius2.tolist() == cr.KNOWN_RADIUS2
    assert float(got.cover2) == -1.0 and got.mind.tolist() == [-1.0] * 6


@pytest.mark.parametrize("T,D", [(4, 1280), (8, 2048)])
def test_largest_staged_centres(T, D):
    """The two shapes the launcher has to take at least (T D = 5120 and 16384), a class that ends inside a workgroup."""
    host = cr.int_case(70, D, T, seed=T + D)
    ref = cr.select_ref(host, 9, start=3, checkpoints=(9,))
    got = ops.coreset_select(to_dev(host), 9, start=3)
    assert got.sel.tolist() == ref["sel"] and torch.equal(got.radius2.cpu(), ref["radius2"].float())
    assert torch.equal(got.mind.cpu(), ref["mind"].float()) and float(got.cover2) == ref["cover2"]


# ---------------------------------------------------------------------------------------------------- random unit rows
@pytest.mark.parametrize("rows,D,T,clusters", [(700, 96, 2, 0), (700, 96, 2, 9), (333, 1280, 4, 0), (333, 1280, 4, 5),
                                               (1500, 32, 1, 40)])
def test_random_unit_rows_replay(rows, D, T, clusters):
    host = cr.unit_case(rows, D, T, seed=rows + D + clusters, clusters=clusters)
    taps = to_dev(host)
    a = ops.coreset_select(taps, 64, start=rows // 2)
    worst = cr.replay_check(host, a.sel, a.radius2, start=rows // 2, mind=a.mind, cover2=a.cover2,
                            what=f"rows={rows} D={D} T={T} clusters={clusters}")
    print(f"coreset rows={rows} D={D} T={T} clusters={clusters}: worst radius err/bound {worst:.3f}")
    r = a.radius2.cpu()
    assert bool((r[1:-1] >= r[2:]).all()) and float(a.cover2) <= float(r[-1])          # non-increasing, bit for bit
    again = ops.coreset_select(taps, 64, start=rows // 2)
    for x, y, name in zip(a, again, a._fields):
        assert torch.equal(x, y), f"two runs differ in {name}"
    half = ops.coreset_select(taps, 32, start=rows // 2)
    assert torch.equal(half.sel, a.sel[:32]) and torch.equal(half.radius2, a.radius2[:32])     # nesting
    cr.replay_check(host, half.sel, half.radius2, mind=half.mind, cover2=half.cover2, what="n=32")
    assert bool((a.mind <= half.mind).all())                                            # mind only ever takes minima
    assert float(half.cover2) == float(a.radius2[32])                                   # the cover of 32 is the next radius


# ----------------------------------------------------------------------------------- a class in the middle of a larger bank
@pytest.mark.parametrize("rows,D,T,lead", [(G + 1, 96, 2, 37), (200, 1280, 4, 5), (2 * G, 32, 1, 1)])
def test_class_in_the_middle_of_a_poisoned_bank(rows, D, T, lead):
    """The rows before and behind the class are NaN poison: one read of them poisons a distance.  Every output has the bits of
    the class run alone, sel stays inside the class, and the frames around the outputs are untouched."""
    host = cr.unit_case(rows, D, T, seed=rows + lead, clusters=4)
    alone = ops.coreset_select(to_dev(host), min(rows, 40), start=rows - 1)
    banks = []
    for t in host:
        bank = fb.poisoned((lead + rows + 29, D), BF16, DEV)
        bank[lead:lead + rows] = t.to(DEV)
        banks.append(bank)
    n = min(rows, 40)
    bufs, out = framed_out(n, rows)
    got = ops._coreset_select_into(out, banks, n, row0=lead, rows=rows, start=rows - 1)
    for x, y, name in zip(alone, got, alone._fields):
        assert torch.equal(x, y), f"{name} depends on the class's place in the bank"
    assert int(got.sel.min()) >= 0 and int(got.sel.max()) < rows and bool(torch.isfinite(got.mind).all())
    assert_frames(bufs, "class in the middle")
    cr.replay_check(host, got.sel, got.radius2, start=rows - 1, mind=got.mind, cover2=got.cover2, what="middle class")


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched():
    T, D, rows, n = 2, 32, 100, 10
    taps = to_dev(cr.unit_case(rows, D, T, seed=1))
    bufs, out = framed_out(n, rows)
    lib, p = ops._L(), ops._p
    wsb = lib.mh_coreset_ws_bytes(rows)
    ws = fb.poisoned((wsb // 4,), I32, DEV)
    ptrs = (ctypes.c_void_p * T)(*(t.data_ptr() for t in taps))
    holes = (ctypes.c_void_p * T)(taps[0].data_ptr(), None)
    odd = (ctypes.c_void_p * T)(taps[0].data_ptr(), taps[1].data_ptr() + 2)
    good = dict(taps=ptrs, T=T, ld=D, D=D, row0=0, rows=rows, n=n, start=0, sel=p(out.sel), r2=p(out.radius2), mind=p(out.mind),
                cover2=p(out.cover2), ws=p(ws), wsb=wsb)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mh_coreset_select(a["taps"], a["T"], a["ld"], a["D"], a["row0"], a["rows"], a["n"], a["start"], a["sel"],
                                     a["r2"], a["mind"], a["cover2"], a["ws"], a["wsb"], ops._s())

    for kw in (dict(taps=None), dict(taps=holes), dict(taps=odd), dict(sel=None), dict(r2=None), dict(mind=None),
               dict(cover2=None), dict(ws=None), dict(T=0), dict(T=9), dict(D=0), dict(D=4), dict(D=12, ld=16), dict(ld=D - 8),
               dict(ld=D + 4), dict(row0=-1), dict(rows=0), dict(rows=-5), dict(n=0), dict(n=rows + 1), dict(start=-1),
               dict(start=rows), dict(wsb=wsb - 1), dict(wsb=0)):
        with pytest.raises(_lib.MyriadHipError, match="MH_ERR_ARG"):
            _lib.check(call(**kw), f"mh_coreset_select {kw}")
    with pytest.raises(_lib.MyriadHipError, match="MH_ERR_UNSUPPORTED"):
        _lib.check(call(T=2, D=8200, ld=8200), "mh_coreset_select T D = 16400")
    torch.cuda.synchronize()
    for buf in (*bufs, ws):
        fb.assert_untouched(buf, "refused mh_coreset_select")
    # the wrapper refuses what the launcher cannot see, before any launch
    f32 = [t.float() for t in taps]
    strided = [torch.cat([t, t], dim=1)[:, :D] for t in taps]
    for bad_taps, kw in ((f32, {}), (strided, {}), ([taps[0], taps[1][:-1]], {}), ([], {}), (taps * 5, {}),
                         ([t.cpu() for t in taps], {}), (taps, dict(row0=1, rows=rows)), (taps, dict(row0=-1, rows=rows)),
                         (taps, dict(rows=rows + 1)), (taps, dict(rows=0)), (taps, dict(start=rows)), (taps, dict(start=-1)),
                         ([t[:, :12].contiguous() for t in taps], {})):
        with pytest.raises(_lib.MyriadHipError):
            ops._coreset_select_into(out, bad_taps, n, **kw)
        with pytest.raises(_lib.MyriadHipError):
            ops.coreset_select(bad_taps, n, **kw)
    for bad_n in (0, rows + 1, -1):
        with pytest.raises(_lib.MyriadHipError):
            ops.coreset_select(taps, bad_n)
    with pytest.raises(_lib.MyriadHipError):
        ops._coreset_select_into(ops.CoresetResult(out.sel, out.radius2, out.cover2, out.mind[:-1]), taps, n)
    torch.cuda.synchronize()
    for buf in bufs:
        fb.assert_untouched(buf, "refused ops.coreset_select")
    assert math.isinf(float(ops._coreset_select_into(out, taps, n).radius2[0]))       # and the good call still runs
