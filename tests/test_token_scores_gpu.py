"""mh_token_scores_rows per entry against the float64 log-softmax within the derived bound of tests/token_scores_ref.py, on both
launch paths, with idle rows, NaN borders, a poisoned output and every refusal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from tests import token_scores_ref as T  # noqa: E402

DEV = "cuda:0"


def _launch(buf_d, V, ids_d, watch, live_d):
    """One launch into a poisoned [SCORE_ROWS + 2, R + 2] buffer (ldo = R + 2, two rows beyond the ten); the whole buffer back."""
    out = torch.full((ops.SCORE_ROWS + 2, T.R + 2), T.POISON, dtype=torch.float32, device=DEV)
    table = ops.score_watch_table([w for w in watch if w >= 0], V)
    table[:len(watch)] = torch.tensor(watch, dtype=torch.int32)                 # the -1 stays where the set has it
    ops.token_scores_rows(buf_d[:, :V], ids_d, table.to(DEV), out[:ops.SCORE_ROWS], live_d)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("V", T.GRID_V)
def test_token_scores_rows_against_fp64_within_the_derived_bound(V):
    buf, ldl, ids = T.make_case(V)
    buf_d, ids_d = torch.from_numpy(buf).to(DEV), torch.from_numpy(ids).to(DEV)
    live_d = torch.tensor(T.LIVE, dtype=torch.int32, device=DEV)
    assert buf_d.stride(0) == ldl != V
    worst = 0.0
    for watch in T.watch_sets(V):
        for live in (live_d, None):
            out = _launch(buf_d, V, ids_d, watch, live)
            assert np.all(out[ops.SCORE_ROWS:] == T.POISON) and np.all(out[:, T.R:] == T.POISON)     # outside [0:10, 0:R]
            for r in range(T.R):
                got = out[:ops.SCORE_ROWS, r]
                if ids[r] < 0 or (live is not None and not T.LIVE[r]):
                    assert np.all(got == 0.0), (V, r, got)
                    continue
                row = buf[r, :V]
                E = T.bound(T.row_X(row), V)
                lse, lp = T.ref64(row, [ids[r]] + [w for w in watch if w >= 0])
                assert T.within(got[:2], [lse, lp[0]], E), (V, r, got[:2], lse, lp[0], E)
                k = 1
                for w, wid in enumerate(watch):
                    if wid < 0:
                        assert got[2 + w] == 0.0
                        continue
                    assert T.within(got[2 + w], lp[k], E), (V, r, w, got[2 + w], lp[k], E)
                    if np.isfinite(lp[k]):
                        worst = max(worst, abs(float(got[2 + w]) - lp[k]) / E)
                    k += 1
                assert np.all(got[2 + len(watch):] == 0.0)                       # unused watch slots
                if r == T.INF_ROW and T.INF_COL in watch:
                    assert got[2 + watch.index(T.INF_COL)] == -np.inf
            if live is not None:                                                 # idle logits rows are bit-unchanged
                back = buf_d.cpu().numpy()
                assert np.array_equal(back.view(np.int32), buf.view(np.int32))
    print(f"V={V}: worst |err| / E = {worst:.3f}")


def test_token_scores_rows_refusals_leave_the_output_untouched():
    V = 1000
    buf, ldl, ids = T.make_case(V)
    buf_d, ids_d = torch.from_numpy(buf).to(DEV), torch.from_numpy(ids).to(DEV)
    watch = ops.score_watch_table([0, V - 1], V).to(DEV)
    out = torch.full((ops.SCORE_ROWS, T.R + 2), T.POISON, dtype=torch.float32, device=DEV)
    L, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()                                                   # noqa: E731
    good = [p(buf_d), ldl, p(ids_d), p(watch), p(out), T.R + 2, T.R, V, None, s]
    assert L.mh_token_scores_rows(*good) == 0
    torch.cuda.synchronize()
    assert float(out[0, 0]) != T.POISON
    out.fill_(T.POISON)
    for at, bad in ((0, None), (2, None), (3, None), (4, None), (7, 0), (7, -3), (5, T.R - 1)):
        args = list(good)
        args[at] = bad
        assert L.mh_token_scores_rows(*args) == -1, (at, bad)                    # MH_ERR_ARG
    for rows in (0, -2):                                                         # nothing to do: MH_OK, no launch
        args = list(good)
        args[6] = rows
        assert L.mh_token_scores_rows(*args) == 0
    torch.cuda.synchronize()
    assert bool((out == T.POISON).all())
    with pytest.raises(_lib.MyriadHipError):                                     # the wrapper: a watch table of another size
        ops.token_scores_rows(buf_d[:, :V], ids_d, watch[:4], out)
    assert bool((out == T.POISON).all())
