"""Reference and error bound of mh_token_scores_rows (csrc/scores.hip): the log-softmax, at temperature 1, of an f32 logits row
at a few ids.  `ref64` is the float64 reference, `restate_f32` a plain f32 numpy restatement of the kernel's arithmetic (not of its
summation order), `bound` the per-entry tolerance E(X, V) derived below, and `mistakes` the plausible wrong kernels the CPU test
shows to land outside it.

The bound.  u = 2^-24 (f32 unit round-off), X = max |x_j| over the row's V columns, m = max_j x_j, T = the terms one thread adds
(32 with the row in registers: 8 float4; ceil(V / 1024) on the strided path).  The kernel computes, in f32,

    d_j  = x_j - m                        |error| <= u |d_j| <= 2 X u                       (one rounding)
    e_j  = expf(d_j)                      relative error <= 2 X u   (the argument's error, exp' = exp)
                                                         + 2 u      (expf: 1 ulp = 2^-23 relative, the HIP math API's table)
    s    = sum_j e_j                      relative error <= (T + 6 + 16) u on top: every term is positive, so each addition's
                                          rounding is relative to a partial sum <= s; a term passes through at most T - 1
                                          additions in its thread, 6 in the wave's butterfly and 16 across the 16 waves
    l    = logf(s)                        s in [1, V] (the maximum's term is exactly 1), so l in [0, ln V]:
                                          |error| <= (relative error of s)  (log' = 1 / s)  +  2 u ln V  (logf: 1 ulp of l)
    lse  = m + l                          |error| <= u (X + ln V)                            (one rounding)
    out  = x_j - lse                      |error| <= u |x_j - lse| <= u (2 X + ln V)         (one rounding)

An e_j below the smallest normal number may be flushed to zero: V * 2^-126 against s >= 1, nothing at this scale.  Summing the
first-order terms:

    E(X, V) = 1.01 * u * (5 X + 4 ln V + T + 24),   T = max(32, ceil(V / 1024))

The factor 1.01 covers the products of the terms above (every relative error here is below 2^-10, so second-order terms are below
a thousandth of the first-order ones).  Nothing in it was fitted to the kernel's output.  The same bound holds for out[0] = lse
itself, whose error is a part of the above."""
import math

import numpy as np

U = 2.0 ** -24


def bound(X: float, V: int) -> float:
    T = max(32, -(-int(V) // 1024))
    return 1.01 * U * (5.0 * float(X) + 4.0 * math.log(V) + T + 24.0)


def ref64(x_row, ids):
    """(lse, [x[id] - lse for id in ids]) in float64 of one f32 row (a numpy array of V entries); -inf entries are fine."""
    x = np.asarray(x_row, dtype=np.float64)
    m = x.max()
    lse = m + math.log(np.exp(x - m).sum())
    return lse, np.array([x[int(i)] - lse for i in ids], dtype=np.float64)


def restate_f32(x_row, ids):
    """The kernel's arithmetic in plain f32 numpy: subtract the maximum, exp, sum, log, two additions."""
    x = np.asarray(x_row, dtype=np.float32)
    m = x.max()
    lse = np.float32(m + np.log(np.exp(x - m, dtype=np.float32).sum(dtype=np.float32), dtype=np.float32))
    return lse, np.array([x[int(i)] - lse for i in ids], dtype=np.float32)


def within(got, want, E: float) -> bool:
    """Every entry of `got` within E of `want`; an infinite reference entry (a -inf logit) must be met exactly; NaN never passes."""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    fin = np.isfinite(want)
    return bool(np.all(got[~fin] == want[~fin]) and np.all(np.abs(got[fin] - want[fin]) <= E))


# ---------------------------------------------------------------- plausible mistakes (f32 numpy, like restate_f32)
def _lse32(x):
    m = x.max()
    return np.float32(m + np.log(np.exp(x - m, dtype=np.float32).sum(dtype=np.float32), dtype=np.float32))


def mistake_ban_in_normaliser(x_row, ids, eos: int):
    """The EOS ban applied to the row before the normaliser (the pick kernels' view of the row)."""
    x = np.asarray(x_row, dtype=np.float32).copy()
    raw = x.copy()
    x[eos] = -np.inf
    lse = _lse32(x)
    return lse, np.array([raw[int(i)] - lse for i in ids], dtype=np.float32)


def mistake_temperature(x_row, ids, inv_temp: float):
    """The sampling temperature applied (p_max's convention)."""
    x = np.asarray(x_row, dtype=np.float32) * np.float32(inv_temp)
    lse = _lse32(x)
    return lse, np.array([x[int(i)] - lse for i in ids], dtype=np.float32)


def mistake_no_max(x_row, ids):
    """log(sum exp(x)) without subtracting the maximum."""
    x = np.asarray(x_row, dtype=np.float32)
    with np.errstate(over="ignore"):
        lse = np.log(np.exp(x, dtype=np.float32).sum(dtype=np.float32), dtype=np.float32)
    return lse, np.array([x[int(i)] - lse for i in ids], dtype=np.float32)


def mistake_border(buf_row, V: int, ids):
    """Columns past V of the padded row read (whole float4 loads at a ragged tail)."""
    with np.errstate(invalid="ignore"):
        return restate_f32(np.asarray(buf_row, dtype=np.float32)[:(V + 3) // 4 * 4 + 4], ids)


def mistake_neighbour_lse(x_rows, r: int, ids):
    """Row r's entries against row r + 1's normaliser (a row-index slip in the output write)."""
    lse, _ = restate_f32(x_rows[(r + 1) % len(x_rows)], ())
    x = np.asarray(x_rows[r], dtype=np.float32)
    return lse, np.array([x[int(i)] - lse for i in ids], dtype=np.float32)


# ---------------------------------------------------------------- the kernel test's cases (shared by the CPU and the GPU test)
GRID_V = (32000, 1000, 999, 33000)      # the register path, a ragged tail on it, an odd V on the fallback, V above 32768
R = 6
LIVE = (1, 0, 1, 1, 1, 1)               # row 1 is idle by its flag, row 4 by its id (-1)
X80_ROW, INF_ROW, INF_COL = 2, 3, 7     # a row scaled to max |x| = 80; a row with a -inf entry that is also watched
POISON = -777.25


def watch_sets(V: int):
    """Empty, the two ends, and eight ids with a duplicate and a -1 (INF_COL among them)."""
    return [], [0, V - 1], [INF_COL, 5, V - 1, 5, -1, 0, 123, V // 2]


def make_case(V: int):
    """(buf [R, ldl] f32 NaN-filled with the logits in [:, :V], ldl, ids [R] int64): ldl != V, a multiple of 4 where V is one (the
    register path's condition) and odd otherwise; ids = the arg-max on rows 0 and 2, a random id on rows 3 and 5, -1 on row 4."""
    rng = np.random.default_rng(1000 + V)
    ldl = V + 8 if V % 4 == 0 else V + 4
    buf = np.full((R, ldl), np.nan, dtype=np.float32)
    x = (rng.standard_normal((R, V)) * 3.0).astype(np.float32)
    x[X80_ROW] *= np.float32(80.0) / np.abs(x[X80_ROW]).max()
    x[INF_ROW, INF_COL] = -np.inf
    buf[:, :V] = x
    ids = np.array([x[0].argmax(), rng.integers(V), x[2].argmax(), rng.integers(V), -1, rng.integers(V)], dtype=np.int64)
    if ids[3] == INF_COL:
        ids[3] += 1
    return buf, ldl, ids


def row_X(x_row) -> float:
    x = np.asarray(x_row, dtype=np.float64)
    return float(np.abs(x[np.isfinite(x)]).max())
