"""fp64 restatement of the greedy k-centre (farthest-point) coreset rule (csrc/coreset.hip), the replay checker
that holds a kernel's own selection history to it, and the case builders the CPU and GPU tests share.  Nothing here is measured
on the kernel.

The rule, on T row-major matrices x_t [rows, D] (the bf16 values, widened exactly):
    dist2(i, s) = sum_t sum_k (x_t[i, k] - x_t[s, k])^2
    sel[0] = start; radius2[0] = +inf; mind[i] = +inf
    for j = 0 .. n-1:  mind[i] = min(mind[i], dist2(i, sel[j])) for every i;  mind[sel[j]] = -1
                       if j + 1 < n:  sel[j+1] = the LOWEST index among argmax_i mind[i];  radius2[j+1] = that maximum
    cover2 = max_i mind[i] after the last update (-1 when n == rows)

The bound.  A fp32 dist2 (bf16 operands widened exactly, differences, squares and sums in fp32, the sums in any order) is within
gamma * dist2_64 of the fp64 value, gamma = (D T + 3) u32 / (1 - (D T + 3) u32): one rounding for the difference (counted twice
in the square), one for the square and D T - 1 for the sum of the non-negative terms; fused multiply-adds only remove roundings.
min is exact and monotone, hence |mind32[i] - M64[i]| <= gamma * M64[i] for the M64 built from the SAME centres.

The kernel's sequence may leave the fp64 sequence at a near tie and then stays on its own, equally valid, path; so the checker
replays the kernel's own history: at every step j >= 1 it builds M64 from sel[:j] and requires
    sel[j] in range and not selected before,
    M64[sel[j]] (1 + gamma) >= max_i M64[i] (1 - gamma)            (the pick is a maximum up to the rounding of both sides)
    |radius2[j] - M64[sel[j]]| <= gamma M64[sel[j]]
    no unselected row i < sel[j] is identical to row sel[j] in every tap   (dist2's bits depend on its two rows only, so such a
                                                                            row has the same fp32 mind: the lowest index wins)
and, given `exact=True` (integer inputs small enough that every fp32 operation is exact), equality with the fp64 rule."""
import math

import torch

from tests import fp64_bounds as fb

U32 = fb.U32
BF16 = torch.bfloat16
GROUP_ROWS = 64             # rows of one coreset_update workgroup (CS_ROWS; the GPU tests check the library's value)


def gamma(D: int, T: int) -> float:
    k = (D * T + 3) * U32
    return k / (1.0 - k)


def as64(taps):
    return [t.detach().cpu().double() for t in taps]


def dist2_to(x64, s: int) -> torch.Tensor:
    """[rows] fp64: the squared distance of every row to row s, summed over the taps."""
    d = torch.zeros(x64[0].shape[0], dtype=torch.float64)
    for x in x64:
        d = d + ((x - x[s]) ** 2).sum(dim=1)
    return d


def select_ref(taps, n: int, start: int = 0, checkpoints=()):
    """The rule in fp64.  taps: the class's own rows, one [rows, D] tensor per tap.  Returns dict(sel [n] list, radius2 [n] fp64,
    cover2 float, mind [rows] fp64); with `checkpoints` (values of n' <= n) also at[n'] = (mind, cover2) after n' steps: the
    selection for n' is the prefix sel[:n'], radius2[:n']."""
    x = as64(taps)
    rows = x[0].shape[0]
    assert 1 <= n <= rows and 0 <= start < rows
    mind = torch.full((rows,), math.inf, dtype=torch.float64)
    sel, radius2, at = [start], [math.inf], {}
    for j in range(n):
        mind = torch.minimum(mind, dist2_to(x, sel[j]))
        mind[sel[j]] = -1.0
        top = float(mind.max())
        if j + 1 in checkpoints:
            at[j + 1] = (mind.clone(), top)
        if j + 1 < n:
            sel.append(int((mind == top).nonzero()[0]))
            radius2.append(top)
    return dict(sel=sel, radius2=torch.tensor(radius2, dtype=torch.float64), cover2=float(mind.max()), mind=mind, at=at)


def replay_check(taps, sel, radius2, start=None, mind=None, cover2=None, exact: bool = False, what: str = "") -> float:
    """Hold a selector's history (sel [n], radius2 [n], optionally its final mind [rows] and cover2) to the rule; AssertionError
    naming the step otherwise.  Every step is checked.  Returns the largest |radius2 - M64| / (gamma M64) seen."""
    x = as64(taps)
    rows, D, T = x[0].shape[0], x[0].shape[1], len(x)
    g = 0.0 if exact else gamma(D, T)
    sel = [int(s) for s in (sel.tolist() if torch.is_tensor(sel) else sel)]
    r2 = [float(r) for r in (radius2.tolist() if torch.is_tensor(radius2) else radius2)]
    n = len(sel)
    assert len(r2) == n and 1 <= n <= rows, f"{what}: {n} selections, {len(r2)} radii, {rows} rows"
    assert start is None or sel[0] == start, f"{what}: sel[0] = {sel[0]}, start = {start}"
    assert r2[0] == math.inf, f"{what}: radius2[0] = {r2[0]}"
    M = torch.full((rows,), math.inf, dtype=torch.float64)
    taken = torch.zeros(rows, dtype=torch.bool)
    worst = 0.0
    for j, s in enumerate(sel):
        assert 0 <= s < rows, f"{what}: step {j} selects row {s} outside 0..{rows - 1}"
        assert not bool(taken[s]), f"{what}: step {j} selects row {s} again"
        d = dist2_to(x, s)
        if j >= 1:
            top, ms = float(M.max()), float(M[s])
            assert ms * (1 + g) >= top * (1 - g), f"{what}: step {j} picks row {s} with mind {ms:.9g}, the maximum is {top:.9g}"
            assert abs(r2[j] - ms) <= g * ms, f"{what}: step {j} radius2 {r2[j]:.9g}, fp64 {ms:.9g}, bound {g * ms:.3g}"
            if ms > 0:
                worst = max(worst, abs(r2[j] - ms) / (g * ms) if g else 0.0)
            twin = ((d == 0) & ~taken)[:s].nonzero()
            assert twin.numel() == 0, f"{what}: step {j} picks row {s}, the identical row {int(twin[0]) if twin.numel() else -1} is lower"
            if exact:
                low = int((M == top).nonzero()[0])
                assert s == low, f"{what}: step {j} picks row {s}, the lowest row of the maximum is {low}"
        M = torch.minimum(M, d)
        M[s] = -1.0
        taken[s] = True
    if mind is not None:
        m = mind.detach().cpu().double()
        assert m.shape == M.shape, f"{what}: mind has shape {tuple(m.shape)}"
        assert bool((m[taken] == -1.0).all()), f"{what}: a selected row's mind is not -1"
        if bool((~taken).any()):
            fb.assert_within(m[~taken], M[~taken], g * M[~taken], f"{what} mind")
    if cover2 is not None:
        c, top = float(cover2), float(M.max())
        assert abs(c - top) <= g * abs(top), f"{what}: cover2 {c:.9g}, fp64 {top:.9g}"
        if mind is not None:
            assert c == float(mind.max()), f"{what}: cover2 {c!r} is not the maximum of mind {float(mind.max())!r}"
    return worst


# --------------------------------------------------------------------------------------------------------------- cases
KNOWN_ROWS = [[1, 0, 0, 0], [1, 0, 0, 0], [0, 2, 0, 0], [0, 2, 0, 0], [0, 0, -2, 0], [1, 0, 0, 0]]
KNOWN_SEL = [0, 2, 4, 1, 3, 5]
KNOWN_RADIUS2 = [math.inf, 5.0, 5.0, 0.0, 0.0, 0.0]


# the coverage case: sized_clusters(COVER_SIZES, 96, 2, seed=5), six centres from start 0, on the fp64 rule (select_ref).  The
# centres are one row of every cluster, the radii distances between clusters, the cover a distance inside the big cluster.
COVER_SIZES = [900, 40, 30, 20, 7, 3]
COVER_SEL = [0, 960, 901, 993, 999, 970]
COVER_RADIUS2 = [4.22087950657442, 3.999510182740778, 3.9238899566162218, 3.7653579095795067, 3.7437986640616145]
COVER_COVER2 = 0.19203696075874177


def int_case(rows: int, D: int, T: int, seed: int):
    """T [rows, D] bf16 matrices of integers in -2..2, about a third as many distinct rows as rows (one row map for all taps, so
    duplicates are duplicates in every tap): each difference is at most 4, each sum at most 16 D T < 2^24, every fp32 operation
    of dist2 is exact and ties are everywhere."""
    assert 16 * D * T < 2 ** 24
    g = torch.Generator().manual_seed(seed)
    u = max(1, rows // 3)
    which = torch.randint(0, u, (rows,), generator=g)
    return [torch.randint(-2, 3, (u, D), generator=g).to(BF16)[which].contiguous() for _ in range(T)]


def unit_case(rows: int, D: int, T: int, seed: int, clusters: int = 0, spread: float = 0.05):
    """T [rows, D] bf16 matrices of unit rows; `clusters` > 0: the rows of every tap scatter around that many directions, row i
    around direction i % clusters in every tap."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(T):
        x = torch.randn(rows, D, generator=g, dtype=torch.float64)
        if clusters:
            c = torch.randn(clusters, D, generator=g, dtype=torch.float64)
            c = c / c.norm(dim=1, keepdim=True)
            x = c[torch.arange(rows) % clusters] + spread * x / math.sqrt(D)
        out.append((x / x.norm(dim=1, keepdim=True)).to(BF16))
    return out


def sized_clusters(sizes, D: int, T: int, seed: int, spread: float = 0.02):
    """Clusters of the given sizes, one after the other (cluster c holds the rows sum(sizes[:c]) ..), unit rows around one random
    direction per cluster and tap plus `spread` times a standard normal per coordinate (the `unit_rows(centre, spread)` of
    tests/test_expert_bank_gpu.py), normalised.  Returns (taps, cluster of row)."""
    g = torch.Generator().manual_seed(seed)
    label = torch.cat([torch.full((s,), c) for c, s in enumerate(sizes)])
    out = []
    for _ in range(T):
        c = torch.randn(len(sizes), D, generator=g, dtype=torch.float64)
        c = c / c.norm(dim=1, keepdim=True)
        x = c[label] + spread * torch.randn(len(label), D, generator=g, dtype=torch.float64)
        out.append((x / x.norm(dim=1, keepdim=True)).to(BF16))
    return out, label
