"""Plain references for the two beam-search entry points of myriad_amd/csrc/beam.hip, and the named inputs the edge tests
(tests/test_beam_edges_cpu.py, tests/test_beam_edges_gpu.py) share.

mh_beam_topk.  Per row, from the f32 inputs in float64: s = bs + ((x - max) - log(sum(exp(x - max)))), the ban applied after
the log-softmax.  A row that holds a NaN or a +inf logit is all -inf (the sum is not a number, and the kernel maps a NaN score
to -inf); a -inf logit adds 0 to the sum and scores -inf; a row whose running score is -inf or NaN is all -inf.  Per item the
order is score descending, flat index (row_in_item * V + token) ascending -- a total order on the float64 keys, evaluated by a
lexicographic sort of (-s64, flat index).  The inputs below are built so that this order is also the one the kernel's fp32
keys have: a random case is decisive (every gap among the first K + 1 ranks exceeds twice the larger of the two bounds;
tests/test_beam_edges_cpu.py asserts it), and an engineered tie is bit-identical logits under one running score, which any
deterministic evaluation maps to equal keys.

The bound a kernel's fp32 score is held to, per element:
    bound = 2^-23 (|x - max| + |log sum| + |bs| + |s64|) + 64 * 2^-24, and 0 where s64 is -inf.
The first term is one ulp (2 u32) of every value the three roundings of bs + ((x - max) - ls) are taken at.  The constant covers
the error of ls = logf(se): se adds up to 32768 exponentials as 32 per thread, 6 shuffle levels and 16 wave partials, 54 fp32
additions on a sum of positive terms (54 u32 relative, absolute in the logarithm), plus 10 ulp for expf and logf.  No
accuracy table of the device library is installed next to the compiler this suite was written against, so the 10 ulp is a
stated allowance (fp64_bounds.C_FN = 4 each for expf and logf, and a margin of 2), not a documented figure.

mh_beam_reorder_kv.  cache[r, p] = old cache[src[r], p] for p in [max(lo, 0), min(hi, T_cap)), every layer; a parent that is
not a row of r's own item leaves row r as it was.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace
from typing import List

import numpy as np
import torch

NINF = float("-inf")
PLACEHOLDER = 0x7FFFFFFF            # what a wave that ran out of candidates ranks with; it must never reach out_i or part_i


# ---------------------------------------------------------------------------------------------------------------- top-K
def topk_ref(logits_f32: torch.Tensor, scores_f32: torch.Tensor, B: int, nb: int, ban_id: int) -> SimpleNamespace:
    """logits_f32 [R, V], scores_f32 [R], R = B * rpi.  Returns s64 and bound [B, rpi * V] (float64), idx [B, K] (int64: the
    item's top K = 2 nb flat indices, best first) and top [B, min(K + 1, rpi * V)] (one rank more, for the decisiveness check)."""
    assert logits_f32.dtype == torch.float32 and scores_f32.dtype == torch.float32
    R, V = logits_f32.shape
    assert R % B == 0
    rpi, K = R // B, 2 * nb
    x = logits_f32.double()
    bs = scores_f32.double()[:, None]
    dead = torch.isnan(x).any(1) | (x == float("inf")).any(1) | (x == NINF).all(1) | torch.isnan(bs[:, 0]) | (bs[:, 0] == NINF)
    xs = torch.where(dead[:, None], torch.zeros_like(x), x)            # a dead row's arithmetic is not looked at
    a = xs - xs.amax(1, keepdim=True)
    ls = torch.exp(a).sum(1, keepdim=True).log()
    s = torch.where(dead[:, None], torch.zeros_like(bs), bs) + (a - ls)
    s[dead] = NINF
    if 0 <= ban_id < V:
        s[:, ban_id] = NINF
    fin = s > NINF
    a0 = torch.where(fin, a, torch.zeros_like(a))
    s0 = torch.where(fin, s, torch.zeros_like(s))
    bound = torch.where(fin, 2.0 ** -23 * (a0.abs() + ls.abs() + bs.abs() + s0.abs()) + 64 * 2.0 ** -24, torch.zeros_like(s))
    s64, bound = s.reshape(B, rpi * V), bound.reshape(B, rpi * V)
    n = min(K + 1, rpi * V)
    top = np.stack([_first_n(s64[b].numpy(), n) for b in range(B)])
    return SimpleNamespace(s64=s64, bound=bound, idx=torch.from_numpy(top[:, :K].copy()), top=torch.from_numpy(top), K=K, rpi=rpi, V=V)


def _first_n(s: np.ndarray, n: int) -> np.ndarray:
    """The first n flat indices of s in (value descending, index ascending)."""
    kth = np.partition(s, s.size - n)[s.size - n]                      # the n-th largest value: everything >= it can rank
    cand = np.nonzero(s >= kth)[0]
    return cand[np.lexsort((cand, -s[cand]))][:n].astype(np.int64)


def check_scores(got: torch.Tensor, s64: torch.Tensor, bound: torch.Tensor, what: str = "") -> float:
    """got (f32) against s64 element by element: exactly -inf where s64 is, within bound elsewhere (NaN fails).  Returns the
    worst error-to-bound ratio."""
    from tests.fp64_bounds import assert_within
    got = got.double().cpu()
    gone = s64 == NINF
    assert bool((got[gone] == NINF).all()), f"{what}: a score whose reference is -inf is not exactly -inf"
    if bool(gone.all()):
        return 0.0
    return assert_within(got[~gone], s64[~gone], bound[~gone], what)


def decisive(ref: SimpleNamespace) -> float:
    """min over items and k of gap(k, k + 1) / (2 max(bound_k, bound_k+1)) among the first K + 1 ranks: > 1 means no
    evaluation within the bound can order them otherwise.  A -inf score is exact (bound 0): a finite score above it is decided,
    and two -inf neighbours are ordered by their indices alone."""
    worst = float("inf")
    for b in range(ref.top.shape[0]):
        s, e = ref.s64[b][ref.top[b]], ref.bound[b][ref.top[b]]
        for k in range(s.numel() - 1):
            if s[k + 1] > NINF:
                worst = min(worst, float((s[k] - s[k + 1]) / (2 * torch.maximum(e[k], e[k + 1]))))
    return worst


# ---------------------------------------------------------------------------------------------------------------- reorder
def reorder_ref(caches: List[torch.Tensor], src, lo: int, hi: int, B: int, nb: int) -> List[torch.Tensor]:
    """New tensors: every [B * nb, T_cap, C] cache with row r's positions [max(lo, 0), min(hi, T_cap)) taken from row src[r] of
    the old cache, when src[r] is a row of r's own item; row r unchanged otherwise."""
    out = []
    for c in caches:
        T_cap = c.shape[1]
        a, z = max(int(lo), 0), min(int(hi), T_cap)
        new = c.clone()
        for r in range(B * nb):
            s, b = int(src[r]), r // nb
            if b * nb <= s < (b + 1) * nb and s != r and a < z:
                new[r, a:z] = c[s, a:z]
        out.append(new)
    return out


# ---------------------------------------------------------------------------------------------------------------- cases
NBS = (1, 3, 5, 7, 8)
VS = (1023, 1024, 1025, 32000, 32767, 32768)          # and 2 * nb: the kernel's smallest row
SEED0 = 4100
SEED_BUMP = {}                                        # case name -> seed offset, where the first seed is not decisive
TIE_V = 2500
# token j sits in thread j % 1024, register j / 1024, wave (j % 1024) / 64: 5 | 7 two lanes of wave 0; 5 | 69 and 69 | 133 one
# lane in neighbouring waves; 5 | 1029, 7 | 1031, 69 | 1093 one thread's next register; 1023 | 1024 and 2047 | 2048 the last
# thread's register i and the first thread's register i + 1; 300..302 neighbours; token 0 and token V - 1
TIE_TOKENS = (0, 5, 7, 69, 133, 300, 301, 302, 1023, 1024, 1029, 1031, 1093, 1500, 2047, 2048, 2053, 2100, TIE_V - 1)


def _case(name, kind, logits, scores, B, nb, ban=-1, want=None, part_want=None, bit_equal=(), exact_s=None, decisive=False,
          twin=None):
    """want [B, K]: the hand-written flat indices; part_want {row: K tokens}; bit_equal [(item, k0, k1)]: out_s[item, k0:k1] are
    one bit pattern; exact_s [B, K]: hand-derived fp32 scores; decisive: asserted by the CPU test; twin: the name of a case with
    the same answer."""
    return SimpleNamespace(name=name, kind=kind, logits=logits.contiguous(), scores=scores.contiguous(), B=B, nb=nb, K=2 * nb,
                           rpi=logits.shape[0] // B, V=logits.shape[1], ban=ban,
                           want=None if want is None else np.asarray(want, dtype=np.int64).reshape(B, 2 * nb),
                           part_want=part_want or {}, bit_equal=tuple(bit_equal), exact_s=exact_s, decisive=decisive, twin=twin)


def seed_of(name: str) -> int:
    """A case's seed: SEED0 plus a checksum of its name, plus its entry in SEED_BUMP."""
    return SEED0 + sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100000 + SEED_BUMP.get(name, 0)


def _rand(name, R, V, scale=3.0):
    g = torch.Generator().manual_seed(seed_of(name))
    return torch.randn(R, V, generator=g) * scale, -torch.rand(R, generator=g) * 5.0


def _tie_item(name, nb, V, groups):
    """B = 2, rpi = nb: the tie row is the item's last row in item 0 and its first in item 1, score -1.25; the item's other
    rows are random under a score of -50 and never rank.  groups = [(value, tokens)], values above every other logit (<= 2)."""
    K = 2 * nb
    x, _ = _rand(name, 2 * nb, V, scale=1.0)
    x.clamp_(max=2.0)
    sc = torch.full((2 * nb,), -50.0)
    rows = (nb - 1, nb)                                                # global rows; in-item rows nb - 1 and 0
    toks, eq, k0 = [], [], 0
    for val, tk in groups:
        take = sorted(tk)[:K - k0]
        toks += take
        eq.append((k0, k0 + len(take)))
        k0 += len(take)
    assert len(toks) == K
    for r in rows:
        sc[r] = -1.25
        for val, tk in groups:
            x[r, list(tk)] = val
    want = [[(nb - 1) * V + t for t in toks], toks]
    return _case(name, "tie", x, sc, 2, nb, want=want, part_want={rows[0]: toks, rows[1]: toks},
                 bit_equal=[(b, a, z) for b in (0, 1) for a, z in eq])


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = []
    # ---- accuracy and order: random, decisive
    for nb in NBS:
        for B in (1, 3):
            for rpi in sorted({nb, 1}):
                for V in (2 * nb,) + VS:
                    name = f"rand-nb{nb}-B{B}-rpi{rpi}-V{V}"
                    x, sc = _rand(name, B * rpi, V)
                    out.append(_case(name, "rand", x, sc, B, nb, ban=(2 if V > 2 * nb else -1), decisive=True))
    # ---- ties inside a row
    for nb in NBS:
        K = 2 * nb
        out.append(_tie_item(f"tie-pairs-nb{nb}", nb, TIE_V, [(9.0, TIE_TOKENS)]))
        out.append(_tie_item(f"tie-one-wave-nb{nb}", nb, TIE_V, [(9.0, tuple(range(64, 64 + K + 3)) + (2000,))]))
    for nb in (3, 8):
        out.append(_tie_item(f"tie-one-thread-nb{nb}", nb, 32768, [(9.0, tuple(64 + 1024 * i for i in range(32)))]))
        g1 = (TIE_V - 1, 1024, 0)
        out.append(_tie_item(f"tie-two-groups-nb{nb}", nb, TIE_V, [(9.0, g1), (8.0, tuple(t for t in TIE_TOKENS if t not in g1))]))
    for nb in (5, 8):
        every = tuple(w * 64 + 3 for w in range(16))
        out.append(_tie_item(f"tie-every-wave-nb{nb}", nb, TIE_V, [(9.0, every + tuple(t + 1024 for t in every))]))
    # ---- a constant row, one row per item
    for nb in (1, 3, 8):
        K = 2 * nb
        for ban in (-1, 0, 3):
            toks = [t for t in range(K + 1) if t != ban][:K]
            out.append(_case(f"const-nb{nb}-ban{ban}", "const", torch.full((1, 1500), 0.25), torch.tensor([-1.0]), 1, nb, ban=ban,
                             want=toks, part_want={0: toks}, bit_equal=[(0, 0, K)]))
    # ---- ties across the rows of an item.  A running score of -100 keeps bs + lp inside [-128, -64) for every lp in (-28, 0],
    # the binade of bs itself: one ulp of bs survives the sum's rounding whatever lp's own rounding was
    V = 1025
    up = float(np.nextafter(np.float32(-100.0), np.float32(0.0)))
    for nb in (3, 5, 7, 8):
        K = 2 * nb
        flat = torch.full((2 * nb, V), 0.25)
        sc = torch.full((2 * nb,), -100.0)
        out.append(_case(f"rows-const-equal-nb{nb}", "rows", flat, sc, 2, nb, want=[list(range(K))] * 2, bit_equal=[(0, 0, K), (1, 0, K)]))
        sc2 = sc.clone()
        sc2[2], sc2[nb + 2] = up, up
        out.append(_case(f"rows-const-ulp-nb{nb}", "rows", flat, sc2, 2, nb, want=[[2 * V + t for t in range(K)]] * 2,
                         bit_equal=[(0, 0, K), (1, 0, K)]))
        same, _ = _rand(f"rows-same-nb{nb}", 1, V, scale=0.5)
        same.clamp_(max=1.5)
        same[0, 700], same[0, 64] = 9.0, 8.5                          # the row's best two, half a nat apart
        same = same.repeat(2 * nb, 1)
        order = list(range(nb))
        out.append(_case(f"rows-same-equal-nb{nb}", "rows", same, sc, 2, nb,
                         want=[[r * V + t for t in (700, 64) for r in order]] * 2,
                         bit_equal=[(b, a, a + nb) for b in (0, 1) for a in (0, nb)]))
        first2 = [2] + [r for r in order if r != 2]
        out.append(_case(f"rows-same-ulp-nb{nb}", "rows", same, sc2, 2, nb,
                         want=[[r * V + t for t in (700, 64) for r in first2]] * 2,
                         bit_equal=[(b, a + 1, a + nb) for b in (0, 1) for a in (0, nb)]))
        # HF's parked beams: the ulp of fp32 at 1e9 is 64, so -1e9 - log(1025) rounds back to -1e9 and -1e9 + 64 - log(1025)
        # to -1e9 + 64 -- every score of a row is the row's running score
        park = torch.full((2 * nb,), -1e9)
        out.append(_case(f"rows-parked-nb{nb}", "rows", flat, park, 2, nb, want=[list(range(K))] * 2,
                         exact_s=np.full((2, K), -1e9, dtype=np.float32)))
        park2 = park.clone()
        park2[nb - 1], park2[2 * nb - 1] = -1e9 + 64, -1e9 + 64
        out.append(_case(f"rows-parked-one-nb{nb}", "rows", flat, park2, 2, nb, want=[[(nb - 1) * V + t for t in range(K)]] * 2,
                         exact_s=np.full((2, K), np.float32(-1e9) + np.float32(64), dtype=np.float32)))
    # ---- non-finite
    x = torch.full((1, 1025), NINF)
    x[0, 1024], x[0, 3], x[0, 700], x[0, 64] = 2.0, 1.0, 3.0, 0.5
    toks = [700, 1024, 3, 64, 0, 1, 2, 4, 5, 6]
    out.append(_case("few-finite-nb5", "nonfinite", x, torch.tensor([-0.5]), 1, 5, want=toks, part_want={0: toks}))
    x = torch.full((1, 16), NINF)
    x[0, 15], x[0, 0] = 1.0, 2.0
    toks = [0, 15] + list(range(1, 15))
    out.append(_case("few-finite-nb8-V16", "nonfinite", x, torch.tensor([0.0]), 1, 8, want=toks, part_want={0: toks}))
    for nb in (3, 8):
        base, sc = _rand(f"row1-nb{nb}", 2 * nb, 1025)
        off = sc.clone()
        off[1], off[nb + 1] = NINF, NINF
        twin = f"score-ninf-row1-nb{nb}"
        out.append(_case(twin, "nonfinite", base, off, 2, nb, decisive=True))
        for what, val in (("nan", float("nan")), ("pinf", float("inf"))):
            bad = base.clone()
            bad[1, 77], bad[nb + 1, 0] = val, val
            out.append(_case(f"{what}-row1-nb{nb}", "nonfinite", bad, sc, 2, nb, decisive=True, twin=twin))
    # ---- the ban
    x, sc = _rand("ban", 6, 1025)
    x[:, 411] = 20.0                                                   # every row's arg-max
    out.append(_case("ban-argmax", "ban", x, sc, 2, 3, ban=411, decisive=True))
    out.append(_case("ban-none", "ban", x, sc, 2, 3, ban=-1, decisive=True))
    for ban in (1025, 1030):
        out.append(_case(f"ban-{ban}", "ban", x, sc, 2, 3, ban=ban, decisive=True, twin="ban-none"))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case(name: str) -> SimpleNamespace:
    return next(c for c in cases() if c.name == name)


def names(*kinds) -> list:
    return [c.name for c in cases() if not kinds or c.kind in kinds]


@functools.lru_cache(maxsize=None)
def ref(name: str) -> SimpleNamespace:
    """topk_ref of a case, computed once and shared; treat it as read-only."""
    c = case(name)
    return topk_ref(c.logits, c.scores, c.B, c.nb, c.ban)
