"""The rows of the sampler's edge suite, built on the CPU: tests/test_sampling_edges_gpu.py runs them through mh_sample_rows and
its slot form, tests/test_sampling_edges_cpu.py shows that they tell tests/sampling_ref.py from its plausible mis-statements.
A Launch is one call of the uniform entry: R rows of one width under one set of knobs, row r drawing with Philox (seed, t, r).
`expect[r]` = (kept, out) where the answer follows from the row alone in exact arithmetic (asserted whatever the reference's
`near` flag says); every other row is compared with sample_row and was built so that its flag stays down, the tie grid aside."""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from tests import sampling_ref as S

SEED = 0x1234_5678_9ABC_DEF1
NINF, INF = float("-inf"), float("inf")
POS_NAN, NEG_NAN = 0x7FC00000, 0xFFC00000            # the quiet NaN with the sign bit clear / set
# Philox seeds whose (t = 0, row 0) uniform lies next to 0 and next to 1, found by a vectorised host search over SEED + [0, 2^23)
LOW_SEEDS = ((0x1234_5678_9ACE_751E, 0.0), (0x1234_5678_9AC7_177D, 2.0 ** -22))
HIGH_SEEDS = ((0x1234_5678_9AC7_71E6, 1.0 - 2.0 ** -24), (0x1234_5678_9AD3_E90D, 1.0 - 2.0 ** -23))
BAN = 7


@dataclass
class Launch:
    name: str
    x: torch.Tensor                 # [R, V] f32 on the CPU
    top_k: int
    top_p: float
    inv_temp: float = 1.0
    ban: int = -1
    seed: int = SEED
    t: int = 0
    expect: Optional[list] = None   # per row (kept, out) or None
    clean: Optional[torch.Tensor] = None     # the same rows with every NaN written as -inf (what a NaN row must equal)
    _ref: Optional[list] = field(default=None, repr=False)

    @property
    def R(self) -> int:
        return self.x.shape[0]

    @property
    def V(self) -> int:
        return self.x.shape[1]

    def u(self, r: int) -> float:
        return S.uniform(self.seed, self.t, r)

    def ref(self) -> list:
        """sample_row per row, computed once and shared by the tests."""
        if self._ref is None:
            self._ref = [S.sample_row(self.x[r], self.top_k, self.top_p, self.inv_temp, self.ban, u=self.u(r)) for r in range(self.R)]
        return self._ref


def f32_bits(bits) -> torch.Tensor:
    """float32 tensor from explicit bit patterns (through an int32 view, so a NaN keeps its sign and payload)."""
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.int32).copy()).view(torch.float32)


def nan(sign_set: bool) -> torch.Tensor:
    return f32_bits([NEG_NAN if sign_set else POS_NAN])[0]


def seed_where(x, top_k, top_p, inv_temp, ban, start, want=None, t=0):
    """The first seed >= start whose row-0 draw at step t is not `near` on row x (and picks id `want`, when given)."""
    for s in range(start, start + 4096):
        r = S.sample_row(x, top_k, top_p, inv_temp, ban, u=S.uniform(s, t, 0))
        if not r["near"] and (want is None or r["out"] == want):
            return s
    raise AssertionError("no such seed within 4096 tries")


# ------------------------------------------------------------------------------------------------ 1. the tie grid
TIE_V = (1, 2, 3, 5, 63, 64, 65, 4095, 4096, 4097, 32765, 32767, 32768)
TIE_ROWS = 3


@functools.lru_cache(maxsize=None)
def tie_grid() -> List[Launch]:
    """Quantised logits round(randn * 3 / step) * step, so the k-th value is tied in most rows: 13 widths x 4 top_k x 4 top_p x 2
    steps, 3 rows each.  T cycles over (0.7, 1.0, 1.3); the ban (the last id) is on in every other launch, shifted by one from one
    top_k to the next so that it meets every top_p and both steps."""
    g = torch.Generator().manual_seed(11)
    out = []
    for n, (V, top_k, top_p, step) in enumerate(itertools.product(TIE_V, (1, 2, 50, 1024), (0.01, 0.5, 0.9, 1.0), (0.25, 1.0 / 64))):
        T = (0.7, 1.0, 1.3)[n % 3]
        ban = V - 1 if (n + n // 8) % 2 else -1
        x = torch.round(torch.randn(TIE_ROWS, V, generator=g) * 3.0 / step) * step
        out.append(Launch(f"tie_V{V}_k{top_k}_p{top_p}_s{step:g}", x, top_k, top_p, 1.0 / T, ban, SEED + n, n % 7 + 1))
    return out


# ------------------------------------------------------------------------------------------------ 2. sort padding and the cap
PAD_V, PAD_N = 2048, (1, 2, 3, 511, 512, 513, 1023, 1024)


def _ramp(V, perm_seed):
    """Distinct logits -i / 256 (exact in fp32; 1024 of them span e^-4, so every candidate carries mass) permuted over the ids;
    (row, ids by rank)."""
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(perm_seed))
    x = torch.empty(V)
    x[perm] = -torch.arange(V, dtype=torch.float32) / 256.0
    return x, perm


@functools.lru_cache(maxsize=None)
def pad_cases() -> List[Launch]:
    out = []
    for n in PAD_N:
        x, perm = _ramp(PAD_V, n)
        out.append(Launch(f"pad_n{n}", x[None], n, 1.0, seed=seed_where(x, n, 1.0, 1.0, -1, SEED + 100 * n)))
        # u next to 1 takes the last candidate: cum[n - 2] is a whole p_last >= e^-4 below the total, u * total 2^-20 of it at most
        out.append(Launch(f"pad_n{n}_u_high", x[None], n, 1.0, seed=HIGH_SEEDS[0][0], expect=[(n, int(perm[n - 1]))]))
        out.append(Launch(f"pad_n{n}_u_low", x[None], n, 1.0, seed=LOW_SEEDS[0][0], expect=[(n, int(perm[0]))]))
    x, perm = _ramp(PAD_V, 77)
    x[perm[1024]] = x[perm[1023]]                                     # one more value tied at rank 1024: 1025 candidates
    for top_p in (1.0, 0.5):
        out.append(Launch(f"pad_tie_1025_p{top_p}", x[None], 1024, top_p, expect=[(-1, int(perm[0]))]))
    x3 = torch.tensor([0.5, 2.0, -1.0])
    out.append(Launch("pad_k5_V3", x3[None], 5, 1.0, seed=seed_where(x3, 5, 1.0, 1.0, -1, SEED + 5)))
    return out


# ------------------------------------------------------------------------------------------------ 3. signed zeros
ZERO_ROWS = dict(plus_first=f32_bits([0x3F800000, 0x00000000, 0x80000000, 0x80000000, 0xBF800000, 0x00000000, 0xC0000000, 0xC0400000]),
                 minus_first=f32_bits([0x3F800000, 0x80000000, 0x00000000, 0x00000000, 0xBF800000, 0x80000000, 0xC0000000, 0xC0400000]))
# (V, where the 8 values start): alone; ending in the one-element last float4 of V = 4097; ids 252..259, which threads 63 and 64
# hold, the last lane of wave 0 and the first of wave 1
ZERO_PLACES = ((8, 0), (4097, 4089), (300, 252))


@functools.lru_cache(maxsize=None)
def zero_cases() -> List[Launch]:
    """[1, 0, -0, -0, -1, 0, -2, -3] (and the same with the zeros' signs swapped) over a floor of -10: with top_k 2 or 3 the k-th
    value is a zero, so ids 0, 1, 2, 3, 5 stay, in that order.  top_p = 1: one seed for each of ids 2, 3 and 5, so u lands in
    the mass of a zero of either sign behind the first; top_p = 0.5 keeps ids 0 and 1 (exclusive mass 1 < 0.5 * (1 + 4 / e)
    = 1.236 < 1 + 1 / e), one seed for each."""
    out = []
    for (V, at), (zname, z), top_k, top_p in itertools.product(ZERO_PLACES, ZERO_ROWS.items(), (2, 3), (1.0, 0.5)):
        x = torch.full((V,), -10.0)
        x[at:at + 8] = z
        for want in ((2, 3, 5) if top_p == 1.0 else (0, 1)):
            s = seed_where(x, top_k, top_p, 1.0, -1, SEED + 1000 * want + V, want=at + want)
            out.append(Launch(f"zero_{zname}_V{V}_k{top_k}_p{top_p}_id{want}", x[None], top_k, top_p, seed=s,
                              expect=[(5 if top_p == 1.0 else 2, at + want)]))
    return out


# ------------------------------------------------------------------------------------------------ 4. NaN and inf rows
@functools.lru_cache(maxsize=None)
def nonfinite_cases() -> List[Launch]:
    """V = 37 (below a wave) and 4097; top_k = 5, top_p 0.9 and 1.0.  A NaN row must give what the same row with -inf in the NaN's
    place gives (`clean`); the +inf and nothing-finite rows have the contract's answers (`expect`)."""
    out = []
    for V in (37, 4097):
        base = torch.randn(V, generator=torch.Generator().manual_seed(V + 1)) * 3.0
        top = int(torch.argmax(base))
        assert top not in (0, BAN, V - 1, 5, 11)
        rows = []                                                     # (name, row, ban, expect)
        for sname, sign in (("pos", False), ("neg", True)):
            for where, at, ban in (("id0", 0, -1), ("last", V - 1, -1), ("argmax", top, -1), ("banned", BAN, BAN)):
                x = base.clone()
                x[at] = nan(sign)
                rows.append((f"nan_{sname}_{where}", x, ban, None))
        x = torch.empty(V)
        x[0::2], x[1::2] = nan(False), nan(True)
        rows.append(("all_nan", x, -1, (-1, 0)))
        rows.append(("all_ninf", torch.full((V,), NINF), -1, (-1, 0)))
        x = torch.full((V,), NINF)
        x[BAN] = 2.0
        rows.append(("ninf_but_the_banned", x, BAN, (-1, 0)))
        x = base.clone()
        x[11] = INF
        rows.append(("one_pinf", x, -1, (1, 11)))
        x = base.clone()
        x[11] = x[5] = INF
        rows.append(("two_pinf", x, -1, (1, 5)))
        x = base.clone()
        x[11], x[3] = INF, nan(False)
        rows.append(("pinf_behind_a_nan", x, -1, (1, 11)))
        x = base.clone()
        x[BAN] = INF
        rows.append(("pinf_on_the_banned", x, BAN, None))
        for (name, x, ban, expect), top_p in itertools.product(rows, (0.9, 1.0)):
            clean = torch.where(torch.isnan(x), torch.full_like(x, NINF), x)
            s = SEED + V if expect is not None else seed_where(clean, 5, top_p, 1.0, ban, SEED + V)
            out.append(Launch(f"{name}_V{V}_p{top_p}", x[None], 5, top_p, ban=ban, seed=s, expect=expect and [expect],
                              clean=clean[None]))
    return out


# ------------------------------------------------------------------------------------------------ 5. extreme knobs
@functools.lru_cache(maxsize=None)
def knob_cases() -> List[Launch]:
    out = []
    V = 1000
    x = torch.randn(3, V, generator=torch.Generator().manual_seed(5)) * 3.0
    top = [int(i) for i in torch.argmax(x, 1)]
    out.append(Launch("top_p_0", x, 50, 0.0, seed=SEED + 1, t=2, expect=[(1, i) for i in top]))
    for name, top_p, inv_temp in (("top_p_1.5", 1.5, 1.0), ("inv_temp_20", 0.9, 20.0), ("inv_temp_0.05", 0.9, 0.05)):
        for r in range(3):
            s = seed_where(x[r], 50, top_p, inv_temp, -1, SEED + 10 * r)
            out.append(Launch(f"{name}_row{r}", x[r:r + 1], 50, top_p, inv_temp, seed=s))
    # finite logits that the temperature pushes to +inf count as +inf: the lowest such id alone (the arg-max is id 1)
    hot = torch.tensor([1.0e38, 3.0e38, 0.0, -1.0, 2.0e38, 5.0, 1.0e30, -3.0e38])
    for top_p in (0.9, 1.0):
        out.append(Launch(f"tempered_to_inf_p{top_p}", hot[None], 50, top_p, 20.0, seed=SEED + 3, expect=[(1, 0)]))
    # u next to 0 and next to 1.  Peaked: one logit 20 above the rest, whose whole mass (e^-20 / (1 - e^-1/4) = 9e-9) is below
    # half an ulp of 1, so every fp32 prefix sum is 1, and below 2^-24, the least distance of u from 1: every u takes the arg-max.
    # Flat: equal logits, every mass 1, every sum and top_p * total an integer, so the arithmetic is exact and the cut and the
    # pick are known
    peaked = -20.0 - torch.arange(65, dtype=torch.float32) / 4.0
    peaked[13] = 0.0
    for (s, u), top_p in itertools.product(LOW_SEEDS + HIGH_SEEDS, (1.0, 0.9)):
        out.append(Launch(f"peaked_u{u:.8f}_p{top_p}", peaked[None], 50, top_p, seed=s, expect=[(50 if top_p == 1.0 else 1, 13)]))
    for V in (8, 1024):
        flat = torch.full((V,), 1.5)
        for (s, u), top_p in itertools.product(LOW_SEEDS + HIGH_SEEDS, (1.0, 0.5)):
            kept = V if top_p == 1.0 else V // 2
            out.append(Launch(f"flat{V}_u{u:.8f}_p{top_p}", flat[None], V, top_p, seed=s, expect=[(kept, 0 if u < 0.5 else kept - 1)]))
    return out


def direct_cases() -> List[Launch]:
    """The launches of tests 2 to 5."""
    return pad_cases() + zero_cases() + nonfinite_cases() + knob_cases()


def tie_grid_counts():
    """(compared, near, overflow) rows of the tie grid by the reference alone."""
    near = over = rows = 0
    for c in tie_grid():
        for r in c.ref():
            rows += 1
            if r["kept"] == -1:
                over += 1
            elif r["near"]:
                near += 1
    return rows - near - over, near, over
