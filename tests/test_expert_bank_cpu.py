"""The vision expert's reference bank without a GPU: the bookkeeping class, the fp64 restatement of the banked one-shot head
(tests/bank_ref.py) against the oracle and the committed goldens, and proof that the restatement's bounds reject each plausible
kernel mistake -- an fp32 emulation of bank_sim_max + bank_sim_finish with the mistake built in, on inputs made for it."""
import numpy as np
import pytest
import torch

from myriad_amd.expert_bank import BankIndex
from oracle import expert_ref as X
from tests import bank_ref as br
from tests import fp64_bounds as fb
from tests.test_expert_oracle import load_case
from tests.test_fp64_bounds_cpu import emu_bilinear

F32 = torch.float32
CHUNK = 128                 # bank rows per chunk of bank_sim_max (BK_CH; tests/test_expert_bank_gpu.py checks the library's value)


# --------------------------------------------------------------------------------------------------------- bookkeeping
def _consistent(ix: BankIndex, want):
    assert ix.names() == [n for n, _ in want] and len(ix) == len(want)
    off = 0
    for n, r in want:
        assert ix.lookup(n) == (off, r) and n in ix
        off += r
    assert ix.total == off


def test_bank_index_add_replace_drop_keep_offsets_contiguous():
    ix = BankIndex()
    assert ix.names() == [] and ix.total == 0
    assert ix.append("bottle", 256) == 0
    assert ix.append("cable", 1024) == 256
    assert ix.append("pcb1", 17) == 1280
    _consistent(ix, [("bottle", 256), ("cable", 1024), ("pcb1", 17)])
    # a tensor of row labels goes through the same cuts the expert applies to its bank tensors
    rows = torch.cat([torch.full((r,), i) for i, r in enumerate((256, 1024, 17))])
    off, n = ix.remove("cable")                                       # replacement = remove + append behind the last class
    assert (off, n) == (256, 1024)
    rows = torch.cat([rows[:off], rows[off + n:], torch.full((512,), 3)])
    assert ix.append("cable", 512) == 273
    _consistent(ix, [("bottle", 256), ("pcb1", 17), ("cable", 512)])
    for name, label in (("bottle", 0), ("pcb1", 2), ("cable", 3)):
        o, r = ix.lookup(name)
        assert bool((rows[o:o + r] == label).all()) and rows.numel() == ix.total
    assert ix.remove("bottle") == (0, 256)
    _consistent(ix, [("pcb1", 17), ("cable", 512)])
    assert ix.remove("cable") == (17, 512) and ix.remove("pcb1") == (0, 17)
    _consistent(ix, [])


def test_bank_index_errors_name_the_class():
    ix = BankIndex()
    ix.append("bottle", 4)
    with pytest.raises(KeyError, match="zipper"):
        ix.lookup("zipper")
    with pytest.raises(KeyError, match="zipper"):
        ix.remove("zipper")
    with pytest.raises(ValueError, match="bottle"):
        ix.append("bottle", 4)
    with pytest.raises(ValueError):
        ix.append("empty", 0)
    _consistent(ix, [("bottle", 4)])


# ------------------------------------------------------------------------------ the restatement against oracle and goldens
@pytest.fixture(scope="module")
def k2_case():
    torch.set_num_threads(8)
    g, cfg, sd, images, refs, _ = load_case("d1280_1blk_k2")
    _, qt = X.vision_trunk(sd, images, cfg["heads"], cfg["layers"], cfg["blocks"])
    _, rt = X.vision_trunk(sd, refs, cfg["heads"], cfg["layers"], cfg["blocks"])
    return g, cfg, qt, rt


def test_restatement_agrees_with_oracle_and_golden(k2_case):
    """Each sample's bank is its own k references (un-rounded fp64 unit rows: the oracle's cosine similarity, not bf16)."""
    g, cfg, qt, rt = k2_case
    B, k = cfg["B"], cfg["k"]
    N = qt[0].shape[1]
    L = N - 1
    q_taps = [br.normalise_rows(t).reshape(B * N, -1) for t in qt]
    bank_taps = [br.patch_rows(br.normalise_rows(t)) for t in rt]                # reference-major: sample b's rows at b k L
    ranges = [(b * k * L, k * L) for b in range(B)]
    ref = br.head_ref_bound(q_taps, bank_taps, ranges, L, 224, q_row0=1, q_sample_rows=N)
    omap, omask = X.one_shot_maps(qt, rt)
    for got, want, gold in ((ref["amap"][0], omap, g["os_map"]), (ref["simmask"][0], omask, g["os_mask"])):
        np.testing.assert_allclose(got.reshape(want.shape).numpy(), want.double().numpy(), atol=2e-5)
        np.testing.assert_allclose(got.reshape(gold.shape).numpy(), gold, atol=2e-5)


# ------------------------------------------------------------------------------------- fp32 emulation of the two kernels
def emu_head(q_taps, bank_taps, ranges, L, S, q_row0, q_sample_rows, mutant=None):
    """bank_sim_max per tap (scores = the fp64 dot rounded to fp32: inside the accumulation bound), chunk maxima over 16-row
    tiles with tail rows masked, then bank_sim_finish in fp32."""
    T, B = len(q_taps), len(ranges)
    w = torch.tensor(1.0 / (T + 1 if mutant == "wrong_weight" else T), dtype=F32)
    h = int(round(L ** 0.5))
    sim = torch.zeros(B, L, dtype=F32)
    for q, bank in zip(q_taps, bank_taps):
        for b in range(B):
            off, rows = ranges[0] if mutant == "range_of_sample_0" else ranges[b]
            if mutant == "next_class":
                off = off + rows
            lo, hi = off, off + rows
            lo += {"lo_minus": -1, "lo_plus": 1}.get(mutant, 0)
            hi += {"hi_minus": -1, "hi_plus": 1}.get(mutant, 0)
            r0 = b * q_sample_rows + (0 if mutant == "class_token_included" else q_row0)
            if hi <= lo:                                                     # a one-row class cut to nothing: max of no score
                sim[b] += w * torch.full((L,), float("-inf"))
                continue
            s = (q[r0:r0 + L].double() @ bank[lo:hi].double().T).float()
            pad = -(hi - lo) % 16                                            # rows of the last 16-row tile past the class
            fill = 0.0 if mutant == "zero_tail" else float("-inf")
            s = torch.cat([s, torch.full((L, pad), fill, dtype=F32)], dim=1)
            part = torch.stack([s[:, c:c + CHUNK].amax(dim=1) for c in range(0, s.shape[1], CHUNK)])
            m = part[-1] if mutant == "last_chunk_only" else part.amax(dim=0)
            sim[b] += w * m
    sim = sim.view(B, h, h)
    return sim, emu_bilinear(sim, h, h, one_minus=True), emu_bilinear(sim, S, S, one_minus=True)


def _trap_case(seed=11):
    """B = 3 samples of L = 16 patches (N = 17 with the class token), D = 32, T = 2 taps, S = 24.  Bank layout, with a trap
    block (a copy of all B N query rows: cosine 1 with their own query, about 0.8 with every other) before, between and behind
    the classes:
        trap | class A: 201 rows (two chunks, last 16-row tile 9 full) | trap | class B: 17 rows | trap | class C: 1 row | trap
    Query (b, l) is base + 0.5 e_l (e_l orthonormal, orthogonal to base; l = 16 the class token); an own row is -base + noise,
    so every own cosine is negative (about -0.78), except three designated rows -base + 1.5 e_l whose cosine with patch l is
    about -0.12: the class's first row for patch 0, its last row for patch 1 and, in class A, row 5 of the first chunk for
    patch 2.  Any row outside a range therefore wins by O(1), a dropped first or last row loses by O(0.1)."""
    B, L, N, D, T, S = 3, 16, 17, 32, 2, 24
    counts = (201, 17, 1)
    q_taps, bank_taps = [], []
    for t in range(T):
        g = torch.Generator().manual_seed(seed + t)
        basis = torch.linalg.qr(torch.randn(D, D, generator=g, dtype=torch.float64))[0].T      # orthonormal rows
        base, e = basis[0], basis[1:1 + N]
        order = [L] + list(range(L))                                       # token row 0 is the class token (direction e_16)
        q = torch.cat([base[None] + 0.5 * e[order] for _ in range(B)]) + 0.02 * torch.randn(B * N, D, generator=g, dtype=torch.float64)
        q = fb.bf16_round((q / q.norm(dim=-1, keepdim=True)).float())
        blocks = [q.clone()]
        for r in counts:
            own = -base[None] + 0.1 * torch.randn(r, D, generator=g, dtype=torch.float64)
            if r > 5:
                own[5] = -base + 1.5 * e[2]
            own[-1] = -base + 1.5 * e[1]
            own[0] = -base + 1.5 * e[0] if r > 1 else -base + 1.5 * (e[0] + e[1]) / 2 ** 0.5
            blocks += [fb.bf16_round((own / own.norm(dim=-1, keepdim=True)).float()), q.clone()]
        q_taps.append(q)
        bank_taps.append(torch.cat(blocks, dim=0))
    trap = B * N
    ranges, off = [], trap
    for r in counts:
        ranges.append((off, r))
        off += r + trap
    return q_taps, bank_taps, ranges, L, S, 1, N


def _check(mutant=None, case=None):
    q_taps, bank_taps, ranges, L, S, q_row0, qsr = case or _trap_case()
    ref = br.head_ref_bound(q_taps, bank_taps, ranges, L, S, q_row0=q_row0, q_sample_rows=qsr)
    sim, simmask, amap = emu_head(q_taps, bank_taps, ranges, L, S, q_row0, qsr, mutant)
    return br.check_head(sim, simmask, amap, ref, f"emulation[{mutant}]")


def test_emulation_is_within_the_bounds_and_every_cosine_is_negative():
    q_taps, bank_taps, ranges, L, S, q_row0, qsr = _trap_case()
    for q, bank in zip(q_taps, bank_taps):
        m, _ = br.tap_max_ref_bound(q, bank, ranges, L, q_row0, qsr)
        assert float(m.max()) < -0.05                                  # a zero from padding would beat every true score
    assert _check() <= 1.0


MUTANTS = ["zero_tail", "class_token_included", "lo_minus", "lo_plus", "hi_minus", "hi_plus", "next_class", "range_of_sample_0",
           "last_chunk_only", "wrong_weight"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_bounds_catch_the_kernel_mistake(mutant):
    with pytest.raises(AssertionError, match="out of bound"):
        _check(mutant)


def test_chunk_reference_splits_as_the_kernel_does():
    """chunk_max_ref_bound: per-chunk maxima whose max is the whole-range value, one entry per ceil(rows / chunk)."""
    q_taps, bank_taps, ranges, L, S, q_row0, qsr = _trap_case()
    whole, _ = br.tap_max_ref_bound(q_taps[0], bank_taps[0], ranges, L, q_row0, qsr)
    per = br.chunk_max_ref_bound(q_taps[0], bank_taps[0], ranges, L, CHUNK, q_row0, qsr)
    assert [m.shape[0] for m, _ in per] == [2, 1, 1]
    for b, (m, _) in enumerate(per):
        assert torch.equal(m.amax(dim=0), whole[b])
