"""fp64 restatement of the banked one-shot head (csrc/expert_bank.hip: bank_sim_max + bank_sim_finish) with per-element bounds
built from the rounding rules of tests/fp64_bounds.py.  Nothing here is measured on the kernels.

  per tap    P, E = gemm_ref_bound(q_b, bank[off_b : off_b + rows_b]) on the operands as given (the bf16 values the kernel reads):
             value max_j P[:, j], bound max_j E[:, j], because |max x - max y| <= max |x - y|.  A max over chunks of partial maxima
             is the same number: max is exact and associative.
  sim        sum_t w m_t with w = fl32(1 / T): the per-tap bounds times |w|, plus (T + 2) u32 of sum_t |w m_t| for the T products
             and the additions of the accumulator (rowmax_skip's acc += w * max, fused or not).
  simmask    1 - sim: one more u32 of the result.
  amap       1 - bilinear_ac(sim): the bound of the existing bilinear_ac tests (fp64_bounds.bilinear_ref_bound, one_minus) at the
             fp64 sim, plus the sim bound carried through the interpolation, which is a convex combination of four inputs
             (weights rounded: (1 + 8 u32) of the interpolated bound).
"""
import torch

from tests import fp64_bounds as fb

U32 = fb.U32


def normalise_rows(x: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    """x / max(||x||, eps) along the last axis in fp64 (F.cosine_similarity's operands)."""
    x = x.double()
    return x / x.norm(dim=-1, keepdim=True).clamp_min(eps)


def patch_rows(taps_normed: torch.Tensor) -> torch.Tensor:
    """[k, 1 + L, D] rows of k references -> the bank's [k L, D]: class-token rows dropped, reference-major."""
    k, N, D = taps_normed.shape
    return taps_normed[:, 1:].reshape(k * (N - 1), D)


def query_rows(q: torch.Tensor, b: int, L: int, q_row0: int, q_sample_rows: int) -> torch.Tensor:
    r = b * q_sample_rows + q_row0
    return q[r:r + L]


def tap_max_ref_bound(q, bank, ranges, L, q_row0=0, q_sample_rows=None):
    """(m [B, L], e [B, L]) fp64: m[b, l] = max_j <q[b, l], bank[off_b + j]>, j < rows_b."""
    q_sample_rows = q_row0 + L if q_sample_rows is None else q_sample_rows
    ms, es = [], []
    for b, (off, rows) in enumerate(ranges):
        P, E = fb.gemm_ref_bound(query_rows(q, b, L, q_row0, q_sample_rows), bank[off:off + rows])
        ms.append(P.amax(dim=1))
        es.append(E.amax(dim=1))
    return torch.stack(ms), torch.stack(es)


def chunk_max_ref_bound(q, bank, ranges, L, chunk_rows, q_row0=0, q_sample_rows=None):
    """Per chunk of `chunk_rows` bank rows: lists over samples of (m [chunks_b, L], e [chunks_b, L])."""
    q_sample_rows = q_row0 + L if q_sample_rows is None else q_sample_rows
    out = []
    for b, (off, rows) in enumerate(ranges):
        P, E = fb.gemm_ref_bound(query_rows(q, b, L, q_row0, q_sample_rows), bank[off:off + rows])
        cuts = range(0, rows, chunk_rows)
        out.append((torch.stack([P[:, c:c + chunk_rows].amax(dim=1) for c in cuts]),
                    torch.stack([E[:, c:c + chunk_rows].amax(dim=1) for c in cuts])))
    return out


def head_ref_bound(q_taps, bank_taps, ranges, L, S, q_row0=0, q_sample_rows=None, w=None):
    """The whole head in fp64.  q_taps / bank_taps: one [*, D] tensor per tap.  Returns a dict of (value, bound) pairs:
    sim [B, h, h], simmask [B, h, h], amap [B, S, S]."""
    T = len(q_taps)
    w = fb.f32_value(1.0 / T if w is None else w)
    h = int(round(L ** 0.5))
    assert h * h == L
    sim = mag = e = 0.0
    for q, bank in zip(q_taps, bank_taps):
        m, em = tap_max_ref_bound(q, bank, ranges, L, q_row0, q_sample_rows)
        sim = sim + w * m
        mag = mag + (w * m).abs()
        e = e + abs(w) * em
    e = e + (T + 2) * U32 * mag
    B = len(ranges)
    sim, e = sim.view(B, h, h), e.view(B, h, h)
    simmask = 1 - sim
    e_mask = e + U32 * simmask.abs()
    amap, e_map = fb.bilinear_ref_bound(sim, S, S, one_minus=True)
    e_map = e_map + (1 + 8 * U32) * fb.bilinear_ref_bound(e, S, S)[0]
    return dict(sim=(sim, e), simmask=(simmask, e_mask), amap=(amap, e_map))


def check_head(got_sim, got_simmask, got_amap, ref, what=""):
    """assert_within for the three outputs; returns the largest err / bound."""
    worst = 0.0
    for name, got in (("sim", got_sim), ("simmask", got_simmask), ("amap", got_amap)):
        v, e = ref[name]
        worst = max(worst, fb.assert_within(got.reshape(v.shape).to(v.device), v, e, f"{what} {name}"))
    return worst
