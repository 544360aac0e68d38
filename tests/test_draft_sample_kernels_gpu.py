"""The kernels of draft-and-verify decoding under the slot engine's per-row tail (csrc/draft_sample.hip), each held to its bit
contract.  mh_repetition_penalty_draft_rows against mh_repetition_penalty_rows_slots run on copies whose rows carry the bitmap the
contract names (seen[g] plus the earlier fed ids), and against the numpy restatement; mh_sample_rows_draft against
mh_sample_rows_slots / mh_argmax_pmax_rows_slots on the same rows with the per-row state spelled out (seed[g], gen[g] + j, the
row's own live flag) -- the slot entries treat every row alone, one workgroup each; mh_draft_accept_sampled_rows against the integer
restatement and, with kept and seen null, against mh_draft_accept_rows.  One captured graph of the three launches replayed while
the host moves nrow, nguess, live and gen; every refusal on its return code with poisoned outputs left alone."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from tests import draft_sample_ref as ref  # noqa: E402

DEV = "cuda:0"
F32, I32, I64 = torch.float32, torch.int32, torch.long
GK = [(1, 1), (1, 2), (1, 8), (3, 1), (3, 2), (3, 8)]


def _i32(v):
    return torch.tensor(v, dtype=I32, device=DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _state(G, K, variant):
    """(live, nrow): group 0 full, group 1 short (nrow < K), group 2 idle; G = 1 takes `variant` to see a full and a short group."""
    if G == 1:
        return [1], [K if variant == 0 else max(1, K // 2)]
    return [1, 1, 0], [K, max(1, K // 2), K]


def _padded(rows, V, gen):
    """f32 logits [rows, V] as a view of a [rows, ldl] buffer, ldl > V and a multiple of 4, whose border is NaN."""
    ldl = ops.round_up(V, 4) + 8
    buf = torch.full((rows, ldl), float("nan"), dtype=F32)
    buf[:, :V] = torch.randn(rows, V, generator=gen) * 3
    return buf


# ---------------------------------------------------------------------------------------------- mh_repetition_penalty_draft_rows
def _penalty_case(G, K, V, gen):
    """Bitmaps and fed ids with every overlap: an extra that is in the bitmap, two equal extras, extras at id 0 and V - 1."""
    seen_sets, ids_k = [], []
    for g in range(G):
        s = set(torch.randint(0, V, (12,), generator=gen).tolist()) | ({0} if g == 1 else set()) | {V - 2}
        seen_sets.append(s)
        inb, a, b = sorted(s)[len(s) // 2], (7 + g) % V, (V // 2 + g) % V
        ids_k.append(([inb, inb, V - 1, 0, a, a, V - 2, b] if g != 1 else [0, V - 1, inb, a, a, b, b, inb])[:K])
    return seen_sets, ids_k


@pytest.mark.parametrize("V", [33, 100, 32000])
@pytest.mark.parametrize("G,K", GK)
def test_penalty_rows_have_the_slot_kernels_bits_and_the_bitmap_is_only_read(G, K, V):
    gen = torch.Generator().manual_seed(1000 * G + 10 * K + V % 7)
    R, W = G * K, (V + 31) // 32
    pen = torch.tensor([1.3], dtype=F32, device=DEV)
    for variant in range(2 if G == 1 else 1):
        live, nrow = _state(G, K, variant)
        base = _padded(R, V, gen)
        base[:, 3] = 0.0                                                      # zero, negative and positive logits at penalised ids
        base[:, V - 1] = -base[:, V - 1].abs()
        base[:, 0] = base[:, 0].abs()
        seen_sets, ids_k = _penalty_case(G, K, V, gen)
        for s in seen_sets:
            s.add(3)
        seen = torch.from_numpy(np.stack([ref.bitmap_of(s, V) for s in seen_sets])).to(DEV)
        ids_d = torch.tensor(ids_k, dtype=I64).reshape(-1).to(DEV)
        buf, seen0 = base.clone().to(DEV), seen.clone()
        ops.repetition_penalty_draft_rows(buf[:, :V], seen, ids_d, _i32(nrow), _i32(live), pen, K)
        # the contract: the slot kernel on a copy, row (g, j) with the bitmap seen[g] + ids_k[g, :j], prev_ids = ids_k[g, j] and
        # its own live flag
        rbuf = base.clone().to(DEV)
        rows_seen = torch.from_numpy(np.stack([ref.bitmap_of(seen_sets[g] | set(ids_k[g][:j]), V) for g in range(G) for j in range(K)]))
        rows_live = [int(bool(live[g]) and j < nrow[g]) for g in range(G) for j in range(K)]
        ops.repetition_penalty_rows_slots(rbuf[:, :V], rows_seen.to(DEV), ids_d.clone(), pen, _i32(rows_live))
        torch.cuda.synchronize()
        assert torch.equal(_bits(seen), _bits(seen0))                         # the bitmap is unchanged
        got, want = _bits(buf), _bits(rbuf)
        assert torch.equal(got, want), (G, K, V, variant)                     # every row, the NaN border included
        host = ref.penalty_draft_ref(base[:, :V].numpy(), seen_sets, np.array(ids_k).reshape(-1), nrow, live, K, 1.3)
        assert np.array_equal(buf[:, :V].cpu().numpy().view(np.int32), host.view(np.int32)), (G, K, V, variant)
        for g in range(G):
            for j in range(K):
                if not rows_live[g * K + j]:                                  # other rows are left alone
                    assert torch.equal(got[g * K + j], _bits(base[g * K + j]))
        assert bool(buf[:, V:].isnan().all())


# ---------------------------------------------------------------------------------------------------------- mh_sample_rows_draft
def _sampler_rows(G, K, live, nrow, gen0, seeds):
    """The per-row state the slot entries take for the same rows."""
    rl = [int(bool(live[g]) and j < nrow[g]) for g in range(G) for j in range(K)]
    rg = [gen0[g] + j for g in range(G) for j in range(K)]
    rs = [seeds[g] for g in range(G) for j in range(K)]
    return _i32(rl), _i32(rg), torch.tensor(rs, dtype=I64, device=DEV), rl


def _outs(R):
    return (torch.full((R,), -7, dtype=I64, device=DEV), torch.full((R,), float("nan"), dtype=F32, device=DEV),
            torch.full((R,), float("nan"), dtype=F32, device=DEV), torch.full((R,), -7, dtype=I32, device=DEV),
            torch.full((R,), float("nan"), dtype=F32, device=DEV))


def _check_sampler(logits, G, K, V, draw, top_k, top_p, variant, inv_temp=1.0, want_kept=None):
    live, nrow = _state(G, K, variant)
    gen0, seeds = [1, 5, 2][:G], [0x1234567 + 11, -99887766554433, 3][:G]
    eos = V - 3
    min_length = gen0[0] + max(1, K // 2)                                     # the ban ends inside group 0 (K > 1)
    prm = torch.tensor([inv_temp, top_p, float(top_k), 1.0, float(min_length), float(eos)], dtype=F32, device=DEV)
    rl_d, rg_d, rs_d, rl = _sampler_rows(G, K, live, nrow, gen0, seeds)
    R = G * K
    out, mar, pmx, kept, u = _outs(R)
    ops.sample_rows_draft(logits, out, mar, pmx, kept, prm, torch.tensor(seeds, dtype=I64, device=DEV), _i32(gen0), _i32(nrow),
                          _i32(live), K, draw, u_out=u)
    o2, m2, p2, k2, u2 = _outs(R)
    if draw:
        ops.sample_rows_slots(logits, o2, m2, p2, k2, prm, rs_d, rg_d, rl_d, u_out=u2)
    else:
        ops.argmax_pmax_rows_slots(logits, o2, m2, p2, prm, rg_d, rl_d)
    torch.cuda.synchronize()
    tag = (G, K, V, draw, top_k, top_p, variant)
    for a, b in ((out, o2), (mar, m2), (pmx, p2), (kept, k2), (u, u2)):       # kept and u_out: the poison without the draw
        assert torch.equal(_bits(a.to(F32) if a.dtype == I64 else a), _bits(b.to(F32) if b.dtype == I64 else b)), tag
    assert torch.equal(out.cpu(), o2.cpu()), tag
    for r in range(R):
        if not rl[r]:                                                         # idle rows as specified
            assert (int(out[r]), float(mar[r]), float(pmx[r])) == (-1, 0.0, 0.0), tag
            assert int(kept[r]) == (0 if draw else -7) and bool(u[r].isnan()), tag
        elif draw and want_kept is not None:
            assert int(kept[r]) == want_kept, tag
    banned = [r for r in range(R) if rl[r] and (gen0[r // K] + r % K) < min_length]
    assert all(int(out[r]) != eos for r in banned), tag
    return out.cpu(), banned, [r for r in range(R) if rl[r] and r not in banned]


@pytest.mark.parametrize("draw", [0, 1])
@pytest.mark.parametrize("V", [8, 1000, 32768])
@pytest.mark.parametrize("G,K", GK)
def test_sampler_rows_have_the_slot_entries_bits_at_gen_plus_j(G, K, V, draw):
    gen = torch.Generator().manual_seed(7 * G + K + V)
    buf = _padded(G * K, V, gen)
    buf[:, V - 3] = 40.0                                                      # eos_id is the arg-max of every row: the ban decides
    logits = buf.to(DEV)[:, :V]
    inside = False
    for variant in range(2 if G == 1 else 1):
        for top_k in (1, 50):
            for top_p in (0.3, 1.0):
                out, banned, free = _check_sampler(logits, G, K, V, draw, top_k, top_p, variant)
                if not draw or top_k == 1:
                    assert all(int(out[r]) == V - 3 for r in free)            # where the ban has ended the pick is eos_id again
                inside |= any(r < K for r in banned) and any(r < K for r in free)
    assert inside or K == 1                                                   # the ban ends inside group 0


@pytest.mark.parametrize("G,K", [(1, 2), (3, 8)])
def test_sampler_hands_a_flat_row_past_the_cap_to_the_host(G, K):
    V = 2052                                                                  # a tied top-k set of 2051 > 1024 candidates
    logits = torch.zeros((G * K, V), dtype=F32, device=DEV)
    _check_sampler(logits, G, K, V, 1, 50, 1.0, 0, want_kept=-1)
    _check_sampler(logits, G, K, V, 0, 50, 1.0, 0)


def test_sampler_refusals_launch_nothing():
    G, K, V = 2, 2, 64
    L, p = _lib.load(), lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    big = torch.zeros((G * K, 32772), dtype=F32, device=DEV)
    odd = torch.zeros((G * K, 66), dtype=F32, device=DEV)
    ok = torch.zeros((G * K + 1, 64), dtype=F32, device=DEV)
    prm = torch.tensor([1.0, 1.0, 50.0, 1.0, 0.0, 2.0], dtype=F32, device=DEV)
    seed, gen_, nrow, live = torch.zeros(G, dtype=I64, device=DEV), _i32([0, 0]), _i32([2, 2]), _i32([1, 1])
    out, mar, pmx, kept, u = _outs(G * K)

    def call(logits, ldl, V_, K_=K, base=0, **null):
        a = dict(out=out, mar=mar, pmx=pmx, kept=kept, prm=prm, seed=seed, gen=gen_, nrow=nrow, live=live)
        a.update(null)
        ptr = ctypes.c_void_p(logits.data_ptr() + base)
        return L.mh_sample_rows_draft(ptr, ldl, p(a["out"]), p(a["mar"]), p(a["pmx"]), p(a["kept"]), p(u), G, K_, V_, p(a["prm"]),
                                      p(a["seed"]), p(a["gen"]), p(a["nrow"]), p(a["live"]), 1, ops._s())

    assert call(big, 32772, 32772) == -3                                      # MH_ERR_UNSUPPORTED: V past the registers
    assert call(odd, 66, 64) == -3                                            # ldl % 4
    assert call(ok, 64, 64, base=4) == -3                                     # a base off 16 bytes
    assert call(ok, 64, 64, K_=0) == -1 and call(ok, 64, 64, K_=9) == -1      # MH_ERR_ARG
    assert call(ok, 32, 64) == -1 and call(ok, 64, 0) == -1                   # ldl < V, V < 1
    for name in ("out", "mar", "pmx", "kept", "prm", "seed", "gen", "nrow", "live"):
        assert call(ok, 64, 64, **{name: None}) == -1, name
    torch.cuda.synchronize()
    assert out.tolist() == [-7] * (G * K) and kept.tolist() == [-7] * (G * K)
    assert bool(mar.isnan().all()) and bool(pmx.isnan().all()) and bool(u.isnan().all())
    with pytest.raises(_lib.MyriadHipError):
        ops.sample_rows_draft(big, out, mar, pmx, kept, prm, seed, gen_, nrow, live, K, True)
    with pytest.raises(_lib.MyriadHipError):
        ops.sample_rows_draft(ok[:G * K], out, mar, pmx, kept, prm, seed, gen_.to(I64), nrow, live, K, True)
    with pytest.raises(_lib.MyriadHipError):
        ops.repetition_penalty_draft_rows(ok[:G * K], torch.zeros((G, 2), dtype=I64, device=DEV), out, nrow, live, prm[3:], K)


# -------------------------------------------------------------------------------------------------- mh_draft_accept_sampled_rows
def _accept_cases(K):
    """(nguess, leading guesses that match, index of the row the host must draw or None, filler equals the pick, live)."""
    cases = []
    for ng in range(K):
        for m in sorted({0, ng // 2, ng}):                                    # first wrong, some right, all right
            for host in (None, 0, max(m - 1, 0)):                             # ... and a right guess behind a host-drawn row
                cases.append((ng, m, host, m == ng and ng < K - 1, True))
    cases.append((K - 1, K - 1, None, False, False))                          # an idle group
    return cases


@pytest.mark.parametrize("mode", ["kept+seen", "kept", "seen", "neither"])
@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_accept_equals_its_restatement_and_draft_accept_rows_without_kept_and_seen(K, mode):
    V, top_p = 1000, 0.5
    W = (V + 31) // 32
    cases = _accept_cases(K)
    G = len(cases)
    gen = torch.Generator().manual_seed(5 + K)
    nxt = torch.randint(0, V, (G, K), generator=gen)
    ids = torch.randint(0, V, (G, K), generator=gen)
    mar, pmx = torch.rand(G, K, generator=gen), 0.6 + 0.4 * torch.rand(G, K, generator=gen)
    keptv = torch.randint(1, 50, (G, K), generator=gen).to(I32)
    pos, kv0 = torch.randint(0, 500, (G,), generator=gen).to(I32), torch.randint(0, 500, (G,), generator=gen).to(I32)
    gen0, nid = torch.randint(1, 60, (G,), generator=gen).to(I32), torch.randint(0, V, (G,), generator=gen)
    seen_sets = [set(torch.randint(0, V, (5,), generator=gen).tolist()) for _ in range(G)]
    for g, (ng, m, host, fill, _) in enumerate(cases):
        for j in range(K - 1):
            ids[g, j + 1] = (nxt[g, j] + 1) % V
        for j in range(m):
            ids[g, j + 1] = nxt[g, j]
        if fill:
            ids[g, ng + 1] = nxt[g, ng]
        if host is not None:
            keptv[g, host] = -1
            pmx[g, host] = 0.25
    ids[0, 0], ids[min(1, G - 1), 0] = 0, V - 1                               # bitmap edges
    use_kept, use_seen = "kept" in mode, "seen" in mode
    d = lambda t: t.clone().to(DEV)
    seen = torch.from_numpy(np.stack([ref.bitmap_of(s, V) for s in seen_sets])).to(DEV)
    seen0 = seen.clone()
    ids_d, nid_d, pos_d, kv_d, gen_d, step = d(ids.reshape(-1)), d(nid), d(pos), d(kv0), d(gen0), _i32([41])
    ng_d, live_d, tp_d = _i32([c[0] for c in cases]), _i32([int(c[4]) for c in cases]), torch.tensor([top_p], dtype=F32, device=DEV)
    rec = torch.full((G, 4 * K + 1), float("nan"), dtype=F32, device=DEV)
    ops.draft_accept_sampled_rows(d(nxt.reshape(-1)), d(mar.reshape(-1)), d(pmx.reshape(-1)), d(keptv.reshape(-1)) if use_kept else None,
                                  ids_d, nid_d, ng_d, live_d, tp_d, seen if use_seen else None, rec, pos_d, kv_d, gen_d, step, K, V)
    torch.cuda.synchronize()
    assert int(step) == 42
    rec_h, ids_a, seen_a = rec.cpu(), ids_d.cpu().view(G, K), seen.cpu().numpy()
    windows = set()
    for g, (ng, m, host, fill, live) in enumerate(cases):
        want = ref.accept_sampled_ref(nxt[g].tolist(), mar[g].tolist(), pmx[g].tolist(), keptv[g].tolist() if use_kept else None,
                                      ids[g].tolist(), ng, live, top_p, int(pos[g]), int(kv0[g]), int(nid[g]), int(gen0[g]),
                                      seen_sets[g] if use_seen else None, K, V)
        assert rec_h[g].tolist() == want[0], (K, mode, g, cases[g])
        got = (int(ids_a[g, 0]), int(nid_d[g]), int(pos_d[g]), int(kv_d[g]), int(gen_d[g]))
        assert got == want[1:6], (K, mode, g, cases[g])
        assert torch.equal(ids_a[g, 1:], ids[g, 1:])
        assert ref.bitmap_ids(seen_a[g], V) == (want[6] if use_seen else seen_sets[g]), (K, mode, g, cases[g])
        n = int(want[0][-1])
        if live:
            windows.add(n)
            assert n <= ng + 1                                                # a filler is never confirmed
            if host is not None and host < m:
                assert n == host + 1                                          # the right guesses behind a host-drawn row do not stand
    assert windows == set(range(1, K + 1))
    if not use_seen:
        assert torch.equal(_bits(seen), _bits(seen0))
    if mode == "neither":                                                     # mh_draft_accept_rows, bit for bit
        ids2, nid2, pos2, kv2, step2 = d(ids.reshape(-1)), d(nid), d(pos), d(kv0), _i32([41])
        rec2 = torch.full((G, 3 * K + 1), float("nan"), dtype=F32, device=DEV)
        ops.draft_accept_rows(d(nxt.reshape(-1)), d(mar.reshape(-1)), d(pmx.reshape(-1)), ids2, nid2, ng_d, live_d, tp_d, rec2, pos2, kv2,
                              step2, K)
        torch.cuda.synchronize()
        assert torch.equal(_bits(rec[:, :3 * K]), _bits(rec2[:, :3 * K])) and torch.equal(_bits(rec[:, 4 * K]), _bits(rec2[:, 3 * K]))
        assert not bool(rec[:, 3 * K:4 * K].any())
        for a, b in ((ids_d, ids2), (nid_d, nid2), (pos_d, pos2), (kv_d, kv2), (step, step2)):
            assert torch.equal(a.cpu(), b.cpu())


@pytest.mark.parametrize("K", [0, 9])
def test_accept_and_penalty_refuse_k_outside_1_to_8_and_launch_nothing(K):
    G, n, V = 2, 2 * max(K, 1), 64
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    z = lambda *s, dt=F32: torch.zeros(s, dtype=dt, device=DEV)
    nxt, ids, nid = z(n, dt=I64), torch.full((n,), 5, dtype=I64, device=DEV), torch.full((G,), 6, dtype=I64, device=DEV)
    rec, pos, kv, step, gen_ = torch.full((G, 4 * max(K, 1) + 1), float("nan"), dtype=F32, device=DEV), _i32([3, 4]), _i32([8, 9]), _i32([41]), _i32([2, 2])
    seen = z(G, 2, dt=I32)
    rc = _lib.load().mh_draft_accept_sampled_rows(p(nxt), p(z(n)), p(z(n)), p(z(n, dt=I32)), p(ids), p(nid), p(_i32([0, 0])),
                                                  p(_i32([1, 1])), p(z(1)), p(seen), p(rec), p(pos), p(kv), p(gen_), p(step), G, K, V,
                                                  ops._s())
    logits = torch.full((n, V), 2.0, dtype=F32, device=DEV)
    seen[:] = -1
    rc2 = _lib.load().mh_repetition_penalty_draft_rows(p(logits), V, p(seen), p(ids), p(_i32([1, 1])), p(_i32([1, 1])), G, K, V,
                                                       p(torch.tensor([2.0], dtype=F32, device=DEV)), ops._s())
    torch.cuda.synchronize()
    assert rc == -1 and rc2 == -1                                             # MH_ERR_ARG
    assert bool(rec.isnan().all()) and int(step) == 41 and pos.tolist() == [3, 4] and kv.tolist() == [8, 9] and gen_.tolist() == [2, 2]
    assert ids.tolist() == [5] * n and nid.tolist() == [6, 6] and bool((logits == 2.0).all())


# ------------------------------------------------------------------------------------------------------------------ graph replay
def test_one_captured_graph_of_the_three_launches_replays_while_the_host_moves_the_state():
    G, K, V = 3, 4, 100
    W = (V + 31) // 32
    g_ = torch.Generator().manual_seed(3)
    base = torch.randn(G * K, V, generator=g_) * 3
    eos, min_length = 5, 4
    prm = torch.tensor([1.0, 0.9, 50.0, 1.2, float(min_length), float(eos)], dtype=F32, device=DEV)
    logits = torch.empty((G * K, V), dtype=F32, device=DEV)
    seen, ids_k, next_ids = torch.zeros((G, W), dtype=I32, device=DEV), torch.zeros(G * K, dtype=I64, device=DEV), torch.zeros(G, dtype=I64, device=DEV)
    cnt = torch.zeros((4, G), dtype=I32, device=DEV)                          # nguess, nrow, live, gen: what the host moves
    nguess, nrow, live, gen_ = cnt[0], cnt[1], cnt[2], cnt[3]
    seed = torch.tensor([11, 22, 33], dtype=I64, device=DEV)
    pos, kv, step = torch.zeros(G, dtype=I32, device=DEV), torch.zeros(G, dtype=I32, device=DEV), _i32([0])
    out, mar, pmx, kept, _u = _outs(G * K)
    rec, tp = torch.zeros((G, 4 * K + 1), dtype=F32, device=DEV), torch.zeros(1, dtype=F32, device=DEV)

    def launch(lg, o, m, p_, k_, sn, ik, ni, ps, kv_, gn, st, rc):
        ops.repetition_penalty_draft_rows(lg, sn, ik, nrow, live, prm[3:], K)
        ops.sample_rows_draft(lg, o, m, p_, k_, prm, seed, gn, nrow, live, K, True)
        ops.draft_accept_sampled_rows(o, m, p_, k_, ik, ni, nguess, live, tp, sn, rc, ps, kv_, gn, st, K, V)

    main = (logits, out, mar, pmx, kept, seen, ids_k, next_ids, pos, kv, gen_, step, rec)
    logits.copy_(base)
    cnt.copy_(torch.tensor([[0] * G, [1] * G, [0] * G, [0] * G], dtype=I32))
    launch(*main)                                                             # warm (all idle), then capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        launch(*main)
    for ng, lv, gn in (([3, 1, 0], [1, 1, 1], [1, 2, 7]), ([2, 3, 3], [1, 0, 1], [3, 9, 2]), ([0, 2, 1], [0, 1, 1], [5, 1, 3])):
        fed = torch.randint(0, V, (G * K,), generator=g_)
        seen0 = torch.from_numpy(np.stack([ref.bitmap_of(set(torch.randint(0, V, (6,), generator=g_).tolist()), V) for _ in range(G)]))
        state = torch.tensor([ng, [n + 1 for n in ng], lv, gn], dtype=I32)
        # an eager run on copies (same launches, same state) first: its picks become the next replay's guesses, so some stand
        eager = [t.clone() for t in main]
        eager[0].copy_(base)
        eager[5].copy_(seen0)
        eager[6].copy_(fed)
        eager[10] = gn_e = _i32(gn)
        cnt.copy_(state)
        launch(*eager)
        torch.cuda.synchronize()
        picks = eager[1].cpu().view(G, K)
        fed = fed.view(G, K).clone()
        fed[:, 1:3] = picks[:, 0:2].clamp(min=0)                              # rows 1 and 2 guess what rows 0 and 1 picked
        for t, v in ((eager[0], base), (eager[5], seen0), (eager[6], fed.reshape(-1)), (logits, base), (seen, seen0), (ids_k, fed.reshape(-1))):
            t.copy_(v)
        gn_e.copy_(_i32(gn))
        for t in (eager[8], eager[9], eager[11], pos, kv, step):
            t.fill_(17)
        cnt.copy_(state)
        launch(*eager)
        cnt.copy_(state)                                                      # gen is part of cnt: the eager run used its own copy
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(main, eager):
            assert torch.equal(_bits(a.to(F32) if a.dtype == I64 else a), _bits(b.to(F32) if b.dtype == I64 else b)), (ng, lv, gn)
        r = rec.cpu()
        for g in range(G):
            assert int(r[g, 4 * K]) == (0 if not lv[g] else int(r[g, 4 * K])) and int(gen_[g]) == gn[g] + int(r[g, 4 * K])
            assert int(pos[g]) == 17 + int(r[g, 4 * K])
        assert int(step) == 18
