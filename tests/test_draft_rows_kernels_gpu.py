"""The kernels of draft-and-verify decoding in the decode slots.  mh_attn_decode_rope_draft_rows (mh_attn_decode_rope_draft with a
row count nrow[g] per group) against mh_attn_decode_rope_draft on the same inputs, bit for bit below nrow[g]: out rows, rotated q,
cache rows; the rows from nrow[g] on and idle groups leave a poisoned q and cache alone and get zero out rows.  One captured launch
replayed while the host moves pos, nrow and live, and the launcher's refusals on its return code.  mh_draft_accept_rows against an
integer restatement of its rule, exactly."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from tests.test_draft_kernels_gpu import POSITIONS, T_CAP, _bits, _case, _i32, _tables  # noqa: E402

DEV = "cuda:0"
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


# ------------------------------------------------------------------------------------------------ mh_attn_decode_rope_draft_rows
def _check_rows(c, nrow, cos, sin):
    """One launch of the rows form on copies of c's buffers against the K-row kernel on other copies."""
    K, W = c["K"], c["W"]
    for g, (lv, n) in enumerate(zip(c["live"], nrow)):                        # the rows no workgroup may read: NaN, q | k | v
        c["qkv"][g * K + (n if lv else 0):(g + 1) * K] = float("nan")
    qkv, cache = c["qkv"].clone(), c["cache"].clone()
    out = ops.attn_decode_rope_draft_rows(qkv, cache, _i32(c["pos"]), _i32(c["live"]), _i32(nrow), cos, sin, c["H"], c["D"], c["scale"], K,
                                          out=c["out"].clone())
    ref_qkv, ref_cache = c["qkv"].clone(), c["cache"].clone()
    ref_out = ops.attn_decode_rope_draft(ref_qkv, ref_cache, _i32(c["pos"]), _i32(c["live"]), cos, sin, c["H"], c["D"], c["scale"], K,
                                         out=c["out"].clone())
    torch.cuda.synchronize()
    tag = (c["H"], c["D"], K, c["pos"], c["live"], nrow)
    zero = torch.zeros(W, dtype=torch.int16)
    for g, (p, lv, n) in enumerate(zip(c["pos"], c["live"], nrow)):
        rows = n if lv else 0
        for j in range(K):
            r = g * K + j
            if j < rows:                                                      # the K-row kernel's bits: out, rotated q, cache row
                assert torch.equal(_bits(out[r]), _bits(ref_out[r])), (tag, g, j)
                assert torch.equal(_bits(qkv[r]), _bits(ref_qkv[r])), (tag, g, j)
                assert torch.equal(_bits(cache[g, p + j]), _bits(ref_cache[g, p + j])), (tag, g, j)
                assert not bool(out[r].isnan().any()) and not bool(cache[g, p + j].isnan().any()), (tag, g, j)
            else:                                                             # skipped: q as it was, a zero out row
                assert torch.equal(_bits(out[r]), zero), (tag, g, j)
                assert torch.equal(_bits(qkv[r]), _bits(c["qkv"][r])), (tag, g, j)
        lo = p + rows if lv else 0                                            # every cache row the launch must not write
        assert torch.equal(_bits(cache[g, lo:]), _bits(c["cache"][g, lo:])) and bool(cache[g, lo:].isnan().all()), (tag, g)
        assert torch.equal(_bits(cache[g, :p if lv else 0]), _bits(c["cache"][g, :p if lv else 0])), (tag, g)
        assert torch.equal(_bits(qkv[g * K:(g + 1) * K, W:]), _bits(c["qkv"][g * K:(g + 1) * K, W:])), (tag, g)      # k | v only read


@pytest.mark.parametrize("K", [1, 2, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H", [1, 4])
def test_rows_below_nrow_have_the_k_row_kernels_bits_and_the_rest_is_left_alone(H, D, K):
    cos, sin = _tables(T_CAP, D)
    P = POSITIONS(K)
    counts = [1, max(1, K // 2), K]                                           # 1, a middle value, K
    for i, p in enumerate(P):
        pos = [p, P[(i + 3) % len(P)], P[(i + 5) % len(P)]]
        nrow = counts[i % 3:] + counts[:i % 3]                                # every group position sees every count
        _check_rows(_case(H, D, K, pos, [1, 1, 1], seed=400 + i), nrow, cos, sin)
        live = [1, 1, 1]
        live[1 + i % 2] = 0                                                   # one idle group, never the one at p
        _check_rows(_case(H, D, K, pos, live, seed=500 + i), nrow, cos, sin)


def test_one_captured_launch_replays_while_the_host_moves_pos_nrow_and_live():
    H, D, K = 4, 128, 4
    cos, sin = _tables(T_CAP, D)
    c = _case(H, D, K, [0, 0, 0], [1, 1, 1], seed=21)
    c["cache"] = (torch.randn(3, T_CAP, 2 * H * D, generator=torch.Generator().manual_seed(22)) * 0.7).to(BF16).to(DEV)
    qkv, cache, out = c["qkv"].clone(), c["cache"].clone(), c["out"].clone()
    pos, live, nrow = _i32([0, 0, 0]), _i32([1, 1, 1]), _i32([K, K, K])

    def launch():
        ops.attn_decode_rope_draft_rows(qkv, cache, pos, live, nrow, cos, sin, H, D, c["scale"], K, out=out)

    launch()                                                                  # warm, then capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        launch()
    for p, lv, n in (([16, 129, 0], [1, 1, 1], [1, 4, 2]), ([63, 5, 200], [1, 0, 1], [3, 4, 1]), ([T_CAP - K, 127, 64], [0, 1, 1], [4, 2, 4])):
        qkv.copy_(c["qkv"])
        cache.copy_(c["cache"])
        out.fill_(float("nan"))
        pos.copy_(_i32(p))
        live.copy_(_i32(lv))
        nrow.copy_(_i32(n))
        graph.replay()
        ref_qkv, ref_cache = c["qkv"].clone(), c["cache"].clone()
        ref_out = ops.attn_decode_rope_draft(ref_qkv, ref_cache, _i32(p), _i32(lv), cos, sin, H, D, c["scale"], K)
        torch.cuda.synchronize()
        for g in range(3):
            rows = n[g] if lv[g] else 0
            sl = slice(g * K, g * K + rows)
            assert torch.equal(_bits(out[sl]), _bits(ref_out[sl])) and torch.equal(_bits(qkv[sl]), _bits(ref_qkv[sl])), (p, g)
            assert torch.equal(_bits(cache[g, p[g]:p[g] + rows]), _bits(ref_cache[g, p[g]:p[g] + rows])), (p, g)
            rest = slice(g * K + rows, (g + 1) * K)
            assert not bool(out[rest].float().abs().max() > 0) if rows < K else True, (p, g)
            assert torch.equal(_bits(qkv[rest]), _bits(c["qkv"][rest])), (p, g)
            keep = torch.ones(T_CAP, dtype=torch.bool)
            keep[p[g]:p[g] + rows] = False
            assert torch.equal(_bits(cache[g][keep]), _bits(c["cache"][g][keep])), (p, g)


def _raw(c, nrow, cos, sin, K=None, D=None, ld_qkv=None, T=None, no_nrow=False):
    """The C entry itself: (return code, out after, cache after, qkv after)."""
    qkv, cache, out = c["qkv"].clone(), c["cache"].clone(), c["out"].clone()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = _lib.load().mh_attn_decode_rope_draft_rows(p(qkv), qkv.stride(0) if ld_qkv is None else ld_qkv, p(cache), cache.stride(0),
                                                    cache.stride(1), p(_i32(c["pos"])), p(_i32(c["live"])), None if no_nrow else p(_i32(nrow)),
                                                    p(cos), p(sin), p(out), out.stride(0), c["G"], c["K"] if K is None else K, c["H"],
                                                    c["D"] if D is None else D, c["T"] if T is None else T, c["scale"], ops._s())
    torch.cuda.synchronize()
    return rc, out, cache, qkv


def test_the_launcher_refuses_what_the_k_row_launcher_refuses_and_launches_nothing():
    H, D, K = 2, 64, 2
    cos, sin = _tables(T_CAP, 136)
    c = _case(H, D, K, [5], [1], seed=3)
    assert _raw(c, [2], cos, sin)[0] == 0
    for kw, want in ((dict(K=9), -3), (dict(D=136), -3), (dict(D=72), -3), (dict(T=40000), -3),      # MH_ERR_UNSUPPORTED
                     (dict(ld_qkv=3 * H * D + 4), -1), (dict(K=0), -1), (dict(no_nrow=True), -1)):    # MH_ERR_ARG
        rc, out, cache, qkv = _raw(c, [2], cos, sin, **kw)
        assert rc == want, (kw, rc)
        assert bool(out.isnan().all()) and torch.equal(_bits(cache), _bits(c["cache"])) and torch.equal(_bits(qkv), _bits(c["qkv"])), kw


def test_a_row_past_the_cache_is_still_guarded():
    H, D, K = 4, 64, 4
    cos, sin = _tables(T_CAP + 8, D)
    c = _case(H, D, K, [T_CAP - 3], [1], seed=7)                              # rows 0 .. 2 fit, row 3 would be position T_cap
    qkv, cache = c["qkv"].clone(), c["cache"].clone()
    out = ops.attn_decode_rope_draft_rows(qkv, cache, _i32(c["pos"]), _i32([1]), _i32([4]), cos, sin, H, D, c["scale"], K, out=c["out"].clone())
    ref_qkv, ref_cache = c["qkv"].clone(), c["cache"].clone()
    ref_out = ops.attn_decode_rope_draft(ref_qkv, ref_cache, _i32(c["pos"]), _i32([1]), cos, sin, H, D, c["scale"], K, out=c["out"].clone())
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(ref_out)) and torch.equal(_bits(out[3]), torch.zeros(H * D, dtype=torch.int16))
    assert torch.equal(_bits(qkv), _bits(ref_qkv)) and torch.equal(_bits(cache), _bits(ref_cache))


# ------------------------------------------------------------------------------------------------ mh_draft_accept_rows
def _accept_rows_ref(nxt, mar, pmx, ids, ng, live, top_p, pos, kv, nid):
    """The kernel's rule on integers: (record, ids_k[0] after, next_ids after, pos after, kvlen after)."""
    K = len(nxt)
    if not live:
        return [-1.0] * K + [0.0] * (2 * K + 1), ids[0], nid, pos, kv
    n = 1
    for j in range(ng):
        if nxt[j] != ids[j + 1] or (top_p > 0 and not pmx[j] >= top_p):
            break
        n += 1
    return [float(t) for t in nxt] + list(mar) + list(pmx) + [float(n)], nxt[n - 1], nxt[n - 1], pos + n, pos + n + 1


def _accept_rows_cases(K):
    """(nguess, leading real guesses that match, index of a row with a low p_max or None, filler past nguess equals the pick, live).
    Every nguess with every count of matching guesses; with all of them matching, a filler that equals the pick just past them."""
    cases = []
    for ng in range(K):
        for m in range(ng + 1):
            for low in (None, 0, ng // 2, max(ng - 1, 0)):
                cases.append((ng, m, low, m == ng and ng < K - 1, True))
        cases.append((ng, ng, None, ng < K - 1, False))                      # an idle group
    return cases


@pytest.mark.parametrize("top_p", [0.0, 0.5])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 8])
def test_accept_rows_equals_its_restatement(K, top_p):
    cases = _accept_rows_cases(K)
    gen = torch.Generator().manual_seed(70 + K)
    seen, idle, filler, at, sizes, launches = set(), 0, 0, 0, (16, 3, 1), 0
    while at < len(cases):
        G = min(sizes[launches % 3], len(cases) - at)
        if G not in sizes:                                                    # the tail: keep to the three group counts
            G = 3 if G > 3 else 1
        chunk, at, launches = cases[at:at + G], at + G, launches + 1
        nxt = torch.randint(10, 32000, (G, K), generator=gen)
        ids = torch.randint(10, 32000, (G, K), generator=gen)
        mar = torch.rand(G, K, generator=gen)
        pmx = 0.6 + 0.4 * torch.rand(G, K, generator=gen)
        pos = torch.randint(0, 500, (G,), generator=gen).to(I32)
        kv0 = torch.randint(0, 500, (G,), generator=gen).to(I32)
        nid = torch.randint(10, 32000, (G,), generator=gen)
        for g, (ng, m, low, fill, _) in enumerate(chunk):
            for j in range(K - 1):
                ids[g, j + 1] = nxt[g, j] + 1                                 # a guess that is not what row j picked ...
            for j in range(m):
                ids[g, j + 1] = nxt[g, j]                                     # ... unless it is one of the m leading matches
            if fill:
                ids[g, ng + 1] = nxt[g, ng]                                   # the filler just past the real guesses equals the pick
            if low is not None:
                pmx[g, low] = 0.25
        d = lambda t: t.clone().to(DEV)
        ids_d, nid_d, pos_d, kv_d, step = d(ids.reshape(-1)), d(nid), d(pos), d(kv0), _i32([41])
        rec = torch.full((G, 3 * K + 1), float("nan"), dtype=F32, device=DEV)  # poisoned: an idle group's record is written too
        ops.draft_accept_rows(d(nxt.reshape(-1)), d(mar.reshape(-1)), d(pmx.reshape(-1)), ids_d, nid_d, _i32([c[0] for c in chunk]),
                              _i32([int(c[4]) for c in chunk]), torch.tensor([top_p], dtype=F32, device=DEV), rec, pos_d, kv_d, step, K)
        torch.cuda.synchronize()
        assert int(step) == 42                                                # once per launch, idle group 0 or not
        rec, ids_a, nid_a, pos_a, kv_a = rec.cpu(), ids_d.cpu().view(G, K), nid_d.cpu(), pos_d.cpu(), kv_d.cpu()
        for g, (ng, m, low, fill, live) in enumerate(chunk):
            want, id0, n1, p1, kv1 = _accept_rows_ref(nxt[g].tolist(), mar[g].tolist(), pmx[g].tolist(), ids[g].tolist(), ng, live, top_p,
                                                      int(pos[g]), int(kv0[g]), int(nid[g]))
            assert rec[g].tolist() == want, (G, g, chunk[g])
            assert (int(ids_a[g, 0]), int(nid_a[g]), int(pos_a[g]), int(kv_a[g])) == (id0, n1, p1, kv1), (G, g, chunk[g])
            assert torch.equal(ids_a[g, 1:], ids[g, 1:])                      # the guesses are only read
            if not live:
                idle += 1
                continue
            seen.add(int(want[-1]))
            assert want[-1] <= ng + 1                                         # never past the real guesses
            if fill and want[-1] == ng + 1:
                filler += 1                                                   # every real guess stood and the matching filler did not
    assert seen == set(range(1, K + 1)) and idle == K and launches >= 3       # every window length, idle groups, G = 16, 3 and 1
    assert filler > 0 or K == 1


@pytest.mark.parametrize("K", [0, 9])
def test_accept_rows_refuses_k_outside_1_to_8_and_launches_nothing(K):
    G, n = 2, 2 * max(K, 1)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    z = lambda *s, dt=F32: torch.zeros(s, dtype=dt, device=DEV)
    nxt, ids, nid = z(n, dt=torch.long), torch.full((n,), 5, dtype=torch.long, device=DEV), torch.full((G,), 6, dtype=torch.long, device=DEV)
    rec, pos, kv, step = torch.full((G, 3 * max(K, 1) + 1), float("nan"), dtype=F32, device=DEV), _i32([3, 4]), _i32([8, 9]), _i32([41])
    rc = _lib.load().mh_draft_accept_rows(p(nxt), p(z(n)), p(z(n)), p(ids), p(nid), p(_i32([0, 0])), p(_i32([1, 1])), p(z(1)), p(rec),
                                          p(pos), p(kv), p(step), G, K, ops._s())
    torch.cuda.synchronize()
    assert rc == -1                                                           # MH_ERR_ARG
    assert bool(rec.isnan().all()) and int(step) == 41 and pos.tolist() == [3, 4] and kv.tolist() == [8, 9]
    assert ids.tolist() == [5] * n and nid.tolist() == [6, 6]
    with pytest.raises(_lib.MyriadHipError):
        ops.draft_accept_rows(nxt, z(n), z(n), ids, nid, _i32([0, 0]), _i32([1, 1]), z(1), rec, pos, kv, step, K)


def test_the_wrapper_refuses_a_wrong_dtype_of_every_state_buffer():
    G, K = 2, 2
    z = lambda n, dt: torch.zeros((n,), dtype=dt, device=DEV)
    good = dict(nxt=z(G * K, torch.long), margin=z(G * K, F32), pmax=z(G * K, F32), ids_k=z(G * K, torch.long), next_ids=z(G, torch.long),
                nguess=z(G, I32), live=z(G, I32), top_p=z(1, F32), rec=z(G * (3 * K + 1), F32), pos=z(G, I32), kvlen=z(G, I32),
                step_dev=z(1, I32))
    ops.draft_accept_rows(**good, K=K)                                        # idle groups: a launch that changes no state
    torch.cuda.synchronize()
    assert good["pos"].tolist() == [0, 0] and int(good["step_dev"]) == 1 and good["rec"].view(G, -1)[:, 0].tolist() == [-1.0, -1.0]
    for name, dt in (("pos", torch.long), ("kvlen", torch.long), ("step_dev", torch.long), ("margin", torch.float64), ("pmax", BF16),
                     ("rec", torch.float64), ("top_p", torch.float64), ("nguess", torch.long), ("live", torch.bool), ("nxt", I32),
                     ("ids_k", I32), ("next_ids", I32)):
        with pytest.raises(_lib.MyriadHipError):
            ops.draft_accept_rows(**dict(good, **{name: good[name].to(dt)}), K=K)
    assert int(good["step_dev"]) == 1                                         # nothing launched
