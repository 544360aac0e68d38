"""The kernels of draft-and-verify greedy decoding.  mh_attn_decode_rope_draft (K consecutive token rows of each of G sequences in
one launch) against K sequential mh_attn_decode_rope calls on copies of the same buffers, bit for bit: out rows, rotated q, cache
rows; everything it must leave alone is poisoned beforehand.  One replay from a captured graph while the host moves pos, and every
refusal of the launcher on its return code.  mh_draft_accept against a ten-line Python restatement, exactly."""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
T_CAP = 256
# the one-row kernel's wave round-robin (16 keys), its 8 x 16 unrolled group and its 128-key score pass, each at, below and above
# the edge; 0 and the last position the cache takes
POSITIONS = lambda K: [0, 1, 15, 16, 63, 64, 127, 128, 129, T_CAP - K]


def _tables(T, D):
    fr = torch.arange(T).float()[:, None] * (1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D)))[None]
    return fr.cos().contiguous().to(DEV), fr.sin().contiguous().to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _i32(x):
    return torch.tensor(list(x), dtype=I32, device=DEV)


def _case(H, D, K, pos, live, seed, T=T_CAP):
    """Device inputs of one launch: qkv rows, the cache with random rows below pos[g] and NaN from there on (an idle sequence's
    slice is NaN throughout), the NaN out buffer."""
    g = torch.Generator().manual_seed(seed)
    G, W = len(pos), H * D
    qkv = (torch.randn(G * K, 3 * W, generator=g) * 0.7).to(BF16)
    cache = (torch.randn(G, T, 2 * W, generator=g) * 0.7).to(BF16)
    for i, (p, lv) in enumerate(zip(pos, live)):
        cache[i, (p if lv else 0):] = float("nan")
    return dict(H=H, D=D, K=K, G=G, W=W, T=T, pos=list(pos), live=list(live), scale=1.0 / D ** 0.5, qkv=qkv.to(DEV), cache=cache.to(DEV),
                out=torch.full((G * K, W), float("nan"), dtype=BF16, device=DEV))


def _sequential(c, cos, sin, rows=None):
    """K sequential one-row steps per live sequence on copies of the buffers: (out, qkv after, cache after); idle rows of out are 0."""
    qkv, cache = c["qkv"].clone(), c["cache"].clone()
    out = torch.zeros_like(c["out"])
    for g, (p, lv) in enumerate(zip(c["pos"], c["live"])):
        for j in range(c["K"] if rows is None else rows):
            if not lv:
                continue
            r = g * c["K"] + j
            ps = _i32([p + j])
            out[r] = ops.attn_decode_rope(qkv[r:r + 1], cache[g:g + 1], ps, ps, _i32([p + j + 1]), cos, sin, c["H"], c["D"], c["scale"])[0]
    return out, qkv, cache


def _check(c, cos, sin):
    before = c["cache"].clone()
    qkv, cache = c["qkv"].clone(), c["cache"].clone()
    out = ops.attn_decode_rope_draft(qkv, cache, _i32(c["pos"]), _i32(c["live"]), cos, sin, c["H"], c["D"], c["scale"], c["K"], out=c["out"].clone())
    ref_out, ref_qkv, ref_cache = _sequential(c, cos, sin)
    torch.cuda.synchronize()
    tag = (c["H"], c["D"], c["K"], c["pos"], c["live"])
    assert torch.equal(_bits(out), _bits(ref_out)), tag                       # a live row's bits; an idle sequence's rows are zeros
    assert torch.equal(_bits(qkv), _bits(ref_qkv)), tag                       # q rotated in place, k | v as they were
    assert torch.equal(_bits(cache), _bits(ref_cache)), tag                   # rows pos .. pos + K - 1 and nothing else
    W, K = c["W"], c["K"]
    for g, (p, lv) in enumerate(zip(c["pos"], c["live"])):
        if not lv:                                                            # an idle sequence: slice, qkv rows untouched, out 0
            assert torch.equal(_bits(cache[g]), _bits(before[g])) and torch.equal(_bits(qkv[g * K:(g + 1) * K]), _bits(c["qkv"][g * K:(g + 1) * K]))
            assert not bool(out[g * K:(g + 1) * K].float().abs().max() > 0) and not bool(out[g * K:(g + 1) * K].isnan().any())
            continue
        assert torch.equal(_bits(cache[g, :p]), _bits(before[g, :p])), tag    # only read
        assert torch.equal(_bits(cache[g, p + K:]), _bits(before[g, p + K:])) and bool(cache[g, p + K:].isnan().all()), tag
        assert not bool(cache[g, p:p + K].isnan().any()) and not bool(out[g * K:(g + 1) * K].isnan().any()), tag
        assert torch.equal(_bits(qkv[g * K:(g + 1) * K, W:]), _bits(c["qkv"][g * K:(g + 1) * K, W:])), tag


@pytest.mark.parametrize("K", [1, 2, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H", [1, 4])
def test_every_row_has_the_bits_of_sequential_one_row_steps(H, D, K):
    cos, sin = _tables(T_CAP, D)
    P = POSITIONS(K)
    for i, p in enumerate(P):
        other = P[(i + 3) % len(P)]                                           # a second sequence at another position
        _check(_case(H, D, K, [p], [1], seed=100 + i), cos, sin)
        _check(_case(H, D, K, [p, other], [1, 1], seed=200 + i), cos, sin)
        _check(_case(H, D, K, [p, other], [1, 0] if i % 2 else [0, 1], seed=300 + i), cos, sin)


def test_a_row_past_the_cache_writes_nothing_and_gets_a_zero_out_row():
    H, D, K = 4, 64, 4
    cos, sin = _tables(T_CAP + 8, D)
    c = _case(H, D, K, [T_CAP - 3], [1], seed=7)                              # rows 0 .. 2 fit, row 3 would be position T_cap
    qkv, cache = c["qkv"].clone(), c["cache"].clone()
    out = ops.attn_decode_rope_draft(qkv, cache, _i32(c["pos"]), _i32([1]), cos, sin, H, D, c["scale"], K, out=c["out"].clone())
    ref_out, ref_qkv, ref_cache = _sequential(c, cos, sin, rows=3)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[:3]), _bits(ref_out[:3])) and torch.equal(_bits(out[3]), torch.zeros(H * D, dtype=torch.int16))
    assert torch.equal(_bits(qkv), _bits(ref_qkv)) and torch.equal(_bits(cache), _bits(ref_cache))


def test_one_captured_launch_replays_while_the_host_moves_pos():
    H, D, K = 4, 128, 4
    cos, sin = _tables(T_CAP, D)
    c = _case(H, D, K, [0, 0], [1, 1], seed=11)
    c["cache"] = (torch.randn(2, T_CAP, 2 * H * D, generator=torch.Generator().manual_seed(12)) * 0.7).to(BF16).to(DEV)
    qkv, cache, out, pos, live = c["qkv"].clone(), c["cache"].clone(), c["out"].clone(), _i32([0, 0]), _i32([1, 1])

    def launch():
        ops.attn_decode_rope_draft(qkv, cache, pos, live, cos, sin, H, D, c["scale"], K, out=out)

    launch()                                                                  # warm, then capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        launch()
    for p, lv in (([16, 129], [1, 1]), ([63, 5], [1, 0]), ([T_CAP - K, 127], [1, 1])):
        qkv.copy_(c["qkv"])
        cache.copy_(c["cache"])
        out.fill_(float("nan"))
        pos.copy_(_i32(p))
        live.copy_(_i32(lv))
        graph.replay()
        ref_out, ref_qkv, ref_cache = _sequential(dict(c, pos=p, live=lv), cos, sin)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(ref_out)) and torch.equal(_bits(qkv), _bits(ref_qkv)), p
        assert torch.equal(_bits(cache), _bits(ref_cache)), p


def _raw(c, cos, sin, K=None, D=None, ld_qkv=None, T=None):
    """The C entry itself: (return code, out after, cache after, qkv after)."""
    qkv, cache, out = c["qkv"].clone(), c["cache"].clone(), c["out"].clone()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = _lib.load().mh_attn_decode_rope_draft(p(qkv), qkv.stride(0) if ld_qkv is None else ld_qkv, p(cache), cache.stride(0), cache.stride(1),
                                               p(_i32(c["pos"])), p(_i32(c["live"])), p(cos), p(sin), p(out), out.stride(0), c["G"],
                                               c["K"] if K is None else K, c["H"], c["D"] if D is None else D, c["T"] if T is None else T,
                                               c["scale"], ops._s())
    torch.cuda.synchronize()
    return rc, out, cache, qkv


def test_the_launcher_refuses_what_it_cannot_run_and_launches_nothing():
    H, D, K = 2, 64, 2
    cos, sin = _tables(T_CAP, 136)
    c = _case(H, D, K, [5], [1], seed=3)
    assert _raw(c, cos, sin)[0] == 0
    for kw, want in ((dict(K=9), -3), (dict(D=136), -3), (dict(D=72), -3), (dict(T=40000), -3),      # MH_ERR_UNSUPPORTED
                     (dict(ld_qkv=3 * H * D + 4), -1), (dict(K=0), -1)):                              # MH_ERR_ARG
        rc, out, cache, qkv = _raw(c, cos, sin, **kw)
        assert rc == want, (kw, rc)
        assert bool(out.isnan().all()) and torch.equal(_bits(cache), _bits(c["cache"])) and torch.equal(_bits(qkv), _bits(c["qkv"])), kw
    assert ops.attn_decode_draft_supported(32, 128, 8, 8192) and not ops.attn_decode_draft_supported(32, 128, 9, 8192)
    assert not ops.attn_decode_draft_supported(32, 72, 4, 256) and not ops.attn_decode_draft_supported(32, 128, 4, 40000)
    # the LDS bound, derived: 4 * round_up(T_cap, 64) + 8192 + 2 K D bytes against 160 KiB
    fits = (160 * 1024 - 8192 - 2 * 8 * 128) // 4 // 64 * 64
    assert ops.attn_decode_draft_supported(32, 128, 8, fits) and not ops.attn_decode_draft_supported(32, 128, 8, fits + 1)


# ------------------------------------------------------------------------------------------------ mh_draft_accept
def _accept_ref(nxt, mar, pmx, ids, top_p, pos):
    """The kernel's rule, restated: (record, ids[0] after, pos after, kvlen after)."""
    K, n = len(nxt), 1
    for j in range(K - 1):
        if nxt[j] != ids[j + 1] or (top_p > 0 and not pmx[j] >= top_p):
            break
        n += 1
    return [float(t) for t in nxt] + list(mar) + list(pmx) + [float(n)], nxt[n - 1], pos + n, pos + n + 1


def _accept_cases(K):
    """(match pattern, index of a row with a low p_max or None): every pattern for K <= 4, a sample for K = 8."""
    pats = list(itertools.product([0, 1], repeat=K - 1))
    if K == 8:
        g = torch.Generator().manual_seed(8)
        pats = [(1,) * i + (0,) * (7 - i) for i in range(8)] + [pats[int(i)] for i in torch.randint(0, len(pats), (12,), generator=g)]
    return [(pat, low) for pat in pats for low in [None] + list(range(K))]


@pytest.mark.parametrize("top_p", [0.0, 0.5])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 8])
def test_accept_equals_its_restatement(K, top_p):
    cases = _accept_cases(K)
    G = len(cases)
    gen = torch.Generator().manual_seed(40 + K)
    nxt = torch.randint(10, 32000, (G, K), generator=gen)
    ids = torch.randint(10, 32000, (G, K), generator=gen)
    mar = torch.rand(G, K, generator=gen)
    pmx = 0.6 + 0.4 * torch.rand(G, K, generator=gen)
    pos = torch.randint(0, 500, (G,), generator=gen).to(I32)
    for g, (pat, low) in enumerate(cases):
        for j, m in enumerate(pat):
            ids[g, j + 1] = nxt[g, j] if m else nxt[g, j] + 1                 # guess j + 1 is what row j picked, or not
        if low is not None:
            pmx[g, low] = 0.25
    d = lambda t: t.clone().to(DEV)
    ids_d, pos_d, kv_d, step = d(ids.reshape(-1)), d(pos), torch.full((G,), -7, dtype=I32, device=DEV), _i32([41])
    rec = torch.full((G, 3 * K + 1), float("nan"), dtype=F32, device=DEV)
    ops.draft_accept(d(nxt.reshape(-1)), d(mar.reshape(-1)), d(pmx.reshape(-1)), ids_d, torch.tensor([top_p], dtype=F32, device=DEV), rec,
                     pos_d, kv_d, step, K)
    torch.cuda.synchronize()
    rec, ids_a, pos_a, kv_a = rec.cpu(), ids_d.cpu().view(G, K), pos_d.cpu(), kv_d.cpu()
    assert int(step) == 42                                                    # once per launch
    seen = set()
    for g in range(G):
        want, id0, p1, kv1 = _accept_ref(nxt[g].tolist(), mar[g].tolist(), pmx[g].tolist(), ids[g].tolist(), top_p, int(pos[g]))
        assert rec[g].tolist() == want, (g, cases[g])
        assert int(ids_a[g, 0]) == id0 and int(pos_a[g]) == p1 and int(kv_a[g]) == kv1, (g, cases[g])
        assert torch.equal(ids_a[g, 1:], ids[g, 1:])                          # the guesses are only read
        seen.add(int(want[-1]))
    assert seen == set(range(1, K + 1))                                       # every window length occurred
