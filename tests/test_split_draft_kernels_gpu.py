"""The split-KV verify-step attention.  mh_attn_decode_rope_split_draft[_rows] (K consecutive token rows of each of G sequences, one
workgroup per (chunk, sequence, head) that loads every cached key once for the K queries) against nrow[g] sequential
mh_attn_decode_rope_split_rows launches at B = 1 on a copy of the same cache, bit for bit: out rows and the appended cache rows.
out, the partials and every cache row >= pos[g] are NaN beforehand; every other cache row and all of qkv must come back as they
were.  Positions: an empty history, a window straddling a chunk edge at every offset, a window starting on an edge, the last rows
of the cache.  Idle groups, short groups, rows past the cache, one captured launch pair replayed while pos crosses a chunk edge, and
every refusal of the launcher on its return code."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from tests.test_draft_kernels_gpu import _bits, _case, _i32, _tables  # noqa: E402

DEV = "cuda:0"
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
T_CAP = 640
POSITIONS = lambda K, CH: [0, 1, CH - K, CH - 1, CH, CH + 1, T_CAP - K]


def _ws(G, K, H, chunk, T=T_CAP):
    return ops.attn_decode_split_draft_ws(G, K, H, T, DEV, chunk=chunk).fill_(float("nan"))


def _sequential(c, nrow, cos, sin, chunk):
    """nrow[g] sequential one-row split launches per live sequence on a copy of the cache: (out, cache after); other out rows 0."""
    cache = c["cache"].clone()
    out = torch.zeros_like(c["out"])
    part = ops.attn_decode_split_ws(1, c["H"], c["T"], DEV, chunk=chunk).fill_(float("nan"))
    for g, (p, lv, n) in enumerate(zip(c["pos"], c["live"], nrow)):
        for j in range(min(n, c["T"] - p) if lv else 0):
            r = g * c["K"] + j
            out[r] = ops.attn_decode_rope_split_rows(c["qkv"][r:r + 1], cache[g:g + 1], _i32([p + j]), _i32([p + j + 1]), _i32([1]), cos, sin,
                                                     c["H"], c["D"], c["scale"], part, chunk=chunk)[0]
    return out, cache


def _check(c, nrow, cos, sin, chunk, rows_entry):
    """One launch pair on copies of c's buffers against the sequential launches.  nrow: per group, K everywhere without rows_entry."""
    K = c["K"]
    qkv, cache = c["qkv"].clone(), c["cache"].clone()
    part = _ws(c["G"], K, c["H"], chunk, c["T"])
    args = (cos, sin, c["H"], c["D"], c["scale"], K, part)
    if rows_entry:
        out = ops.attn_decode_rope_split_draft_rows(qkv, cache, _i32(c["pos"]), _i32(c["live"]), _i32(nrow), *args, chunk=chunk, out=c["out"].clone())
    else:
        out = ops.attn_decode_rope_split_draft(qkv, cache, _i32(c["pos"]), _i32(c["live"]), *args, chunk=chunk, out=c["out"].clone())
    ref_out, ref_cache = _sequential(c, nrow, cos, sin, chunk)
    torch.cuda.synchronize()
    tag = (c["H"], c["D"], K, chunk, c["pos"], c["live"], nrow)
    assert torch.equal(_bits(qkv), _bits(c["qkv"])), tag                      # qkv is only read: q is rotated in LDS
    assert torch.equal(_bits(out), _bits(ref_out)), tag                       # a token row's bits; every other row is zeros
    assert torch.equal(_bits(cache), _bits(ref_cache)), tag                   # the appended rows' bits and nothing else
    for g, (p, lv, n) in enumerate(zip(c["pos"], c["live"], nrow)):
        rows = min(n, c["T"] - p) if lv else 0
        assert not bool(out[g * K:(g + 1) * K].isnan().any()), tag
        assert not bool(out[g * K + rows:(g + 1) * K].float().abs().max() > 0) if rows < K else True, tag
        assert not bool(cache[g, p:p + rows].isnan().any()), tag
        keep = torch.ones(c["T"], dtype=torch.bool)
        keep[p:p + rows] = False
        assert torch.equal(_bits(cache[g][keep]), _bits(c["cache"][g][keep])), tag      # rows < pos only read, the rest still NaN
        assert bool(cache[g, p + rows:].isnan().all()) if lv else bool(cache[g].isnan().all()), tag


@pytest.mark.parametrize("chunk", [128, 256, 512])
@pytest.mark.parametrize("K", [1, 2, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H", [1, 4])
def test_every_row_has_the_bits_of_sequential_one_row_split_launches(H, D, K, chunk):
    cos, sin = _tables(T_CAP, D)
    P = POSITIONS(K, chunk)
    for i, p in enumerate(P):
        _check(_case(H, D, K, [p], [1], seed=100 + i, T=T_CAP), [K], cos, sin, chunk, rows_entry=False)
        # mixed groups: an idle one in the middle, short groups on either side
        pos = [p, P[(i + 3) % len(P)], P[(i + 5) % len(P)]]
        nrow = [K, K, 1] if i % 2 else [min(2, K), K, max(1, K - 1)]
        _check(_case(H, D, K, pos, [1, 0, 1], seed=200 + i, T=T_CAP), nrow, cos, sin, chunk, rows_entry=True)
    _check(_case(H, D, K, [P[2], P[6]], [1, 1], seed=300, T=T_CAP), [K, K], cos, sin, chunk, rows_entry=False)


@pytest.mark.parametrize("chunk", [128, 512])
def test_rows_past_the_cache_are_zero_and_write_nothing(chunk):
    H, D, K = 4, 64, 4
    cos, sin = _tables(T_CAP + 8, D)
    c = _case(H, D, K, [T_CAP - 2], [1], seed=7, T=T_CAP)                     # rows 0 and 1 fit, rows 2 and 3 would leave the cache
    _check(c, [K], cos, sin, chunk, rows_entry=False)
    _check(c, [3], cos, sin, chunk, rows_entry=True)


def test_one_captured_launch_pair_replays_while_pos_crosses_a_chunk_edge():
    H, D, K, chunk = 4, 128, 4, 128
    cos, sin = _tables(T_CAP, D)
    c = _case(H, D, K, [0, 0, 0], [1, 1, 1], seed=21, T=T_CAP)
    c["cache"] = (torch.randn(3, T_CAP, 2 * H * D, generator=torch.Generator().manual_seed(22)) * 0.7).to(BF16).to(DEV)
    qkv, cache, out = c["qkv"].clone(), c["cache"].clone(), c["out"].clone()
    pos, live, nrow = _i32([0, 0, 0]), _i32([1, 1, 1]), _i32([K, K, K])
    part = _ws(3, K, H, chunk)

    def launch():
        ops.attn_decode_rope_split_draft_rows(qkv, cache, pos, live, nrow, cos, sin, H, D, c["scale"], K, part, chunk=chunk, out=out)

    launch()                                                                  # warm, then capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        launch()
    for p, lv, n in (([125, 300, 0], [1, 1, 1], [4, 4, 2]), ([126, 383, 5], [1, 1, 1], [4, 2, 4]), ([127, 384, 200], [1, 0, 1], [3, 4, 1]),
                     ([128, 255, 64], [1, 1, 1], [4, 4, 4]), ([T_CAP - K, 129, 127], [0, 1, 1], [4, 2, 4])):
        cache.copy_(c["cache"])
        out.fill_(float("nan"))
        part.fill_(float("nan"))
        pos.copy_(_i32(p))
        live.copy_(_i32(lv))
        nrow.copy_(_i32(n))
        graph.replay()
        f_cache = c["cache"].clone()
        f_out = ops.attn_decode_rope_split_draft_rows(c["qkv"], f_cache, _i32(p), _i32(lv), _i32(n), cos, sin, H, D, c["scale"], K,
                                                      _ws(3, K, H, chunk), chunk=chunk)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(f_out)) and torch.equal(_bits(cache), _bits(f_cache)), p
        assert torch.equal(_bits(qkv), _bits(c["qkv"])) and not bool(out.isnan().any()), p
        for g in range(3):
            rows = n[g] if lv[g] else 0
            keep = torch.ones(T_CAP, dtype=torch.bool)
            keep[p[g]:p[g] + rows] = False
            assert torch.equal(_bits(cache[g][keep]), _bits(c["cache"][g][keep])), (p, g)


def _raw(c, cos, sin, rows_entry=False, K=None, D=None, ld_qkv=None, T=None, chunk=128, short=0, null=None, shift=None, G=None):
    """The C entry itself: (return code, out after, cache after, qkv after, partials after)."""
    qkv, cache, out = c["qkv"].clone(), c["cache"].clone(), c["out"].clone()
    part = _ws(c["G"], c["K"], c["H"], 128, c["T"])
    t = dict(qkv=qkv, cache=cache, pos=_i32(c["pos"]), live=_i32(c["live"]), nrow=_i32([c["K"]] * c["G"]), cos=cos, sin=sin, out=out, part=part)
    p = lambda k: None if k == null else ctypes.c_void_p(t[k].data_ptr() + (2 if k == shift else 0))
    head = (p("qkv"), qkv.stride(0) if ld_qkv is None else ld_qkv, p("cache"), cache.stride(0), cache.stride(1), p("pos"), p("live"))
    tail = (p("cos"), p("sin"), p("out"), out.stride(0), p("part"), part.numel() - short, c["G"] if G is None else G,
            c["K"] if K is None else K, c["H"], c["D"] if D is None else D, c["T"] if T is None else T, chunk, c["scale"], ops._s())
    L = _lib.load()
    rc = L.mh_attn_decode_rope_split_draft_rows(*head, p("nrow"), *tail) if rows_entry else L.mh_attn_decode_rope_split_draft(*head, *tail)
    torch.cuda.synchronize()
    return rc, out, cache, qkv, part


def test_the_launcher_refuses_what_its_parents_refuse_and_launches_nothing():
    H, D, K = 2, 64, 2
    cos, sin = _tables(T_CAP, 136)
    c = _case(H, D, K, [5], [1], seed=3, T=T_CAP)
    assert _raw(c, cos, sin)[0] == 0 and _raw(c, cos, sin, rows_entry=True)[0] == 0 and _raw(c, cos, sin, chunk=0)[0] == 0
    refusals = [(dict(K=9), -3), (dict(D=136), -3), (dict(D=72), -3),                                      # MH_ERR_UNSUPPORTED
                (dict(chunk=64), -1), (dict(chunk=1024), -1), (dict(T=8200), -1), (dict(short=1), -1),     # MH_ERR_ARG
                (dict(ld_qkv=3 * H * D + 4), -1), (dict(ld_qkv=3 * H * D - 8), -1), (dict(K=0), -1), (dict(shift="qkv"), -1),
                (dict(shift="cache"), -1), (dict(shift="pos"), -1), (dict(rows_entry=True, null="nrow"), -1),
                (dict(rows_entry=True, shift="nrow"), -1)]
    refusals += [(dict(null=k), -1) for k in ("qkv", "cache", "pos", "live", "cos", "sin", "out", "part")]
    for kw, want in refusals:
        rc, out, cache, qkv, part = _raw(c, cos, sin, **kw)
        assert rc == want, (kw, rc)
        assert bool(out.isnan().all()) and bool(part.isnan().all()), kw
        assert torch.equal(_bits(cache), _bits(c["cache"])) and torch.equal(_bits(qkv), _bits(c["qkv"])), kw
    # no sequence: the answer says whether the shape is supported, and no pointer is read
    assert _raw(c, cos, sin, G=0, null="qkv")[0] == 0 and _raw(c, cos, sin, G=0, K=9)[0] == -3 and _raw(c, cos, sin, G=0, chunk=64)[0] == -1
    assert ops.attn_decode_split_draft_supported(32, 128, 8, 8192) and ops.attn_decode_split_draft_supported(32, 128, 4, 2304, 512)
    assert not ops.attn_decode_split_draft_supported(32, 128, 9, 8192) and not ops.attn_decode_split_draft_supported(32, 72, 4, 256)
    assert not ops.attn_decode_split_draft_supported(32, 128, 4, 8200) and not ops.attn_decode_split_draft_supported(32, 128, 4, 2048, 64)
    L = _lib.load()
    assert L.mh_attn_decode_split_draft_ws_floats(3, 4, 32, 1000, 128) == 3 * 4 * 32 * 8 * 132
    assert L.mh_attn_decode_split_draft_ws_floats(3, 4, 32, 1000, 0) == 3 * 4 * 32 * 8 * 132
    assert L.mh_attn_decode_split_draft_ws_floats(3, 4, 32, 1000, 100) == -1
