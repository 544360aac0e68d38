"""The split-KV decode attention with per-row state (mh_attn_decode_rope_split_rows, the decode slots' form of
mh_attn_decode_rope_split): every live row against the B = 1 split kernel bit for bit and against fp64, idle rows left alone,
no stale partial record in the output, one captured launch pair replayed while rows move, go idle and come back, and the
argument refusals.  Outputs are poisoned with NaN and the caches filled with random canaries before every launch."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
BF16 = torch.bfloat16
PSTRIDE = 132                                                        # floats per (row, head, chunk) partial record

KV_LEN = [1, 64, 128, 129, 300, 640, 257]                            # one key; half a chunk; a chunk; one past; ragged; T_cap; two + 1
IDLE = 2


def _tables(T, D):
    fr = torch.arange(T).float()[:, None] * (1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D)))[None]
    return fr.cos().contiguous(), fr.sin().contiguous()


def _rotate(x, c, s):
    """rotate-half in fp32 of a bf16 [.., D] head, rounded to bf16 once (modeling_llama.py:109-123)."""
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h].float(), x[..., h:].float()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(BF16)


def _reference(qkv, cache_after, pos, kv_len, cos, sin, H, D, scale):
    """fp64 attention of the rotated (bf16-rounded) query over the first kv_len[b] rows of the cache after the append."""
    B, W = qkv.shape[0], H * D
    out = torch.zeros((B, W), dtype=torch.float64)
    for b in range(B):
        p = int(pos[b])
        q = _rotate(qkv[b, :W].view(H, D), cos[p], sin[p]).double()
        n = int(kv_len[b])
        k = cache_after[b, :n, :W].view(n, H, D).double()
        v = cache_after[b, :n, W:].view(n, H, D).double()
        s = torch.einsum("hd,nhd->hn", q, k) * scale
        out[b] = torch.einsum("hn,nhd->hd", torch.softmax(s, -1), v).reshape(W)
    return out


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32)


def _inputs(H, D, T, kv_len, pos, live, seed):
    """CPU inputs of one case: qkv, the canary cache, the int32 state vectors, the rotary tables."""
    g = torch.Generator().manual_seed(seed)
    B, W = len(kv_len), H * D
    cos, sin = _tables(T, D)
    return dict(H=H, D=D, T=T, B=B, W=W, scale=1.0 / D ** 0.5, cos=cos, sin=sin, kv_len=_i32(kv_len), pos=_i32(pos), live=_i32(live),
                qkv=(torch.randn(B, 3 * W, generator=g) * 0.7).to(BF16), cache=(torch.randn(B, T, 2 * W, generator=g) * 0.7).to(BF16))


def _poison(shape):
    return torch.full(shape, float("nan"), dtype=BF16, device=DEV)


def _rows(c, chunk, part=None):
    """One launch of the rows entry on fresh device copies: (out, cache after, qkv after) on the CPU."""
    d = lambda t: t.to(DEV)
    if part is None:
        part = ops.attn_decode_split_ws(c["B"], c["H"], c["T"], DEV, chunk=chunk).fill_(float("nan"))
    q, cache = d(c["qkv"]), d(c["cache"])
    o = ops.attn_decode_rope_split_rows(q, cache, d(c["pos"]), d(c["kv_len"]), d(c["live"]), d(c["cos"]), d(c["sin"]), c["H"], c["D"],
                                        c["scale"], part, chunk=chunk, out=_poison((c["B"], c["W"])))
    torch.cuda.synchronize()
    return o.cpu(), cache.cpu(), q.cpu()


def _solo(c, b, chunk):
    """mh_attn_decode_rope_split at B = 1 on copies of row b's inputs, pos_dev[0] = pos[b]: (out [W], cache slice after)."""
    d = lambda t: t.to(DEV)
    q, cache = d(c["qkv"][b:b + 1].clone()), d(c["cache"][b:b + 1].clone())
    p = d(c["pos"][b:b + 1].clone())
    part = ops.attn_decode_split_ws(1, c["H"], c["T"], DEV, chunk=chunk).fill_(float("nan"))
    o = ops.attn_decode_rope_split(q, cache, p, p, d(c["kv_len"][b:b + 1].clone()), d(c["cos"]), d(c["sin"]), c["H"], c["D"], c["scale"],
                                   part, chunk=chunk, out=_poison((1, c["W"])))
    torch.cuda.synchronize()
    return o.cpu()[0], cache.cpu()[0]


@functools.lru_cache(maxsize=None)
def _case(H, D, T, chunk, variant):
    """The inputs and the rows launch of one case, computed once for the tests that read it.  "edge": pos[b] = kv_len[b] - 1 on
    seven rows, row 2 idle.  "past": two live rows whose new row lies at or past kv_len[b] -- written, not attended -- in the last
    attended chunk (row 3) and in a chunk no key of the row is in (row 4); the B = 1 kernel defines both."""
    kv_len = [min(n, T) for n in KV_LEN]                             # the kernel sees at most T_cap keys; the host keeps pos below it
    pos = [n - 1 for n in kv_len]
    if variant == "past":
        pos[3], pos[4] = min(200, T - 1), min(400, T - 1)
    live = [int(b != IDLE) for b in range(len(kv_len))]
    c = _inputs(H, D, T, kv_len, pos, live, seed=H * 131 + D + chunk + len(variant))
    c["out"], c["cache_after"], c["qkv_after"] = _rows(c, chunk)
    return c


CASES = [(2, 16, 640, 128, "edge"), (3, 64, 640, 128, "edge"), (3, 64, 640, 128, "past"), (3, 64, 640, 256, "edge"),
         (2, 16, 640, 512, "edge"), (32, 128, 384, 128, "edge")]


@pytest.mark.parametrize("H,D,T,chunk,variant", CASES)
def test_every_live_row_has_the_solo_split_kernels_bits_and_an_idle_row_is_left_alone(H, D, T, chunk, variant):
    c = _case(H, D, T, chunk, variant)
    out, cache, B = c["out"], c["cache_after"], c["B"]
    assert torch.equal(c["qkv_after"], c["qkv"])                     # read only, every row (the non-split rows kernel rotates q)
    for b in range(B):
        p = int(c["pos"][b])
        others = torch.ones(T, dtype=torch.bool)
        others[p] = False
        assert torch.equal(cache[b][others], c["cache"][b][others]), b       # every row but pos[b], past kv_len too
        if b == IDLE:
            assert not bool(out[b].float().ne(0).any()) and not bool(out[b].isnan().any())      # zeros over the poison
            assert torch.equal(cache[b], c["cache"][b])
            continue
        o1, c1 = _solo(c, b, chunk)
        assert torch.equal(out[b].view(torch.int16), o1.view(torch.int16)), b
        assert torch.equal(cache[b].view(torch.int16), c1.view(torch.int16)), b
        assert not torch.equal(cache[b][p], c["cache"][b][p])        # the new row was written


@pytest.mark.parametrize("H,D,T,chunk,variant", CASES)
def test_live_rows_stay_within_the_split_kernels_fp64_bound(H, D, T, chunk, variant):
    """The bound of the split kernel's own test at these key counts: half a bf16 ulp of the value (2^-9 relative, 2^-8 allowed)
    plus fp32 accumulation over at most 640 keys."""
    c = _case(H, D, T, chunk, variant)
    ref = _reference(c["qkv"], c["cache_after"], c["pos"], c["kv_len"], c["cos"], c["sin"], H, D, c["scale"])
    for b in range(c["B"]):
        if b == IDLE:
            continue
        err = (c["out"][b].double() - ref[b]).abs()
        bound = ref[b].abs() * 2.0 ** -8 + 1e-4
        print(f"row {b} kv_len {int(c['kv_len'][b])}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (b, float((err - bound).max()))


@pytest.mark.parametrize("H,D,T,chunk", [(3, 64, 640, 128), (2, 16, 640, 256)])
def test_two_launches_agree_and_no_stale_or_unwritten_record_reaches_out(H, D, T, chunk):
    c = _case(H, D, T, chunk, "edge")
    part = ops.attn_decode_split_ws(c["B"], H, T, DEV, chunk=chunk)
    runs = []
    for _ in range(2):
        part.fill_(float("nan"))                                     # whatever the last launch left is gone
        runs.append(_rows(c, chunk, part))
    for x, y in zip(*runs):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))
    # NaN exactly where no workgroup of this launch writes: the idle row's records and every chunk at or past kv_len[b]
    rec = part.view(c["B"] * H, -1, PSTRIDE)
    assert rec.shape[1] == (T + chunk - 1) // chunk
    for b in range(c["B"]):
        used = 0 if b == IDLE else (int(c["kv_len"][b]) + chunk - 1) // chunk
        rec[b * H:(b + 1) * H, used:] = float("nan")
    again = _rows(c, chunk, part)
    for x, y in zip(runs[0], again):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))
    live = [b for b in range(c["B"]) if b != IDLE]
    assert not bool(again[0][live].isnan().any())
    assert torch.equal(again[0].view(torch.int16), c["out"].view(torch.int16))       # and the shared case's launch


def test_one_captured_launch_pair_replays_while_rows_move_go_idle_and_come_back():
    torch.manual_seed(11)
    B, H, D, T, chunk = 3, 3, 64, 640, 128
    W = H * D
    cos, sin = (t.to(DEV) for t in _tables(T, D))
    cache = (torch.randn(B, T, 2 * W, device=DEV) * 0.7).to(BF16)
    qkv = (torch.randn(B, 3 * W, device=DEV) * 0.7).to(BF16)
    pos, kvl, live = (torch.zeros((B,), dtype=torch.int32, device=DEV) for _ in range(3))
    part = ops.attn_decode_split_ws(B, H, T, DEV, chunk=chunk)
    part2 = torch.empty_like(part)
    out = _poison((B, W))
    step = lambda c, o, p: ops.attn_decode_rope_split_rows(qkv, c, pos, kvl, live, cos, sin, H, D, 0.125, p, chunk=chunk, out=o)

    def state(kv_len, alive):
        kvl.copy_(_i32(kv_len))
        pos.copy_(_i32([n - 1 for n in kv_len]))
        live.copy_(_i32(alive))

    state((5, 6, 7), (1, 1, 1))
    step(cache, out, part)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(cache, out, part)
    moves = [((10, 200, 127), (1, 1, 1)), ((128, 256, 1), (1, 1, 1)), ((129, 640, 300), (1, 1, 1)),   # each row through its own lengths
             ((130, 640, 301), (1, 0, 1)), ((131, 400, 302), (1, 1, 1))]                              # row 1 idle, then live again
    for kv_len, alive in moves:
        state(kv_len, alive)
        before = cache.clone()
        out.fill_(float("nan"))
        g.replay()
        eager_c = before.clone()
        eager_o = step(eager_c, _poison((B, W)), part2.fill_(float("nan")))
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), eager_o.view(torch.int16)), kv_len
        assert torch.equal(cache, eager_c), kv_len
        for b in range(B):
            if alive[b]:
                assert not bool(out[b].isnan().any()) and not torch.equal(cache[b, kv_len[b] - 1], before[b, kv_len[b] - 1])
            else:
                assert not bool(out[b].float().ne(0).any()) and torch.equal(cache[b], before[b])


def test_refusals():
    def call(H=2, D=16, T=128, B=2, chunk=128, part=None, cache_rows=None, live_dtype=torch.int32, short=0):
        W = H * D
        cos, sin = (t.to(DEV) for t in _tables(16, D))
        qkv = torch.zeros((B, 3 * W), dtype=BF16, device=DEV)
        cache = torch.zeros((B if cache_rows is None else cache_rows, T, 2 * W), dtype=BF16, device=DEV)
        z = torch.zeros((B,), dtype=torch.int32, device=DEV)
        if part is None:
            n = B * H * ((T + 127) // 128) * PSTRIDE                 # enough for every chunk size
            part = torch.zeros((n - short,), dtype=torch.float32, device=DEV)
        return ops.attn_decode_rope_split_rows(qkv, cache, z, z + 1, torch.ones((B,), dtype=live_dtype, device=DEV), cos, sin, H, D, 0.25,
                                               part, chunk=chunk)

    call()                                                           # the base arguments are accepted
    torch.cuda.synchronize()
    for kw in (dict(D=12), dict(H=1, D=8, T=8192 + 64, B=1), dict(short=1), dict(chunk=64)):
        with pytest.raises(_lib.MyriadHipError, match="MH_ERR_ARG"):
            call(**kw)
    with pytest.raises(_lib.MyriadHipError, match="cache"):
        call(cache_rows=3)
    with pytest.raises(_lib.MyriadHipError, match="live"):
        call(live_dtype=torch.int64)
    torch.cuda.synchronize()
