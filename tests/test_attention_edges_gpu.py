"""The attention kernels at their edges against fp64 autograd-free references (tests/fp64_bounds.py: attn_ref_bound), element
by element, with every output and scratch the wrappers allocate poisoned (and dq / dk / dv passed as poisoned buffers):
sequence lengths on both sides of the fragment (16), chunk (32) and tile (64) boundaries, ragged kv_len per batch row next to
those boundaries, positions offset per batch, a late score spike (the running max jumps), keys and values past kv_len set to
+-1e4 (a mask off by one changes the answer decisively).

Padded rows (queries >= kv_len): the forward's value there is the causal value of the keys < kv_len (finite, within the
bound); with dout zero there -- what the model feeds -- dq, dk and dv rows >= kv_len are exactly 0.0, because the qkv dgrad GEMM
and the LoRA weight gradients sum over every row.  Columns of a wider qkv / dqkv row that the kernels do not own stay untouched."""
import pytest
import torch

from myriad_amd import ops
from tests import fp64_bounds as fb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


_rnd = fb.rnd


def _option(name, value):
    return fb.lib_options(**{name: value})


def _heads(t, B, S, H, D):
    return t.reshape(B, S, H, D).transpose(1, 2)


def _tok(t):
    B, H, S, D = t.shape
    return t.transpose(1, 2).reshape(B, S, H * D)


def _rope_tables(D):
    return fb.rope_tables(D, device=DEV)


def _pad_rows(x3, kv_len, value):
    """Rows >= kv_len[b] of a [B, S, C] view set to +-value (alternating sign by column)."""
    S, C = x3.shape[1], x3.shape[2]
    sign = torch.where(torch.arange(C, device=x3.device) % 2 == 0, 1.0, -1.0)
    for b, n in enumerate(kv_len.tolist()):
        if n < S:
            x3[b, n:] = (value * sign).to(x3.dtype)


def _tokens_then_padding(B, S, C, seed):
    """Dense bf16 [B, S, C] (batches back to back) followed by 8 rows of +-1e4: a read past the last batch's S is decisive."""
    flat = _rnd(B * S + 8, C, seed=seed).to(BF16).to(DEV)
    _pad_rows(flat[None], torch.tensor([B * S]), 1e4)
    return flat[:B * S].view(B, S, C)


def _padded_rows(B, S, C, extra, seed):
    """bf16 [B, S, C] view of a [B, S + extra, C] buffer whose rows past S are +-1e4: an over-read past S is decisive."""
    buf = _rnd(B, S + extra, C, seed=seed).to(BF16).to(DEV)
    _pad_rows(buf, torch.full((B,), S), 1e4)
    return buf[:, :S]


def _out_window(B, S, W):
    return fb.out_window(B, S, W, DEV)


_check_outside = fb.check_outside


def _check_grads(r, got, valid_q, valid_k, what, tol_map=None):
    for nm, g, valid in zip(("dq", "dk", "dv"), got, (valid_q, valid_k, valid_k)):
        ref, bnd = r[nm], r[nm + "_bound"]
        if tol_map is not None and nm in tol_map:
            ref, bnd = tol_map[nm]
        fb.assert_within(g, _tok(ref), _tok(bnd), f"{what} {nm}")
        if valid is not None:
            pad = g[~valid]
            assert bool((pad == 0).all()), f"{what} {nm}: padded rows not exactly zero (max |.| {float(pad.abs().max())})"


# ----------------------------------------------------------------------------------------------- fused rotary attention
def _rope_case(B, H, S, kv, monkeypatch, split, via_gemm=None):
    D, W = 128, H * 128
    ld = 3 * W + 64                                        # the LoRA-bordered qkv row: 64 columns the kernels do not own
    kv_len = torch.tensor(kv, dtype=torch.int32, device=DEV)
    qkv = _tokens_then_padding(B, S, ld, 100 + S)
    _pad_rows(qkv[:, :, W:3 * W], kv_len, 1e4)
    spike = kv[0] - 2
    if spike > 0:
        qkv[0, spike, W:2 * W] = (qkv[0, spike, W:2 * W].float() * 4).to(BF16)
    cos, sin = _rope_tables(D)
    pos = (torch.arange(S)[None] + 7 * torch.arange(B)[:, None]).to(torch.int32).to(DEV)
    scale = D ** -0.5
    with fb.poisoned_allocations(monkeypatch):
        o, lse = ops.attn_rope_fwd(qkv, H, D, scale, pos.view(-1), cos, sin, kv_len=kv_len)
    pl = pos.long()
    q, k, v = (_heads(qkv[:, :, i * W:(i + 1) * W].float(), B, S, H, D) for i in range(3))
    qr, qe = fb.rope_bf16(q, pl, cos, sin)
    kr, ke = fb.rope_bf16(k, pl, cos, sin)
    fb.assert_rope_exempt_share(qe, "q"), fb.assert_rope_exempt_share(ke, "k")
    valid = torch.arange(S, device=DEV)[None] < kv_len[:, None]
    dout = _rnd(B, S, W, seed=7).to(BF16).to(DEV) * valid[..., None]
    if via_gemm is not None:                               # dO = a bw^T inside mh_gemm_attn_rope_bwd
        Kd = via_gemm
        a = _rnd(B * S, Kd, seed=8, scale=0.5).to(BF16).to(DEV) * valid.reshape(-1, 1)
        bw = _rnd(W, Kd, seed=9, scale=0.05).to(BF16).to(DEV)
        kern, splits = ops.gemm_plan(B * S, W, Kd, out_f32=True)
        sbf = splits > 1 and kern in (2, 4, 5) and W % 8 == 0
        dO64, e_dO = fb.gemm_ref_bound(a, bw, out_bf16=True, splits=splits, bf16_slabs=sbf)
        dout_h, dout_err = _heads(dO64.reshape(B, S, W), B, S, H, D), _heads(e_dO.reshape(B, S, W), B, S, H, D)
    else:
        dout_h, dout_err = _heads(dout.float(), B, S, H, D), None
    mask = fb.attn_mask(B, S, S, True, kv_len, DEV)
    # the backward is checked as a function of what it reads: this o and lse (themselves within their bounds just below)
    r = fb.attn_ref_bound(qr, kr, v, scale, mask, q_err=qe, k_err=ke, dout=dout_h, dout_err=dout_err,
                          o_in=_heads(o.float(), B, S, H, D), lse_in=lse)
    fb.assert_within(o, _tok(r["o"]), _tok(r["o_bound"]), f"S={S} o")
    fb.assert_within(lse, r["lse"], r["lse_bound"], f"S={S} lse")
    with _option("attn_bwd_split", split):
        ops.ensure_workspace(torch.device(DEV)).fill_(255)
        with fb.poisoned_allocations(monkeypatch):
            if via_gemm is not None:
                dqkv = ops.gemm_attn_rope_bwd(a, bw, qkv, o, lse, H, D, scale, pos.view(-1), cos, sin, kv_len=kv_len)
            else:
                dqkv = ops.attn_rope_bwd(qkv, o, dout, lse, H, D, scale, pos.view(-1), cos, sin, kv_len=kv_len)
    fb.assert_untouched(dqkv[:, :, 3 * W:], f"S={S} dqkv border columns")
    # dq, dk leave the kernel un-rotated (fp32, then one rounding): R^T of the gradients w.r.t. the rotated operands, the
    # accumulation bounds mapped through |R^T|
    un = {}
    for nm in ("dq", "dk"):
        g64 = fb.rope64(r[nm], pl, cos.double(), sin.double(), sign=-1.0)
        e = (fb.rope_abs_map(r[nm + "_bound_acc"], pl, cos.double(), sin.double())
             + 4 * fb.U32 * fb.rope_abs_map(r[nm].abs(), pl, cos.double(), sin.double()))
        un[nm] = (g64, e + fb.U16 * (g64.abs() + e))
    got = [dqkv[:, :, i * W:(i + 1) * W] for i in range(3)]
    _check_grads(r, got, valid, valid, f"S={S} split={split}", un)


ROPE_CASES = [  # B, H, S, kv_len per batch row
    (2, 2, 1, [1, 1]),
    (2, 2, 2, [2, 1]),
    (3, 2, 15, [15, 1, 14]),
    (2, 2, 16, [16, 15]),
    (3, 2, 17, [17, 16, 1]),
    (2, 2, 31, [31, 17]),
    (2, 2, 32, [32, 31]),
    (3, 2, 33, [33, 32, 16]),
    (3, 2, 144, [144, 143, 17]),
    (2, 2, 159, [158, 15]),
    (3, 2, 160, [160, 159, 16]),
]


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("B,H,S,kv", ROPE_CASES, ids=[f"S{c[2]}" for c in ROPE_CASES])
def test_attn_rope_fwd_bwd_edges(B, H, S, kv, split, monkeypatch):
    """attn_seq.hip forward and backward (attn_bwd_split 0: one workgroup per (b, h), 1: two), S = 1 included."""
    assert ops.attn_rope_supported(S, 128)
    _rope_case(B, H, S, kv, monkeypatch, split)


@pytest.mark.parametrize("B,H,S,kv,K", [(1, 32, 148, [131], 4096), (2, 2, 100, [100, 63], 256)], ids=["split", "unsplit"])
def test_gemm_attn_rope_bwd_edges(B, H, S, kv, K, monkeypatch):
    """The o_proj dgrad fused into the rotary attention backward: dO's slabs (split) or bf16 matrix (unsplit) summed inside."""
    ops.ensure_workspace(torch.device(DEV))
    splits = ops.gemm_plan(B * S, H * 128, K, out_f32=True)[1]
    assert (splits > 1) == (K == 4096)
    _rope_case(B, H, S, kv, monkeypatch, 1, via_gemm=K)


@pytest.mark.parametrize("S,kv", [(161, [161, 64]), (200, [129, 200]), (300, [257, 1])])
def test_long_sequence_fallback_rope_then_tiled_attention(S, kv, monkeypatch):
    """Past the fused kernel's 160 rows the model runs rope_ on q | k, then causal attn_fwd / attn_bwd with kv_len."""
    B, H, D = 2, 2, 128
    W = H * D
    assert not ops.attn_rope_supported(S, D)
    kv_len = torch.tensor(kv, dtype=torch.int32, device=DEV)
    qkv = _tokens_then_padding(B, S, 3 * W, 200 + S)
    _pad_rows(qkv[:, :, W:], kv_len, 1e4)
    cos, sin = _rope_tables(D)
    pos = (torch.arange(S)[None] + 5 * torch.arange(B)[:, None]).to(torch.int32).to(DEV)
    raw = qkv.clone()
    ops.rope_(qkv.view(B * S, 3 * W), 0, 2 * H, D, pos.view(-1), cos, sin, 1.0)
    q, k, v = qkv[:, :, :W], qkv[:, :, W:2 * W], qkv[:, :, 2 * W:]
    scale = D ** -0.5
    valid = torch.arange(S, device=DEV)[None] < kv_len[:, None]
    dout = _rnd(B, S, W, seed=11).to(BF16).to(DEV) * valid[..., None]
    with fb.poisoned_allocations(monkeypatch):
        o, lse = ops.attn_fwd(q, k, v, H, D, scale, causal=True, kv_len=kv_len)
        bufs = [_out_window(B, S, W) for _ in range(3)]
        dq, dk, dv = (w for _, w in bufs)
        ops.attn_bwd(q, k, v, o, dout, lse, H, D, scale, causal=True, kv_len=kv_len, dq=dq, dk=dk, dv=dv)
    for (buf, _), nm in zip(bufs, ("dq", "dk", "dv")):
        _check_outside(buf, S, W, f"S={S} {nm}")
    pl = pos.long()
    r = fb.attn_ref_bound(_heads(q.float(), B, S, H, D), _heads(k.float(), B, S, H, D), _heads(v.float(), B, S, H, D), scale,
                          fb.attn_mask(B, S, S, True, kv_len, DEV), dout=_heads(dout.float(), B, S, H, D),
                          o_in=_heads(o.float(), B, S, H, D), lse_in=lse)
    fb.assert_within(o, _tok(r["o"]), _tok(r["o_bound"]), f"S={S} o")
    fb.assert_within(lse, r["lse"], r["lse_bound"], f"S={S} lse")
    _check_grads(r, (dq, dk, dv), valid, valid, f"S={S}")
    # the rotation itself against fp64 (one rounding)
    for nm, got in (("q", q), ("k", k)):
        x64 = _heads(raw[:, :, :W] if nm == "q" else raw[:, :, W:2 * W], B, S, H, D).double()
        rot64 = fb.rope64(x64, pl, cos.double(), sin.double())
        e = 4 * fb.U32 * fb.rope_abs_map(x64.abs(), pl, cos.double(), sin.double())
        fb.assert_within(_heads(got, B, S, H, D), rot64, fb.U16 * (rot64.abs() + e) + e, f"rope_ {nm}")


# ------------------------------------------------------------------------------------------------------ tiled kernels
TILED = [  # B, H, Sq, Sk, D, causal, kv_len (None: all keys)
    (2, 2, 63, 63, 64, True, [63, 40]),
    (2, 2, 64, 64, 88, True, [64, 63]),
    (2, 2, 65, 65, 128, True, [65, 64]),
    (2, 2, 127, 129, 64, True, [129, 65]),
    (2, 1, 128, 128, 88, False, [128, 127]),
    (2, 2, 129, 129, 128, True, [129, 128]),
    (1, 2, 257, 257, 64, True, [193]),
    (2, 2, 1, 63, 128, True, [63, 1]),
    (2, 2, 1, 129, 88, False, [129, 64]),
    (2, 2, 64, 257, 128, False, None),
    (1, 2, 63, 128, 64, True, None),
    (2, 2, 129, 65, 88, False, [65, 1]),
]


@pytest.mark.parametrize("B,H,Sq,Sk,D,causal,kv", TILED)
def test_tiled_attention_fwd_bwd_edges(B, H, Sq, Sk, D, causal, kv, monkeypatch):
    """attention.hip with option attn_full = 0: the 64 x 64 tiles, except that the Sq = 1 rows' forward is its KV-cache decode
    kernel (attn_decode_kernel: mh_attn_fwd takes it for Sq == 1 without bias); the backward is the tiled dq and dk / dv
    kernels throughout.  o, lse, dq / dk / dv against fp64; Sq, Sk, kv_len on and next to the tile boundaries, causal with
    Sq < Sk, q / k / v as views of wider rows with 8 rows of +-1e4 past Sk (and past kv_len) in every batch."""
    W = H * D
    kv_len = None if kv is None else torch.tensor(kv, dtype=torch.int32, device=DEV)
    qbuf = _padded_rows(B, Sq, W + 16, 8, 300 + Sq)
    kvbuf = _padded_rows(B, Sk, 2 * W + 8, 8, 301 + Sk)
    if kv_len is not None:
        _pad_rows(kvbuf[:, :, :2 * W], kv_len, 1e4)
    q, k, v = qbuf[:, :, :W], kvbuf[:, :, :W], kvbuf[:, :, W:2 * W]
    scale = D ** -0.5
    valid_q = None
    if kv_len is not None and Sq == Sk:
        valid_q = torch.arange(Sq, device=DEV)[None] < kv_len[:, None]
    dout = _rnd(B, Sq, W, seed=12).to(BF16).to(DEV)
    if valid_q is not None:
        dout = dout * valid_q[..., None]
    with _option("attn_full", 0), fb.poisoned_allocations(monkeypatch):
        o, lse = ops.attn_fwd(q, k, v, H, D, scale, causal=causal, kv_len=kv_len)
        bufs = [_out_window(B, Sq, W), _out_window(B, Sk, W), _out_window(B, Sk, W)]
        dq, dk, dv = (w for _, w in bufs)
        ops.attn_bwd(q, k, v, o, dout, lse, H, D, scale, causal=causal, kv_len=kv_len, dq=dq, dk=dk, dv=dv)
    for (buf, _), nm, S in zip(bufs, ("dq", "dk", "dv"), (Sq, Sk, Sk)):
        _check_outside(buf, S, W, nm)
    mask = fb.attn_mask(B, Sq, Sk, causal, kv_len, DEV)
    h = lambda t, S: _heads(t.float(), B, S, H, D)            # noqa: E731
    r = fb.attn_ref_bound(h(q, Sq), h(k, Sk), h(v, Sk), scale, mask, dout=h(dout, Sq), o_in=h(o, Sq), lse_in=lse)
    what = f"{Sq}x{Sk} D={D}"
    fb.assert_within(o, _tok(r["o"]), _tok(r["o_bound"]), what + " o")
    fb.assert_within(lse, r["lse"], r["lse_bound"], what + " lse")
    valid_k = None if kv_len is None else torch.arange(Sk, device=DEV)[None] < kv_len[:, None]
    _check_grads(r, (dq, dk, dv), valid_q, valid_k, what)


def _kernels_run(fn):
    """Names of the device kernels fn() launches (torch.profiler's device trace: every launch of the process, the library's
    included)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}


@pytest.mark.parametrize("Sq,Sk,D", [(32, 1, 40), (81, 31, 64), (7, 32, 88), (32, 33, 40), (81, 287, 88), (100, 288, 64),
                                     (33, 289, 88)])
def test_attn_full_edges_and_the_tiled_form(Sq, Sk, D, monkeypatch):
    """attn_full.hip (all keys of an (image, head) staged at once) at key counts on both sides of its 32-key steps and its 288
    limit; Sk = 289 takes the tiled path.  Both settings of option attn_full give o and lse within the fp64 bound, and the
    device trace shows which kernel ran: attn_full_fwd_kernel for option 1 up to 288 keys (its launcher falls back to the
    tiles silently when it refuses a layout), attn_fwd_kernel otherwise."""
    B, H = 2, 3
    W = H * D
    qbuf = _padded_rows(B, Sq, 3 * W + 16, 8, 400 + Sk)
    kvbuf = _padded_rows(B, Sk, 2 * W, 8, 401 + Sk)
    q, k, v = qbuf[:, :, :W], kvbuf[:, :, :W], kvbuf[:, :, W:]
    scale = D ** -0.5
    h = lambda t, S: _heads(t.float(), B, S, H, D)            # noqa: E731
    r = fb.attn_ref_bound(h(q, Sq), h(k, Sk), h(v, Sk), scale, fb.attn_mask(B, Sq, Sk, False, None, DEV))
    outs = []
    for full in (1, 0):
        res = {}
        with _option("attn_full", full), fb.poisoned_allocations(monkeypatch):
            names = _kernels_run(lambda: res.update(out=ops.attn_fwd(q, k, v, H, D, scale)))
        o, lse = res["out"]
        want = "attn_full_fwd_kernel" if full and Sk <= 288 else "attn_fwd_kernel"
        assert any(want in n for n in names), f"attn_full={full} Sk={Sk}: expected {want}, the device ran {sorted(names)}"
        fb.assert_within(o, _tok(r["o"]), _tok(r["o_bound"]), f"attn_full={full} o")
        fb.assert_within(lse, r["lse"], r["lse_bound"], f"attn_full={full} lse")
        outs.append(o)
    if Sk == 289:
        assert torch.equal(outs[0], outs[1]), "past 288 keys both settings run the tiled kernel"


# ------------------------------------------------------------------------------------------------------------- decode
def test_attn_decode_rope_per_row_positions_and_lengths(monkeypatch):
    """mh_attn_decode_rope (one decode token, single workgroup per (b, h)): q and the new k rotated at each row's own position,
    k | v appended at cache row pos_dev[0], the query attending kv_len[b] cached keys (a different count per row; rows past it
    +-1e4).  The output, the rotated q written back and the appended cache row against fp64; every other cache row and the
    k / v columns of qkv unchanged."""
    B, H, D, T = 3, 4, 128, 200
    W = H * D
    pos_b, kv_b, app = [5, 63, 130], [65, 128, 200], 64
    qkv = _rnd(B, 3 * W + 64, seed=500).to(BF16).to(DEV)
    cache = _rnd(B, T, 2 * W, seed=501).to(BF16).to(DEV)
    kv_len = torch.tensor(kv_b, dtype=torch.int32, device=DEV)
    _pad_rows(cache, kv_len, 1e4)
    pos = torch.tensor(pos_b, dtype=torch.int32, device=DEV)
    pos_dev = torch.tensor([app], dtype=torch.int32, device=DEV)
    cos, sin = _rope_tables(D)
    scale = D ** -0.5
    qkv0, cache0 = qkv.clone(), cache.clone()
    with fb.poisoned_allocations(monkeypatch):
        out = ops.attn_decode_rope(qkv, cache, pos, pos_dev, kv_len, cos, sin, H, D, scale)
    pl = pos.long()[:, None]
    q = qkv0[:, :W].float().view(B, 1, H, D).transpose(1, 2)
    knew = qkv0[:, W:2 * W].float().view(B, 1, H, D).transpose(1, 2)
    qr, qe = fb.rope_bf16(q, pl, cos, sin)
    kr_new, ke_new = fb.rope_bf16(knew, pl, cos, sin)
    fb.assert_rope_exempt_share(qe, "q"), fb.assert_rope_exempt_share(ke_new, "appended k")
    fb.assert_within(qkv[:, :W].view(B, 1, H, D).transpose(1, 2), qr, qe, "q rotated in place")
    assert torch.equal(qkv[:, W:], qkv0[:, W:]), "k / v columns and the border of qkv must not change"
    fb.assert_within(cache[:, app, :W].view(B, 1, H, D).transpose(1, 2), kr_new, ke_new, "appended k")
    assert torch.equal(cache[:, app, W:], qkv0[:, 2 * W:3 * W]), "appended v"
    rows = torch.ones(T, dtype=torch.bool)
    rows[app] = False
    assert torch.equal(cache[:, rows], cache0[:, rows]), "cache rows other than pos_dev[0] changed"
    k = cache0[:, :, :W].float().view(B, T, H, D).transpose(1, 2).double()
    ke = torch.zeros_like(k)
    k[:, :, app], ke[:, :, app] = kr_new[:, :, 0], ke_new[:, :, 0]
    v = cache[:, :, W:].float().view(B, T, H, D).transpose(1, 2)
    r = fb.attn_ref_bound(qr, k, v, scale, fb.attn_mask(B, 1, T, False, kv_len, DEV), q_err=qe, k_err=ke)
    fb.assert_within(out.view(B, 1, H, D).transpose(1, 2), r["o"], r["o_bound"], "decode o")
