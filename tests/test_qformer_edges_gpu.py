"""The kernels that exist only for training the Q-Former (freeze_qformer: False, qformer_dropout > 0) and for the ViT fine-tune,
at their edges against fp64 (tests/fp64_bounds.py), element by element: the DROP instances of the tiled attention kernels
(mh_attn_fwd_dropout / mh_attn_bwd_dropout, every head-dimension instance), the LayerNorms with hidden dropout fused in
(mh_layernorm_fwd_dropout / mh_layernorm_bwd_dropout) and the TN weight-gradient GEMM (mh_gemm_tn_wgrad).

Every dropout mask is fb.keep_mask_ref, the integer restatement of the hash, never the library's own mask kernel.  Every output
and scratch buffer a wrapper allocates starts poisoned; every buffer the tests pass in is a window of a poisoned (outputs) or
+-1e4-filled (operands) parent, whose frame must stay untouched and whose over-read is decisive.  A rejected call leaves its
outputs untouched.

The threshold is 1.0 of the derived bound throughout.  Worst err / bound measured on an MI355X (python -m pytest -s prints
the RATIO lines; records, not thresholds):
    attn_bwd_dropout dk bf16 DP=128             0.547
    attn_bwd_dropout dk bf16 DP=64              0.88
    attn_bwd_dropout dk bf16 DP=96              0.556
    attn_bwd_dropout dq bf16 DP=128             0.518
    attn_bwd_dropout dq bf16 DP=64              0.777
    attn_bwd_dropout dq bf16 DP=96              0.566
    attn_bwd_dropout dv bf16 DP=128             0.529
    attn_bwd_dropout dv bf16 DP=64              0.83
    attn_bwd_dropout dv bf16 DP=96              0.5
    attn_fwd_dropout lse f32 DP=128             0.0934
    attn_fwd_dropout lse f32 DP=64              0.166
    attn_fwd_dropout lse f32 DP=96              0.101
    attn_fwd_dropout o bf16 DP=128              0.408
    attn_fwd_dropout o bf16 DP=64               0.648
    attn_fwd_dropout o bf16 DP=96               0.48
    gemm_tn_wgrad bias f32                      0.0668
    gemm_tn_wgrad bias f32 accumulate           0.16
    gemm_tn_wgrad out f32                       0.565
    gemm_tn_wgrad out f32 accumulate            0.982
    layernorm_bwd_dropout dx f32                0.122
    layernorm_bwd_dropout dz bf16               0.995
    layernorm_fwd_dropout x f32                 0.498
    layernorm_fwd_dropout y bf16                0.995
    layernorm_fwd_dropout y f32                 0.32
Outputs rounded to bf16 reach ~1.0 by construction where nothing but the output's own half-ulp is left of the bound (the
LayerNorm's bf16 twins of an fp32 output at 0.32 and below), and so does an accumulate form where the earlier value dwarfs what
is added (the bound is then the half-ulp of that one sum).
"""
import pytest
import torch

from myriad_amd import _lib, ops
from tests import fp64_bounds as fb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
WORST = {}


def note(name, ratio):
    """Record a kernel output's err / bound (the docstring's table)."""
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))
    print(f"RATIO {name} {ratio:.3g} (worst so far {WORST[name]:.3g})")


def _big(rows, cols):
    """bf16 [rows, cols] of +-1e4, the sign alternating by column."""
    sign = torch.where(torch.arange(cols) % 2 == 0, 1.0, -1.0)
    return (1e4 * sign).to(BF16).expand(rows, cols).clone()


# -------------------------------------------------------------------------------------------------------- attention dropout
def _heads(t, B, S, H, D):
    return t.float().reshape(B, S, H, D).transpose(1, 2)


def _tok(t):
    B, H, S, D = t.shape
    return t.transpose(1, 2).reshape(B, S, H * D)


def _padded_rows(B, S, C, seed):
    """bf16 [B, S + 8, C] whose rows past S are +-1e4: an over-read past S is decisive."""
    buf = fb.rnd(B, S + 8, C, seed=seed).to(BF16)
    buf[:, S:] = _big(8, C)
    return buf.to(DEV)


def _attn_operands(B, H, Sq, Sk, D):
    """q, k, v as column windows of wider rows: one fused [q | k | v] buffer when Sq == Sk (the self-attention's qkv), else q
    from [B, Sq + 8, W + 16] and k | v from one [B, Sk + 8, 2 W + 8] buffer (the cross-attention's ckv)."""
    W = H * D
    if Sq == Sk:
        qkv = _padded_rows(B, Sq, 3 * W + 8, 600 + Sq)
        return qkv[:, :Sq, :W], qkv[:, :Sq, W:2 * W], qkv[:, :Sq, 2 * W:3 * W]
    qb, kvb = _padded_rows(B, Sq, W + 16, 600 + Sq), _padded_rows(B, Sk, 2 * W + 8, 601 + Sk)
    return qb[:, :Sq, :W], kvb[:, :Sk, :W], kvb[:, :Sk, W:2 * W]


ATTN_SEED = 0x3C5A7E1F90B2D486
ATTN_CASES = [  # B, H, Sq, Sk, D, p, seed
    (2, 3, 32, 257, 64, 0.1, ATTN_SEED),                 # the model's cross-attention
    (2, 3, 32, 32, 64, 0.1, ATTN_SEED),                  # the self-attention
    (2, 3, 81, 81, 64, 0.5, ATTN_SEED),
    (2, 3, 63, 65, 40, 0.5, ATTN_SEED),                  # D < DP
    (1, 2, 64, 64, 88, 0.1, ATTN_SEED),                  # DP = 96
    (2, 2, 65, 63, 128, 0.1, ATTN_SEED),                 # DP = 128
    (2, 3, 1, 31, 64, 0.5, ATTN_SEED),                   # the dropout forward has no Sq = 1 detour
    (2, 3, 129, 1, 64, 0.1, ATTN_SEED),
    (1, 3, 81, 129, 64, 0.1, ATTN_SEED | (1 << 63)),     # bit 63 of the seed: the second draw
]


@pytest.mark.parametrize("B,H,Sq,Sk,D,p,seed", ATTN_CASES, ids=[f"{c[2]}x{c[3]}-D{c[4]}-p{c[5]}" for c in ATTN_CASES])
def test_attention_dropout_fwd_bwd_edges(B, H, Sq, Sk, D, p, seed, monkeypatch):
    """o, lse, dq, dk, dv of the DROP instances against attn_ref_bound(keep=...): the backward as a function of the o and lse
    it is handed.  B = 2 and H = 3 so that a dropped b or h term of the mask index shows."""
    W = H * D
    q, k, v = _attn_operands(B, H, Sq, Sk, D)
    dout = fb.rnd(B, Sq, W, seed=12).to(BF16).to(DEV)
    scale = D ** -0.5
    with fb.lib_options(attn_full=0), fb.poisoned_allocations(monkeypatch):
        o, lse = ops.attn_fwd_dropout(q, k, v, H, D, scale, p, seed)
        bufs = [fb.out_window(B, Sq, W, DEV), fb.out_window(B, Sk, W, DEV), fb.out_window(B, Sk, W, DEV)]
        dq, dk, dv = (w for _, w in bufs)
        ops.attn_bwd_dropout(q, k, v, o, dout, lse, H, D, scale, p, seed, dq=dq, dk=dk, dv=dv)
    torch.cuda.synchronize()
    for (buf, _), nm, S in zip(bufs, ("dq", "dk", "dv"), (Sq, Sk, Sk)):
        fb.check_outside(buf, S, W, nm)
    keep = fb.keep_mask_ref(seed, B * H * Sq, Sk, p).view(B, H, Sq, Sk).to(DEV)
    r = fb.attn_ref_bound(_heads(q, B, Sq, H, D), _heads(k, B, Sk, H, D), _heads(v, B, Sk, H, D), scale,
                          fb.attn_mask(B, Sq, Sk, False, None, DEV), dout=_heads(dout, B, Sq, H, D), o_in=_heads(o, B, Sq, H, D),
                          lse_in=lse, keep=keep)
    what = f"{Sq}x{Sk} D={D} p={p}"
    dp = f"DP={64 if D <= 64 else 96 if D <= 96 else 128}"
    note(f"attn_fwd_dropout o bf16 {dp}", fb.assert_within(o, _tok(r["o"]), _tok(r["o_bound"]), what + " o"))
    note(f"attn_fwd_dropout lse f32 {dp}", fb.assert_within(lse, r["lse"], r["lse_bound"], what + " lse"))
    for nm, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        note(f"attn_bwd_dropout {nm} bf16 {dp}", fb.assert_within(got, _tok(r[nm]), _tok(r[nm + "_bound"]), f"{what} {nm}"))


@pytest.mark.parametrize("p", [1.0, -0.1, float("nan")])
def test_attention_dropout_rejects_a_bad_probability_and_leaves_the_outputs_alone(p):
    B, H, Sq, Sk, D = 2, 3, 32, 32, 64
    W = H * D
    q, k, v = _attn_operands(B, H, Sq, Sk, D)
    dout = fb.rnd(B, Sq, W, seed=12).to(BF16).to(DEV)
    o, lse = fb.poisoned((B, Sq, W), BF16, DEV), fb.poisoned((B, H, Sq), F32, DEV)
    rc = ops._L().mh_attn_fwd_dropout(ops._p(q), ops._p(k), ops._p(v), ops._p(o), ops._p(lse), B, H, Sq, Sk, D,
                                      *ops._strides(q, k, v, o), D ** -0.5, p, ATTN_SEED, ops._s())
    with pytest.raises(_lib.MyriadHipError):
        _lib.check(rc, "mh_attn_fwd_dropout")
    with pytest.raises(_lib.MyriadHipError):
        ops.attn_fwd_dropout(q, k, v, H, D, D ** -0.5, p, ATTN_SEED)
    o_in, lse_in = fb.rnd(B, Sq, W, seed=13).to(BF16).to(DEV), fb.rnd(B, H, Sq, seed=14).to(DEV) + 4
    bufs = [fb.out_window(B, S, W, DEV) for S in (Sq, Sk, Sk)]
    with pytest.raises(_lib.MyriadHipError):
        ops.attn_bwd_dropout(q, k, v, o_in, dout, lse_in, H, D, D ** -0.5, p, ATTN_SEED, dq=bufs[0][1], dk=bufs[1][1], dv=bufs[2][1])
    torch.cuda.synchronize()
    fb.assert_untouched(o, "o"), fb.assert_untouched(lse, "lse")
    for (buf, _), nm in zip(bufs, ("dq", "dk", "dv")):
        fb.assert_untouched(buf, nm)


# -------------------------------------------------------------------------------------------------------- LayerNorm dropout
LN_EPS = 1e-12                                            # BERT's layer_norm_eps
LN_SEED_IN, LN_SEED_OUT = 0x1234567811111111, 0x7ABCDEF022222222


def _ln_form(M, D, form, monkeypatch):
    z, res, w, b, dy, p_in, p_out = (None if t is None else (t.to(DEV) if torch.is_tensor(t) else t)
                                     for t in fb.ln_dropout_inputs(M, D, form, seed=700 + D))
    ki = fb.keep_mask_ref(LN_SEED_IN, M, D, p_in).to(DEV) if p_in > 0 else None
    ko = fb.keep_mask_ref(LN_SEED_OUT, M, D, p_out).to(DEV) if p_out > 0 else None
    kw = dict(p_in=p_in, seed_in=LN_SEED_IN, p_out=p_out, seed_out=LN_SEED_OUT)
    what = f"form {form} {M}x{D}"
    with fb.poisoned_allocations(monkeypatch):
        x, yb, yf = ops.layernorm_fwd_dropout(z, res, w, b, LN_EPS, **kw)
    torch.cuda.synchronize()
    r = fb.ln_dropout_fwd_ref_bound(z, res, w, b, LN_EPS, ki, ko, x_out=x)
    if res is None:
        assert x is None
    else:
        note("layernorm_fwd_dropout x f32", fb.assert_within(x, r["x"], r["x_bound"], what + " x_out"))
    note("layernorm_fwd_dropout y f32", fb.assert_within(yf, r["y"], r["y_bound"], what + " y f32"))
    note("layernorm_fwd_dropout y bf16", fb.assert_within(yb, r["y"], r["y_bf16_bound"], what + " y bf16"))
    xin = z if res is None else x
    with fb.poisoned_allocations(monkeypatch):
        dx, dz = ops.layernorm_bwd_dropout(dy, xin, w, LN_EPS, **kw)
        dx1, none = ops.layernorm_bwd_dropout(dy, xin, w, LN_EPS, want_bf16=False, **kw)
    torch.cuda.synchronize()
    rb = fb.ln_dropout_bwd_ref_bound(dy, xin, w, LN_EPS, ki, ko)
    note("layernorm_bwd_dropout dx f32", fb.assert_within(dx, rb["dx"], rb["dx_bound"], what + " dx"))
    note("layernorm_bwd_dropout dz bf16", fb.assert_within(dz, rb["dz"], rb["dz_bound"], what + " dz"))
    assert none is None and torch.equal(dx1, dx), what + ": dx without the bf16 output"


@pytest.mark.parametrize("D", [1, 8, 255, 256, 257, 768, 1030])
@pytest.mark.parametrize("M", [13, 1])
def test_layernorm_dropout_fwd_bwd_edges(M, D, monkeypatch):
    """The four forms of fb.ln_dropout_inputs: widths on both sides of the 256-thread stride (odd ones included: the kernels
    use scalar accesses), every row kind of fb.norm_rows at M = 13."""
    for form in "abcd":
        _ln_form(M, D, form, monkeypatch)


def _ln_raw(M, D, p_in, p_out, bufs):
    z, res, w, b, dy, x_out, yb, yf, dx, dz = (ops._p(t) for t in bufs)
    L = ops._L()
    return (L.mh_layernorm_fwd_dropout(z, res, w, b, x_out, yb, yf, M, D, LN_EPS, p_in, LN_SEED_IN, p_out, LN_SEED_OUT, ops._s()),
            L.mh_layernorm_bwd_dropout(dy, z, w, dx, dz, M, D, LN_EPS, p_in, LN_SEED_IN, p_out, LN_SEED_OUT, ops._s()))


def _ln_raw_buffers(M, D):
    ins = [fb.rnd(M, D, seed=s).to(DEV) for s in (1, 2)] + [fb.rnd(D, seed=s).to(DEV) for s in (3, 4)] + [fb.rnd(M, D, seed=5).to(DEV)]
    outs = [fb.poisoned((M, D), dt, DEV) for dt in (F32, BF16, F32, F32, BF16)]
    return ins + outs, outs


def test_layernorm_dropout_with_no_rows_touches_nothing():
    bufs, outs = _ln_raw_buffers(4, 257)
    assert _ln_raw(0, 257, 0.1, 0.1, bufs) == (0, 0)
    torch.cuda.synchronize()
    for i, t in enumerate(outs):
        fb.assert_untouched(t, f"M = 0 output {i}")


@pytest.mark.parametrize("p", [1.0, -0.1, float("nan")])
def test_layernorm_dropout_rejects_a_bad_probability_and_leaves_the_outputs_alone(p):
    bufs, outs = _ln_raw_buffers(4, 257)
    for p_in, p_out in ((p, 0.1), (0.1, p)):
        for rc in _ln_raw(4, 257, p_in, p_out, bufs):
            with pytest.raises(_lib.MyriadHipError):
                _lib.check(rc, "layernorm dropout")
    z, res, w, b, dy = bufs[:5]
    with pytest.raises(_lib.MyriadHipError):
        ops.layernorm_fwd_dropout(z, res, w, b, LN_EPS, p_in=p, seed_in=1)
    with pytest.raises(_lib.MyriadHipError):
        ops.layernorm_bwd_dropout(dy, z, w, LN_EPS, p_out=p, seed_out=1)
    torch.cuda.synchronize()
    for i, t in enumerate(outs):
        fb.assert_untouched(t, f"rejected p output {i}")


# ------------------------------------------------------------------------------------------------------- TN weight gradient
def _tn_operand(M, C, left, right, vals):
    """vals [M, C] as the window rows 1 .. M, columns left .. left + C of a bf16 parent whose every other element (the columns
    beside it, the row before, 4 rows past M) holds +-1e4; the parent's row stride is a multiple of 8."""
    assert (left + C + right) % 8 == 0
    parent = _big(M + 5, left + C + right)
    parent[1:M + 1, left:left + C] = vals.to(BF16)
    parent = parent.to(DEV)
    return parent[1:M + 1, left:left + C]


def _tn_out(N, K, prev=None, prev_bias=None):
    """out [N, K] as a window of a poisoned wider fp32 buffer (pre-filled when accumulating), bias [N] likewise."""
    obuf, bbuf = fb.poisoned((N + 2, K + 8), F32, DEV), fb.poisoned((N + 8,), F32, DEV)
    out, bias = obuf[1:N + 1, 4:4 + K], bbuf[4:4 + N]
    if prev is not None:
        out.copy_(prev), bias.copy_(prev_bias)
    return obuf, bbuf, out, bias


def _tn_frames(obuf, bbuf, N, K, what):
    fb.assert_frame_untouched(obuf, slice(1, N + 1), slice(4, 4 + K), what + " out")
    fb.assert_untouched(bbuf[:4], what + " bias head"), fb.assert_untouched(bbuf[4 + N:], what + " bias tail")


def _tn_case(M, N, K, splits, monkeypatch):
    dy = _tn_operand(M, N, 8, 8, fb.lora_rows(M, N, seed=800 + M))
    x = _tn_operand(M, K, 16, 8, fb.rnd(M, K, seed=801 + M))
    s = splits if splits else ops._L().mh_gemm_tn_wgrad_auto_splits(M, N, K)
    what = f"tn_wgrad {M}x{N}x{K} splits={splits}"
    prev, prev_bias = fb.rnd(N, K, seed=802).to(DEV), fb.rnd(N, seed=803).to(DEV)
    for acc in (False, True):
        pw, pb = (prev, prev_bias) if acc else (None, None)
        rW, eW, rb, eb = fb.tn_wgrad_ref_bound(dy, x, s, pw, pb)
        runs = []
        for _ in range(2):
            obuf, bbuf, out, bias = _tn_out(N, K, pw, pb)
            with fb.poisoned_allocations(monkeypatch):
                ops.gemm_tn_wgrad(dy, x, out, bias=bias, accumulate=acc, splits=splits)
            torch.cuda.synchronize()
            _tn_frames(obuf, bbuf, N, K, what)
            runs.append((out.clone(), bias.clone()))
        tag = " accumulate" if acc else ""
        note("gemm_tn_wgrad out f32" + tag, fb.assert_within(runs[0][0], rW, eW, what + tag + " out"))
        note("gemm_tn_wgrad bias f32" + tag, fb.assert_within(runs[0][1], rb, eb, what + tag + " bias"))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), what + ": not bit-identical run to run"
    # without a bias: the same out, the bias buffer untouched
    obuf, bbuf, out, _ = _tn_out(N, K)
    with fb.poisoned_allocations(monkeypatch):
        ops.gemm_tn_wgrad(dy, x, out, splits=splits)
    torch.cuda.synchronize()
    fb.assert_frame_untouched(obuf, slice(1, N + 1), slice(4, 4 + K), what + " out (no bias)")
    fb.assert_untouched(bbuf, what + " absent bias")
    rW, eW, _, _ = fb.tn_wgrad_ref_bound(dy, x, s)
    note("gemm_tn_wgrad out f32", fb.assert_within(out, rW, eW, what + " out (no bias)"))


TN_M = [1, 31, 32, 33, 257]
TN_SPLITS = [1, 2, 3, 8, 0]                               # 0: the library's choice
TN_NK = [(64, 64), (128, 192), (192, 128), (64, 192), (192, 64)]


@pytest.mark.parametrize("splits", TN_SPLITS)
@pytest.mark.parametrize("M", TN_M)
def test_tn_wgrad_edges(M, splits, monkeypatch):
    """M on and next to the 32-row step, every split count (M = 33 with 8 splits and M = 1 with any leave trailing splits
    empty), N and K rotating through 64, 128, 192."""
    N, K = TN_NK[(TN_M.index(M) + TN_SPLITS.index(splits)) % len(TN_NK)]
    _tn_case(M, N, K, splits, monkeypatch)


def test_tn_wgrad_empty_trailing_split(monkeypatch):
    """M = 40 in 3 splits: 32 rows, 8 rows, none."""
    assert fb.tn_rows_per(40, 3) == 32
    _tn_case(40, 128, 128, 3, monkeypatch)


@pytest.mark.parametrize("splits", [1, 2])
def test_tn_wgrad_with_no_rows(splits, monkeypatch):
    """M = 0: out and bias become exactly 0; accumulating, both stay bit for bit."""
    N, K = 64, 128
    dy, x = _tn_operand(0, N, 8, 8, torch.zeros(0, N)), _tn_operand(0, K, 16, 8, torch.zeros(0, K))
    prev, prev_bias = fb.rnd(N, K, seed=804).to(DEV), fb.rnd(N, seed=805).to(DEV)
    for acc in (False, True):
        obuf, bbuf, out, bias = _tn_out(N, K, prev if acc else None, prev_bias if acc else None)
        with fb.poisoned_allocations(monkeypatch):
            ops.gemm_tn_wgrad(dy, x, out, bias=bias, accumulate=acc, splits=splits)
        torch.cuda.synchronize()
        _tn_frames(obuf, bbuf, N, K, f"M = 0 accumulate={acc}")
        if acc:
            assert torch.equal(out.view(torch.int32), prev.view(torch.int32)) and torch.equal(bias.view(torch.int32), prev_bias.view(torch.int32))
        else:
            assert bool((out == 0).all()) and bool((bias == 0).all())


def test_tn_wgrad_rejections_leave_the_output_alone():
    M = 33

    def rejected(dy, x, N, K):
        obuf, bbuf, out, bias = _tn_out(N, K)
        with pytest.raises(_lib.MyriadHipError):
            ops.gemm_tn_wgrad(dy, x, out, bias=bias)
        torch.cuda.synchronize()
        fb.assert_untouched(obuf, "rejected out"), fb.assert_untouched(bbuf, "rejected bias")

    good_dy, good_x = _tn_operand(M, 64, 8, 8, fb.rnd(M, 64, seed=1)), _tn_operand(M, 64, 16, 8, fb.rnd(M, 64, seed=2))
    rejected(_tn_operand(M, 96, 8, 8, fb.rnd(M, 96, seed=3)), good_x, 96, 64)                  # N % 64
    rejected(good_dy, _tn_operand(M, 96, 8, 8, fb.rnd(M, 96, seed=4)), 64, 96)                  # K % 64
    odd = fb.rnd(M, 64 + 4, seed=5).to(BF16).to(DEV)                                            # ld % 8 == 4, aligned start
    rejected(good_dy, odd[:, :64], 64, 64)
    rejected(odd[:, :64], good_x, 64, 64)
    wide = fb.rnd(M, 64 + 8, seed=6).to(BF16).to(DEV)                                           # ld % 8 == 0, start 8-byte aligned
    assert wide[:, 4:68].data_ptr() % 16 == 8
    rejected(good_dy, wide[:, 4:68], 64, 64)
    rejected(wide[:, 4:68], good_x, 64, 64)
