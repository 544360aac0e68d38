"""The conv-stack kernels (csrc/conv.hip: im2col, col2im, ReLU+maxpool forward / backward, weight pack, gradient unpack) and the
anomaly-map heads (csrc/expert.hip: pair_logits, zs_accumulate, rowmax_skip, bilinear_ac) element by element against float64, at
the shapes, strides and inputs where such kernels go wrong.  Outputs start as NaN poison (the wrappers' own allocations through
poisoned_allocations; caller-provided outputs are windows of one larger poisoned buffer whose frame must stay untouched -- dW and
db are views into one flat buffer, as the model holds them); every launch runs twice and must give the same bits (none of these
kernels uses atomics); every element is compared with tests/fp64_bounds.py's reference for that kernel: torch.equal for the data
movement, the derived bound for the arithmetic (tests/test_fp64_bounds_cpu.py shows that a torch emulation passes each and that
the plausible mistakes fail it).

Launch paths only these tests reach:
    conv_pack_kernel, scalar path        test_pack_unpack at K = 9, 63 (K % 4 != 0: the first stem layer)
    conv_pack_kernel, per-row tail       test_pack_unpack at K = 36 (K % 4 == 0, K % 8 != 0: the chunk that holds the bias)
    conv_unpack_kernel, scalar path      test_pack_unpack at K = 9, 63
    relu_pool_fwd/bwd_kernel<bf16_t>     test_relu_pool with a bf16 y
    second and later grid sweeps         test_conv_geometry at (8, 224, 224, 1) (6.4 M im2col items under the 4096 x 256 cap),
                                         test_relu_pool_many_windows, test_zs_accumulate / test_bilinear_ac at B S S > 2^20
    im2col(bias_col=False), K % 64 != 0  test_conv_geometry: refused (the kernel marks column K of a padded row with 1.0)

Worst err / bound per kernel, from one run of this module on an MI355X (the value assert_within returns; `-s` prints them):
    bilinear_ac f32                             0.443
    bilinear_ac one_minus                       0.998
    chain conv y f32                            0.17
    chain dgrad dcol bf16                       0.995
    chain dx of bf16 dcol                       0.831
    chain pool bf16                             0.982
    chain wgrad f32                             0.0122
    col2im f32                                  0.105
    pair_logits f32                             0.127
    rowmax_skip accumulate                      0.493
    zs_accumulate map                           0.998
    zs_accumulate mask                          0.999
    im2col, conv_pack, conv_unpack_grad, relu_pool_fwd / _bwd: torch.equal (no bound)
Outputs rounded to bf16 reach ~1.0 by construction (the bound's last term is the half-ulp of the correctly rounded result), and so
do the accumulate forms, whose bound is the half-ulp of the sum onto the earlier value wherever that value dwarfs what is added,
and bilinear_ac's one_minus form, whose bound is the half-ulp of the final 1 - v wherever v itself is exact (an identity resize,
h = w = 1, a sample on a grid point); the chain's dx is a sum of bf16-rounded dcol values.  Every other fp32 output is held to
<= 0.5 by note().  bilinear_ac takes its source position from one correctly rounded division of exact integers: in the form
o * fl(step) the position carries two roundings, and an emulation without contraction then reaches 0.6 of the bound at 16 -> 224.
"""
import pytest
import torch

from myriad_amd import _lib, ops
from tests import fp64_bounds as fb
from tests.fp64_bounds import assert_untouched, assert_within, poisoned, poisoned_allocations

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
WORST = {}

# bounds that are the half-ulp of one correct rounding and nothing else (a bf16 value, the fp32 sum onto an earlier value, or
# bilinear_ac's final 1 - v, which is all there is where v itself is exact: an identity resize, h = w = 1, a sample on a grid
# point): err / bound approaches 1 by construction
HALF_ULP_ONLY = ("bf16", "accumulate", "one_minus")


def note(name, ratio):
    """Record a kernel's err / bound (printed with -s: the docstring's table) and hold every other fp32 output to the factor-two
    head-room the bounds were accepted with."""
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))
    print(f"RATIO {name} {ratio:.3g} (worst so far {WORST[name]:.3g})")
    if not any(k in name for k in HALF_ULP_ONLY):
        assert ratio <= 0.5, f"{name}: err / bound {ratio:.3g} leaves less than a factor two of head-room"


def dev(t):
    return t.to(DEV)


def sync():
    torch.cuda.synchronize()


def same_bits(a, b):
    iv = {BF16: torch.int16, F32: torch.int32}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def twice(fn):
    """Run a launch twice; both results must have the same bits.  Returns the first."""
    r1 = fn()
    sync()
    r2 = fn()
    sync()
    for a, b in zip(r1 if isinstance(r1, tuple) else (r1,), r2 if isinstance(r2, tuple) else (r2,)):
        assert same_bits(a, b), "two launches of the same kernel differ"
    return r1


def window(n, dtype, margin=64):
    """(flat poisoned buffer, its n-element window) with `margin` elements either side."""
    buf = poisoned((n + 2 * margin,), dtype, DEV)
    return buf, buf[margin:margin + n]


def assert_margins(buf, n, what, margin=64):
    assert_untouched(buf[:margin], what + " (before)")
    assert_untouched(buf[margin + n:], what + " (after)")


# ------------------------------------------------------------------------------------------------------------ conv geometry
CONV_CASES = [(2, 224, 224, 1, 3, 1), (1, 112, 112, 4, 3, 1), (3, 28, 28, 16, 3, 1), (2, 14, 14, 256, 3, 1),   # the stem's shapes
              (8, 224, 224, 1, 3, 1),                                   # 6.4 M items: seven sweeps of the capped grid
              (1, 6, 10, 8, 3, 1),                                      # non-square
              (2, 7, 7, 1024, 5, 0), (1, 5, 5, 64, 5, 0),               # the head: a valid 5x5; a single output position
              (1, 2, 2, 4, 3, 1)]                                       # every tap of some rows lies outside the image


@pytest.mark.parametrize("B,H,W,C,k,pad", CONV_CASES)
def test_conv_geometry(B, H, W, C, k, pad, monkeypatch):
    K = k * k * C
    x = dev(fb.rnd(B, H, W, C, seed=600 + C + H).to(BF16))
    with poisoned_allocations(monkeypatch):
        col = twice(lambda: ops.im2col(x, k, k, pad))
    assert col.shape[1] == ops.round_up(K + 1, 64)
    assert torch.equal(col, fb.im2col_ref(x, k, k, pad, col.shape[1], True)), "im2col (bias column)"
    del col
    if K % 64 == 0:
        with poisoned_allocations(monkeypatch):
            col = twice(lambda: ops.im2col(x, k, k, pad, bias_col=False))
        assert col.shape[1] == K and torch.equal(col, fb.im2col_ref(x, k, k, pad, K, False)), "im2col (no bias column)"
        del col
    else:                                   # a padded row would carry the ones column at K: refused, not silently biased
        with pytest.raises(_lib.MyriadHipError):
            ops.im2col(x, k, k, pad, bias_col=False)
    dcol = fb.col2im_input(B, H, W, C, k, k, pad, seed=700 + C + H, device=DEV)
    with poisoned_allocations(monkeypatch):
        dx = twice(lambda: ops.col2im(dcol, B, H, W, C, k, k, pad))
    ref, bound = fb.col2im_ref_bound(dcol, B, H, W, C, k, k, pad)
    note("col2im f32", assert_within(dx, ref, bound, "col2im"))


# ------------------------------------------------------------------------------------------------------------------ pooling
def _pool_check(B, H, W, C, dtype, windowed, pad_cols_to, monkeypatch, seed):
    y = fb.pool_edge_windows(B, H, W, C, seed=seed, dtype=dtype)
    if windowed:                                          # y as a column window of a wider buffer: ldy > C
        wide = poisoned((B * H * W, C + 24), dtype, DEV)
        wide[:, 8:8 + C] = dev(y)
        yd = wide[:, 8:8 + C]
    else:
        yd = dev(y)
    dp = dev(fb.rnd(B, H // 2, W // 2, C, seed=seed + 1) + 3.0)      # no zero gradient: a wrong route or gate always shows
    with poisoned_allocations(monkeypatch):
        p = twice(lambda: ops.relu_pool_fwd(yd, B, H, W, C))
        dy, full = twice(lambda: ops.relu_pool_bwd(dp, yd, B, H, W, C, pad_cols_to=pad_cols_to))
    cpad = ops.round_up(C, pad_cols_to)
    assert full.shape == (B * H * W, cpad) and dy.shape == (B * H * W, C)
    assert torch.equal(p, fb.relu_pool_fwd_ref(dev(y), B, H, W, C)), "relu_pool_fwd"
    assert torch.equal(full, fb.relu_pool_bwd_ref(dp, dev(y), B, H, W, C, cpad)), "relu_pool_bwd"
    assert torch.equal(dy, full[:, :C])
    if windowed:
        assert_untouched(wide[:, :8], "y's frame"), assert_untouched(wide[:, 8 + C:], "y's frame")


@pytest.mark.parametrize("C", [4, 16, 64, 1024])
@pytest.mark.parametrize("pad_cols_to", [1, 64])
@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_relu_pool(dtype, windowed, pad_cols_to, C, monkeypatch):
    """The constructed windows (ties at every position pair, all equal, all negative, maximum 0.0 / -0.0, a one-ulp lead) in every
    case; a bf16 y runs relu_pool_*_kernel<bf16_t>."""
    _pool_check(2, 4, 6, C, dtype, windowed, pad_cols_to, monkeypatch, seed=800 + C)


def test_relu_pool_many_windows(monkeypatch):
    """1.18 M windows: the capped grid's second sweep."""
    _pool_check(2, 48, 48, 1024, F32, False, 64, monkeypatch, seed=850)


@pytest.mark.parametrize("H,W", [(5, 6), (4, 7)])
def test_relu_pool_odd_extent_is_refused(H, W):
    B, C = 1, 4
    y, dp = dev(fb.rnd(B * H * W, C, seed=860)), dev(fb.rnd(B, H // 2, W // 2, C, seed=861))
    p, dy = poisoned((B, H // 2, W // 2, C), BF16, DEV), poisoned((B * H * W, C), BF16, DEV)
    L, P, S = ops._L(), ops._p, ops._s
    assert L.mh_relu_maxpool2_fwd(P(y), 1, C, P(p), B, H, W, C, S()) != 0
    assert L.mh_relu_maxpool2_bwd(P(dp), P(y), 1, C, P(dy), C, B, H, W, C, S()) != 0
    sync()
    assert_untouched(p, "refused relu_pool_fwd"), assert_untouched(dy, "refused relu_pool_bwd")
    with pytest.raises(_lib.MyriadHipError):
        ops.relu_pool_fwd(y, B, H, W, C)
    with pytest.raises(_lib.MyriadHipError):
        ops.relu_pool_bwd(dp, y, B, H, W, C)


# ---------------------------------------------------------------------------------------------------------- pack and unpack
@pytest.mark.parametrize("Cout", [1, 4, 257])
@pytest.mark.parametrize("K", [9, 36, 63, 64, 144, 2304])
def test_pack_unpack(K, Cout, monkeypatch):
    """K = 9, 63: the scalar pack and unpack paths; K = 36: the vector path's per-row tail chunk holds the bias column."""
    Kpad = ops.round_up(K + 1, 64)
    Wm, bias = dev(fb.rnd(Cout, K, seed=900 + K)), dev(fb.rnd(Cout, seed=901 + K) + 2.0)
    for b in (bias, None):
        buf, flat = window(Cout * Kpad, BF16)
        out = flat.view(Cout, Kpad)
        twice(lambda: ops.conv_pack(Wm, b, out=out).clone())
        assert torch.equal(out, fb.conv_pack_ref(Wm, b, Kpad)), f"conv_pack (bias: {b is not None})"
        assert_margins(buf, Cout * Kpad, "conv_pack")
        with poisoned_allocations(monkeypatch):
            assert same_bits(ops.conv_pack(Wm, b), out)
    dWp = dev(fb.rnd(Cout, Kpad, seed=902 + K))
    for with_db in (True, False):
        n = Cout * K + Cout                                   # dW then db in one flat buffer, as the model holds them
        buf, flat = window(n, F32)
        dW, db = flat[:Cout * K].view(Cout, K), flat[Cout * K:]

        def run():
            ops.conv_unpack_grad(dWp, dW, db if with_db else None)
            return dW.clone(), db.clone()
        twice(run)
        assert torch.equal(dW, dWp[:, :K]), "conv_unpack_grad dW"
        if with_db:
            assert torch.equal(db, dWp[:, K]), "conv_unpack_grad db"
        else:
            assert_untouched(db, "db=None")
        assert_margins(buf, n, "conv_unpack_grad")


def test_pack_unpack_bad_kpad_is_refused():
    Cout, K = 4, 36
    Wm, bias, dWp = dev(fb.rnd(Cout, K, seed=910)), dev(fb.rnd(Cout, seed=911)), dev(fb.rnd(Cout, 64, seed=912))
    Wp, dW, db = poisoned((Cout, 64), BF16, DEV), poisoned((Cout, K), F32, DEV), poisoned((Cout,), F32, DEV)
    L, P, S = ops._L(), ops._p, ops._s
    for Kpad in (K, 44, 60):                                  # no room for the bias column; not a multiple of 8
        assert L.mh_conv_pack_weight(P(Wm), P(bias), P(Wp), Cout, K, Kpad, S()) != 0, Kpad
    assert L.mh_conv_unpack_grad(P(dWp), P(dW), P(db), Cout, K, K, S()) != 0
    sync()
    assert_untouched(Wp, "refused conv_pack"), assert_untouched(dW, "refused unpack"), assert_untouched(db, "refused unpack")


# -------------------------------------------------------------------------------------------------------------- pair_logits
@pytest.mark.parametrize("rows", [1, 3, 4, 1029])
@pytest.mark.parametrize("C", [4, 64, 252, 256, 768, 1024])
def test_pair_logits(C, rows, monkeypatch):
    """rows_per_batch in {1, 3, 257}: the text pair changes inside a workgroup's four rows; p contiguous and as a strided window;
    rows scaled by 1e-4 and 1e4 next to each other."""
    for rpb in (1, 3, 257):
        p, text = fb.pair_inputs(rows, C, rpb, seed=1000 + C + rows + rpb)
        wide = poisoned((rows, C + 12), F32, DEV)
        wide[:, 4:4 + C] = dev(p)
        ref, bound = fb.pair_logits_ref_bound(dev(p), dev(text), rpb, 100.0)
        for pd in (dev(p), wide[:, 4:4 + C]):
            with poisoned_allocations(monkeypatch):
                out = twice(lambda: ops.pair_logits(pd, dev(text), rpb, 100.0))
            note("pair_logits f32", assert_within(out, ref, bound, f"pair_logits C={C} rows={rows} rpb={rpb}"))


def test_pair_logits_refuses_a_width_off_the_float4_grid():
    p, text = fb.pair_inputs(3, 6, 1, seed=1100)
    with pytest.raises(_lib.MyriadHipError):
        ops.pair_logits(dev(p), dev(text), 1)
    out = poisoned((3, 2), F32, DEV)
    pd, td = dev(p), dev(text)
    assert ops._L().mh_pair_logits(ops._p(pd), 6, ops._p(td), ops._p(out), 3, 1, 6, 100.0, ops._s()) != 0
    sync()
    assert_untouched(out, "refused pair_logits")


# ------------------------------------------------------------------------------------------- zs_accumulate and bilinear_ac
def _many(S):
    return 2 ** 20 // (S * S) + 1                            # B S S > 2^20: the capped grid sweeps twice


@pytest.mark.parametrize("h,S", [(16, 224), (16, 16), (1, 7), (2, 3), (7, 224)])
@pytest.mark.parametrize("many", [False, True])
def test_zs_accumulate(h, S, many):
    """Two accumulations with different weights onto non-zero accumulators; logit differences up to +-60."""
    B = _many(S) if many else 1
    lg, mask0, map0 = fb.zs_inputs(B, h, S, seed=1200 + h + S)
    lg = dev(lg)
    bm, mask = window(B * h * h, F32)
    ba, amap = window(B * S * S, F32)
    mask, amap = mask.view(B, h, h), amap.view(B, S, S)
    mask.copy_(mask0), amap.copy_(map0)
    for w in (0.37, 1.6):
        prev = (mask.clone(), amap.clone())

        def run():
            m, a = prev[0].clone(), prev[1].clone()
            ops.zs_accumulate(lg, m, a, w)
            return m, a
        m2, a2 = twice(run)
        ops.zs_accumulate(lg, mask, amap, w)
        sync()
        assert same_bits(mask, m2) and same_bits(amap, a2)
        rm, em, ra, ea = fb.zs_accumulate_ref_bound(lg, prev[0], prev[1], w)
        note("zs_accumulate mask", assert_within(mask, rm, em, f"zs mask h={h} S={S} B={B}"))
        note("zs_accumulate map", assert_within(amap, ra, ea, f"zs map h={h} S={S} B={B}"))
    assert_margins(bm, B * h * h, "zs mask_acc"), assert_margins(ba, B * S * S, "zs map_acc")


BILINEAR_CASES = [(16, 16, 224, 224), (16, 16, 16, 16), (1, 1, 7, 7), (2, 2, 3, 3), (7, 7, 224, 224),   # the zs geometries
                  (5, 9, 33, 20), (5, 9, 1, 20), (5, 9, 33, 1), (16, 16, 7, 7), (7, 9, 7, 9)]           # non-square, H == 1, W == 1, down, identity


@pytest.mark.parametrize("h,w,H,W", BILINEAR_CASES)
@pytest.mark.parametrize("many", [False, True])
def test_bilinear_ac(h, w, H, W, many, monkeypatch):
    B = 2 ** 20 // (H * W) + 1 if many else 1
    x = dev(fb.rnd(B, h, w, seed=1300 + h + W))
    for one_minus in (False, True):
        with poisoned_allocations(monkeypatch):
            out = twice(lambda: ops.bilinear_ac(x, H, W, one_minus))
        ref, bound = fb.bilinear_ref_bound(x, H, W, one_minus)
        note("bilinear_ac one_minus" if one_minus else "bilinear_ac f32", assert_within(out, ref, bound, f"bilinear_ac {(h, w)} -> {(H, W)} B={B} one_minus={one_minus}"))
        if (h, w) == (H, W):
            assert torch.equal(out, 1 - x if one_minus else x), "identity resize"


# -------------------------------------------------------------------------------------------------------------- rowmax_skip
@pytest.mark.parametrize("period", [0, 257, 5])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 514, 2056])
def test_rowmax_skip(cols, period):
    """Contiguous and as scores[:, :cols] of a wider matrix whose excluded columns hold the largest values; a maximum in a skipped
    column; a row of -inf but for one entry; rows not a multiple of 4."""
    for rows in (7, 1029):
        full, acc0 = fb.rowmax_inputs(rows, cols, cols + 8, seed=1400 + cols + rows)
        wide = poisoned((rows, cols + 8), F32, DEV)
        wide.copy_(full)
        for s in (wide[:, :cols].contiguous(), wide[:, :cols]):
            buf, acc = window(rows, F32)
            acc.copy_(acc0)
            prev = acc.clone()

            def run():
                a = prev.clone()
                ops.rowmax_skip(s, a, period, 0.61)
                return a
            a2 = twice(run)
            ops.rowmax_skip(s, acc, period, 0.61)
            sync()
            assert same_bits(acc, a2)
            ref, bound = fb.rowmax_skip_ref_bound(s, prev, period, 0.61)
            note("rowmax_skip accumulate", fb.rowmax_check(acc, ref, bound, f"rowmax_skip cols={cols} period={period} rows={rows}"))
            assert_margins(buf, rows, "rowmax_skip acc")


# ---------------------------------------------------------------------------------------------------------------- one chain
def _auto_splits(M, N, K):
    """The K split ops.gemm_auto_f32 chooses (1: the plain GEMM)."""
    tiles, kt = ((M + 127) // 128) * ((N + 127) // 128), K // 64
    return 1 if tiles >= 128 or kt < 16 else max(1, min(kt // 4, 512 // tiles))


@pytest.mark.parametrize("case", fb.CHAIN_CASES)
def test_stem_layer_chain(case, monkeypatch):
    """One stem layer forward and backward as VENet runs it -- pack -> im2col -> gemm -> pool; pool-backward -> wgrad GEMM -> unpack;
    dgrad GEMM -> col2im -- against fp64 conv2d / max_pool2d autograd, the bound composed from gemm_ref_bound and the pieces.
    Windows whose routing is a decision get no gradient (at most 1 % of them: asserted, and on the CPU before any GPU run)."""
    ci, co, B, H, W, _ = case
    ops.ensure_workspace(DEV)
    x, wm, bias, dp = fb.stem_chain_case(*case)
    M, K = B * H * W, 9 * ci
    Kpad = ops.round_up(K + 1, 64)
    r = fb.stem_chain_ref(x, wm, bias, dp, wgrad_splits=_auto_splits(co, Kpad, ops.round_up(M, 64)))
    assert float(r["decisions"].double().mean()) <= 0.01
    xd, wmd, bd, dpd = dev(x), dev(wm), dev(bias), dev(r["dp_used"])
    with poisoned_allocations(monkeypatch):
        wp = ops.conv_pack(wmd, bd)
        col = ops.im2col(xd, 3, 3, 1)
        y = twice(lambda: ops.gemm(col, wp, out_dtype=F32))
        p = ops.relu_pool_fwd(y, B, H, W, co)
        dy, dyfull = ops.relu_pool_bwd(dpd, y, B, H, W, co, pad_cols_to=64)
        dwp = torch.empty((co, Kpad), dtype=F32, device=DEV)
        ops.gemm_auto_f32(ops.transpose_to_bf16(dy, 64), ops.transpose_to_bf16(col, 64), dwp)
        buf, flat = window(co * K + co, F32)
        dW, db = flat[:co * K].view(co, K), flat[co * K:]
        ops.conv_unpack_grad(dwp, dW, db)
        dcol = ops.gemm(dyfull, ops.transpose_to_bf16(wp, 64))
        dx = ops.col2im(dcol, B, H, W, ci, 3, 3, 1)
    sync()
    g = {k: dev(v) for k, v in r.items() if isinstance(v, torch.Tensor)}
    assert torch.equal(wp, g["wp"]) and torch.equal(col, g["col"])
    note("chain conv y f32", assert_within(y, g["y"], g["y_bound"], "chain y"))
    note("chain pool bf16", assert_within(p.reshape(B, H // 2, W // 2, co), g["p"], g["p_bound"], "chain pool"))
    assert torch.equal(dyfull, g["dy"]), "chain relu_pool_bwd: a window outside the decisions is routed differently"
    note("chain wgrad f32", assert_within(dwp, g["dwp"], g["dwp_bound"], "chain wgrad"))
    assert torch.equal(dW, dwp[:, :K]) and torch.equal(db, dwp[:, K])
    assert_within(dW, g["dW"], g["dwp_bound"][:, :K], "chain dW against autograd")
    assert_within(db, g["db"], g["dwp_bound"][:, K], "chain db against autograd")
    assert_margins(buf, co * K + co, "chain dW / db")
    note("chain dgrad dcol bf16", assert_within(dcol, g["dcol"], g["dcol_bound"], "chain dcol"))
    note("chain dx of bf16 dcol", assert_within(dx, g["dx"], g["dx_bound"], "chain dx"))
