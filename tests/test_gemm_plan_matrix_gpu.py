"""Every GEMM plan kernel (ops.GEMM_KERNEL_NAMES 0-6, split and unsplit where the planner allows both) and every epilogue
against fp64, element by element (tests/fp64_bounds.py), with outputs written into a poisoned window of a wider poisoned buffer
(owned elements all written, nothing outside touched) and the split-K scratch filled with NaN bytes before each split launch
(a slab read before it is written shows up).  Each row of the table states the plan the planner gives it: if the planner moves
a shape, the row fails by name instead of its coverage vanishing.

The 256 x 256 tile runs as both instances option gemm256_impl selects (1: the hand-scheduled gemm_x4 loop -- the shipped
library carries its eight-wave form only -- 0: the plain eight-wave kernel), with few (< 32) and many (>= 32) k-tiles per
workgroup.  Largest err/bound seen on the MI355X over this file and test_attention_edges_gpu.py: 0.996, a bf16 output one
half-ulp from its fp64 value (1184x4096x64 with bias) -- the output rounding, not the accumulation, is what the bound is tight on."""
import pytest
import torch

from myriad_amd import _lib, ops
from tests import fp64_bounds as fb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32

# name, M, N, K, options set for the row, expected (kernel, splits) of the bf16 and f32 outputs (GELU_PLANS: where the
# GELU epilogue plans differently -- the weight-streaming kernel has none)
ROWS = [
    ("gemv_m1", 1, 4096, 4096, {}, (0, 1)),
    ("gemv_m2_k192", 2, 1000, 192, {}, (0, 1)),
    ("gemv_m16_n1001", 16, 1001, 256, {}, (0, 1)),
    ("past_gemv_m17", 17, 768, 768, {}, (6, 1)),
    ("t64_qformer", 81, 768, 768, {}, (6, 1)),
    ("t64_small", 17, 100, 256, {}, (6, 1)),
    ("t64_300", 300, 520, 256, {}, (6, 1)),
    ("t64_n1001", 300, 1001, 256, {}, (6, 1)),
    ("t64_n1002", 300, 1002, 256, {}, (6, 1)),
    ("t64_n1003", 300, 1003, 256, {}, (6, 1)),
    ("t160x128_m148", 148, 4096, 4096, {}, (4, 8)),
    ("t160x128_vit", 257, 1408, 6144, {}, (4, 11)),
    ("t160x96_m161", 161, 4096, 1024, {}, (5, 2)),
    ("t160x128_m129", 129, 4096, 4096, {}, (4, 8)),
    ("t160x128_m160", 160, 4096, 4096, {}, (4, 8)),
    ("t160x128_m320", 320, 4096, 4096, {}, (4, 4)),
    ("t160x128_f32slabs", 148, 4100, 4096, {}, (4, 7)),
    ("t160x96_unsplit_n4097", 148, 4097, 4096, {}, (5, 1)),
    ("t160x128_unsplit", 148, 32766, 512, {}, (4, 1)),
    ("t256_split", 1184, 4096, 4096, {}, (2, 3)),
    ("t256_unsplit_few_ktiles", 2056, 4224, 1408, {}, (2, 1)),
    ("t256_unsplit_many_ktiles", 2056, 4224, 4096, {}, (2, 1)),
    ("t256_f32slabs_n4100", 1184, 4100, 4096, {}, (2, 3)),
    ("t256_ragged_ktiles", 1184, 4096, 4288, {}, (2, 3)),
    ("t256_m257", 257, 4096, 4096, {"gemm_skinny": 0}, (2, 5)),
    ("t128_m256", 256, 4096, 4096, {"gemm_skinny": 0}, (1, 8)),
    ("t128_m255", 255, 4096, 4096, {"gemm_skinny": 0}, (1, 8)),
    ("t128x64_vit", 2056, 1408, 1408, {}, (3, 1)),
    ("t128x64_n1001", 2056, 1001, 1408, {}, (3, 1)),
    ("t128x64_k128", 200, 136, 128, {}, (3, 1)),
    ("t128x64_k64_n1002", 1000, 1002, 64, {}, (3, 1)),
    ("t128_k128", 1184, 4096, 128, {}, (1, 1)),
    ("t128_k64", 1184, 4096, 64, {}, (1, 1)),
    ("t128_split_m64", 64, 4096, 4096, {}, (1, 16)),
    ("t128_split_m128", 128, 4096, 4096, {}, (1, 16)),
]
GELU_PLANS = {"gemv_m1": (1, 16), "gemv_m2_k192": (3, 1), "gemv_m16_n1001": (3, 1)}


def _lib_():
    return _lib.load()


_options = fb.lib_options
_rnd = fb.rnd


def _operand(rows, K, seed, scale, wide):
    """bf16 [rows, K] on the device; `wide`: a view into a buffer with a longer row (lda / ldb > K)."""
    x = (_rnd(rows, K + (64 if wide else 0), seed=seed) * scale).to(BF16).to(DEV)
    return x[:, :K]


def _bf16_slabs(M, N, K, out_f32, gelu):
    kernel, splits = ops.gemm_plan(M, N, K, out_f32=out_f32, gelu=gelu)
    return splits, splits > 1 and kernel in (2, 4, 5) and N % 8 == 0 and _lib_().mh_get_option(b"slab_bf16") == 1


def _window(M, N, dt):
    """A poisoned [M, N] window (row 1.., column 8..) of a wider poisoned buffer: ldc = N + 16 rounded up to 8."""
    ld = (N + 16 + 7) // 8 * 8
    buf = fb.poisoned((M + 2, ld), dt, DEV)
    return buf, buf[1:M + 1, 8:8 + N]


def _residual(M, N, seed):
    """f32 [M, N] residual with a row stride that is a multiple of 4 (the ABI's rule for ldr), also for N % 4 != 0."""
    ld = (N + 3) // 4 * 4
    return _rnd(M, ld, seed=seed).to(DEV)[:, :N]


def _check_window(buf, win, M, N, ref, bnd, what):
    r = fb.assert_within(win, ref, bnd, what)
    fb.assert_untouched(buf[0], what + " row above")
    fb.assert_untouched(buf[M + 1], what + " row below")
    fb.assert_untouched(buf[:, :8], what + " left columns")
    fb.assert_untouched(buf[:, 8 + N:], what + " right columns")
    return r


def _run_epilogues(a, b, M, N, K, bias, res, regstage=False):
    ws = ops.ensure_workspace(torch.device(DEV))
    worst = 0.0
    forms = [  # name, out dtype, kwargs, gelu
        ("f32", F32, {}, False),
        ("bf16", BF16, {}, False),
        ("bias", BF16, dict(bias=bias), False),
        ("bias_gelu", BF16, dict(bias=bias), True),
        ("alpha_bias_residual", F32, dict(bias=bias, residual=res, alpha=0.5), False),
    ]
    for name, dt, kw, gelu in forms:
        splits, sbf = _bf16_slabs(M, N, K, dt == F32, gelu)
        if regstage:
            splits, sbf = 1, False
        buf, win = _window(M, N, dt)
        ws.fill_(255)                                        # NaN in every slab format
        ops.gemm(a, b, out=win, gelu=gelu, regstage=regstage, **kw)
        ref, bnd = fb.gemm_ref_bound(a, b, alpha=kw.get("alpha", 1.0), bias=kw.get("bias"), residual=kw.get("residual"),
                                     gelu=gelu, out_bf16=dt == BF16, splits=splits, bf16_slabs=sbf)
        worst = max(worst, _check_window(buf, win, M, N, ref, bnd, f"{M}x{N}x{K} {name}"))
    # in place: out is residual (f32), a window of a wider buffer
    splits, sbf = _bf16_slabs(M, N, K, True, False)
    if regstage:
        splits, sbf = 1, False
    buf, win = _window(M, N, F32)
    win.copy_(res)
    ws.fill_(255)
    ops.gemm(a, b, out=win, residual=win, regstage=regstage)
    ref, bnd = fb.gemm_ref_bound(a, b, residual=res, splits=splits, bf16_slabs=sbf)
    worst = max(worst, _check_window(buf, win, M, N, ref, bnd, f"{M}x{N}x{K} in place"))
    return worst


def _row_impls(plan):
    return (1, 0) if plan[0] == 2 else (None,)


@pytest.mark.parametrize("name,M,N,K,opts,plan", ROWS, ids=[r[0] for r in ROWS])
def test_plan_matrix_rows(name, M, N, K, opts, plan):
    """Plan asserted first, then f32 / bf16 output, bias, bias + GELU, alpha + bias + residual and in-place out-is-residual,
    each into a poisoned window of a wider buffer; operands are views with lda / ldb > K on every other row."""
    ops.ensure_workspace(torch.device(DEV))
    wide = [r[0] for r in ROWS].index(name) % 2 == 1
    with _options(**opts):
        for f32, gelu, want in ((False, False, plan), (True, False, plan), (False, True, GELU_PLANS.get(name, plan))):
            got = ops.gemm_plan(M, N, K, out_f32=f32, gelu=gelu)
            assert got == want, f"row {name} (f32={f32}, gelu={gelu}): the planner now gives {got}, not {want}"
        a = _operand(M, K, 1, 1.0, wide)
        # asymmetric B with rows of very different sizes: a small row is held to a bound of its own size
        b = (_rnd(N, K, seed=2, scale=0.05) * (1 + 30 * (torch.arange(N) % 7 == 0))[:, None]).to(BF16).to(DEV)
        if wide:
            b = torch.cat([b, b[:, :64]], 1)[:, :K]
        bias = _rnd(N, seed=3).to(DEV)
        res = _residual(M, N, 4)
        for impl in _row_impls(plan):
            with _options(**({} if impl is None else {"gemm256_impl": impl})):
                _run_epilogues(a, b, M, N, K, bias, res)


def test_regstage_instance():
    """The register-staged 128 x 128 instance (flag GEMM_REGSTAGE: always kernel 1, never split)."""
    import ctypes
    k, s = ctypes.c_int(0), ctypes.c_int(0)
    M, N, K = 200, 1001, 192
    for flags in (ops.GEMM_REGSTAGE, ops.GEMM_REGSTAGE | ops.GEMM_OUT_F32, ops.GEMM_REGSTAGE | ops.GEMM_GELU):
        assert _lib_().mh_gemm_plan(M, N, K, flags, ctypes.addressof(k), ctypes.addressof(s)) == 0
        assert (k.value, s.value) == (1, 1), flags
    a = _operand(M, K, 5, 1.0, True)
    b = _operand(N, K, 6, 0.05, False)
    _run_epilogues(a, b, M, N, K, _rnd(N, seed=7).to(DEV), _residual(M, N, 8), regstage=True)


def test_table_reaches_every_plan_kernel_split_and_unsplit():
    """Kernel ids 0-6 all appear; 1, 2, 4 and 5 (the ones the planner splits) both split and unsplit; the 256 tile with few and
    many k-tiles per workgroup, bf16 and fp32 slabs, a k-tile count the split count does not divide."""
    plans = {r[5] for r in ROWS}
    assert {k for k, _ in plans} == set(ops.GEMM_KERNEL_NAMES) == set(range(7))
    for k in (1, 2, 4, 5):
        assert (k, 1) in plans and any(p[0] == k and p[1] > 1 for p in plans), k
    assert any(r[5] == (2, 1) and r[3] // 64 < 32 for r in ROWS) and any(r[5] == (2, 1) and r[3] // 64 >= 32 for r in ROWS)
    split = [r for r in ROWS if r[5][1] > 1]
    assert any(r[2] % 8 == 4 for r in split) and any(r[2] % 8 == 0 for r in split)
    assert any((r[3] // 64) % r[5][1] for r in split)
    assert any(r[2] % 4 for r in ROWS) and {64, 128} <= {r[3] for r in ROWS}


# ------------------------------------------------------------------------------------------------------------ fused forms
def _assert_split(M, N, K, split):
    kernel, splits = ops.gemm_plan(M, N, K, out_f32=True)
    assert (splits > 1) == split, f"{M}x{N}x{K}: plan ({kernel}, {splits}) -- the shape no longer covers the {'split' if split else 'unsplit'} form"


@pytest.mark.parametrize("M,N,K,split", [(1184, 4096, 4096, True), (300, 512, 256, False)])
def test_gemm_residual_rmsnorm_and_rmsnorm_bwd_vs_fp64(M, N, K, split, monkeypatch):
    """h = a b^T + residual (f32), y = RMSNorm(h) w (bf16, into a view of a wider buffer); and the fused dgrad + RMSNorm
    backward dx = r w dy - x r^3 mean(x w dy) + dres (f32 and bf16): under poisoned allocations, against fp64."""
    ops.ensure_workspace(torch.device(DEV))
    _assert_split(M, N, K, split)
    eps = 1e-6
    a = _operand(M, K, 11, 1.0, True)
    b = _operand(N, K, 12, 0.05, False)
    res = _rnd(M, N, seed=13).to(DEV)
    w = (1 + 0.1 * _rnd(N, seed=14)).to(DEV)
    splits, sbf = _bf16_slabs(M, N, K, True, False)
    h64, e_h = fb.gemm_ref_bound(a, b, residual=res, splits=splits, bf16_slabs=sbf)
    r = torch.rsqrt((h64 * h64).mean(-1, keepdim=True) + eps)
    w64 = w.double()
    y64 = w64 * h64 * r
    gN = fb.g_acc(N)
    e_y = w64.abs() * r * (e_h + h64.abs() * r * r * (h64.abs() * e_h).mean(-1, keepdim=True)) + (gN + 2 ** -21) * y64.abs()
    e_y = e_y + fb.U16 * (y64.abs() + e_y)
    ybuf, ywin = _window(M, N, BF16)
    ws = ops.ensure_workspace(torch.device(DEV))
    ws.fill_(255)
    with fb.poisoned_allocations(monkeypatch):
        h, y = ops.gemm_residual_rmsnorm(a, b, res, w, eps, y_out=ywin)
    fb.assert_within(h, h64, e_h, "h")
    _check_window(ybuf, ywin, M, N, y64, e_y, "y")
    # backward: dy = a2 b2^T (f32, maybe slabs), x = h, dres
    a2 = _operand(M, K, 15, 0.3, False)
    b2 = _operand(N, K, 16, 0.05, True)
    x = h64.float()
    dres = _rnd(M, N, seed=17).to(DEV)
    splits, sbf = _bf16_slabs(M, N, K, True, False)
    dy64, e_dy = fb.gemm_ref_bound(a2, b2, splits=splits, bf16_slabs=sbf)
    x64 = x.double()
    rx = torch.rsqrt((x64 * x64).mean(-1, keepdim=True) + eps)
    m = (x64 * w64 * dy64).mean(-1, keepdim=True)
    dx64 = rx * w64 * dy64 - x64 * rx ** 3 * m + dres.double()
    e_dx = (rx * w64.abs() * e_dy + x64.abs() * rx ** 3 * (x64.abs() * w64.abs() * e_dy).mean(-1, keepdim=True)
            + 2 ** -21 * rx * (w64 * dy64).abs()
            + x64.abs() * rx ** 3 * (gN * (x64 * w64 * dy64).abs().mean(-1, keepdim=True) + 2 ** -21 * m.abs())
            + 2 * fb.U32 * dx64.abs())
    ws.fill_(255)
    with fb.poisoned_allocations(monkeypatch):
        dx, dxb = ops.gemm_rmsnorm_bwd(a2, b2, x, w, eps, dres=dres)
    fb.assert_within(dx, dx64, e_dx, "dx")
    fb.assert_within(dxb, dx64, e_dx + fb.U16 * (dx64.abs() + e_dx), "dx bf16")


@pytest.mark.parametrize("M,N,K,split", [(2056, 1408, 6144, True), (2056, 1408, 1408, False)])
def test_gemm_residual_layernorm_vs_fp64(M, N, K, split, monkeypatch):
    """h = a b^T + bias + residual (f32), y = LayerNorm(h) w + nb (bf16), under poisoned allocations, against fp64."""
    ops.ensure_workspace(torch.device(DEV))
    _assert_split(M, N, K, split)
    eps = 1e-6
    a = _operand(M, K, 21, 1.0, False)
    b = _operand(N, K, 22, 0.05, True)
    bias = _rnd(N, seed=23).to(DEV)
    res = _rnd(M, N, seed=24).to(DEV) + 3.0                # an offset mean: the centring cancels
    w = (1 + 0.1 * _rnd(N, seed=25)).to(DEV)
    nb = (0.1 * _rnd(N, seed=26)).to(DEV)
    splits, sbf = _bf16_slabs(M, N, K, True, False)
    h64, e_h = fb.gemm_ref_bound(a, b, bias=bias, residual=res, splits=splits, bf16_slabs=sbf)
    gN = fb.g_acc(N)
    mean = h64.mean(-1, keepdim=True)
    c = h64 - mean
    var = (c * c).mean(-1, keepdim=True)
    r = torch.rsqrt(var + eps)
    y64 = c * r * w.double() + nb.double()
    d = e_h + e_h.mean(-1, keepdim=True) + gN * h64.abs().mean(-1, keepdim=True) + fb.U32 * c.abs()
    e_r = r * r * ((c.abs() * d).mean(-1, keepdim=True) + 0.5 * gN * var) + 2 ** -21
    e_y = w.double().abs() * r * (d + c.abs() * e_r) + 2 * fb.U32 * (y64.abs() + nb.double().abs())
    e_y = e_y + fb.U16 * (y64.abs() + e_y)
    ops.ensure_workspace(torch.device(DEV)).fill_(255)
    with fb.poisoned_allocations(monkeypatch):
        h, y = ops.gemm_residual_layernorm(a, b, bias, res, w, nb, eps)
    fb.assert_within(h, h64, e_h, "h")
    fb.assert_within(y, y64, e_y, "y")


def _silu64(g):
    return g / (1 + torch.exp(-g))


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("M,I,K,D,split", [(300, 256, 128, 256, False), (148, 11008, 4096, 4096, True)])
def test_gemm_swiglu_fwd_bwd_vs_fp64(M, I, K, D, split, fused, monkeypatch):
    """gu = bf16(x wgu^T) (128-blocked gate | up), act = bf16(silu(g) u) from the stored gu; dgu = the SiLU-gate backward of
    dact = bf16(dh wdT^T) at the stored gu.  Under poisoned allocations, against fp64 (the 148-row down dgrad is a K split)."""
    ops.ensure_workspace(torch.device(DEV))
    _assert_split(M, I, D, split)                          # the down dgrad whose slabs the gate backward sums
    blk = ops.SWIGLU_BLK
    x = _operand(M, K, 31, 0.5, False)
    wg = (_rnd(I, K, seed=32, scale=0.05)).to(BF16).to(DEV)
    wu = (_rnd(I, K, seed=33, scale=0.05)).to(BF16).to(DEV)
    wgu = ops.interleave_gate_up(wg, wu)
    dh = _operand(M, D, 34, 0.1, False)
    wdT = _operand(I, D, 35, 0.05, False)
    with _options(swiglu_fused=fused):
        ops.ensure_workspace(torch.device(DEV)).fill_(255)
        with fb.poisoned_allocations(monkeypatch):
            gu, act = ops.gemm_swiglu_fwd(x, wgu)
            dgu = ops.gemm_swiglu_bwd(dh, wdT, gu)
    splits, sbf = _bf16_slabs(M, 2 * I, K, False, False)
    gu64, e_gu = fb.gemm_ref_bound(x, wgu, out_bf16=True, splits=splits, bf16_slabs=sbf)
    fb.assert_within(gu, gu64, e_gu, "gu")
    g = gu.double().view(M, I // blk, 2, blk)[:, :, 0].reshape(M, I)
    u = gu.double().view(M, I // blk, 2, blk)[:, :, 1].reshape(M, I)
    sg = _silu64(g)
    act64 = sg * u
    fb.assert_within(act, act64, (16 * fb.U32 + fb.U16) * act64.abs() + 1e-30, "act")
    splits, sbf = _bf16_slabs(M, I, D, False, False)
    dact64, e_dact = fb.gemm_ref_bound(dh, wdT, out_bf16=True, splits=splits, bf16_slabs=sbf)
    sig = torch.sigmoid(g)
    dsilu = sig * (1 + g * (1 - sig))
    dg64, du64 = dact64 * u * dsilu, dact64 * sg
    e_dg = e_dact * (u * dsilu).abs() + 2 ** -20 * dg64.abs()
    e_du = e_dact * sg.abs() + 2 ** -20 * du64.abs()
    e_dg, e_du = e_dg + fb.U16 * (dg64.abs() + e_dg), e_du + fb.U16 * (du64.abs() + e_du)
    d3 = dgu.view(M, I // blk, 2, blk)
    fb.assert_within(d3[:, :, 0].reshape(M, I), dg64, e_dg, "dg")
    fb.assert_within(d3[:, :, 1].reshape(M, I), du64, e_du, "du")


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("M,N,K,D,split", [(81, 3072, 768, 768, False), (2056, 6144, 1408, 1408, False),
                                           (148, 4096, 4096, 4096, True)])
def test_gemm_gelu_fwd_bwd_vs_fp64(M, N, K, D, split, fused, monkeypatch):
    """pre = bf16(x w^T + bias), act = bf16(gelu(pre)); dpre = bf16(bf16(dy wT^T) gelu'(pre)).  Under poisoned allocations,
    against fp64 (the 2056-row product is the 256 tile and the 148-row one a K split: there the entry points run the two
    launches)."""
    ops.ensure_workspace(torch.device(DEV))
    _assert_split(M, N, K, split)
    _assert_split(M, N, D, split)
    x = _operand(M, K, 41, 0.5, True)
    w = _operand(N, K, 42, 0.08, False)
    bias = _rnd(N, seed=43, scale=0.3).to(DEV)
    dy = _operand(M, D, 44, 0.1, False)
    wT = _operand(N, D, 45, 0.05, True)
    with _options(gelu_fused=fused):
        ops.ensure_workspace(torch.device(DEV)).fill_(255)
        with fb.poisoned_allocations(monkeypatch):
            pre, act = ops.gemm_gelu_fwd(x, w, bias)
            dpre = ops.gemm_gelu_bwd(dy, wT, pre)
    splits, sbf = _bf16_slabs(M, N, K, False, False)
    pre64, e_pre = fb.gemm_ref_bound(x, w, bias=bias, out_bf16=True, splits=splits, bf16_slabs=sbf)
    fb.assert_within(pre, pre64, e_pre, "pre")
    p = pre.double()
    act64 = torch.nn.functional.gelu(p)
    fb.assert_within(act, act64, (4 * fb.U32 + fb.U16) * act64.abs() + 2e-7 * p.abs() + 1e-30, "act")
    splits, sbf = _bf16_slabs(M, N, D, False, False)
    dact64, e_dact = fb.gemm_ref_bound(dy, wT, out_bf16=True, splits=splits, bf16_slabs=sbf)
    cdf = 0.5 * (1 + torch.erf(p / 2 ** 0.5))
    dgelu = cdf + p * torch.exp(-0.5 * p * p) / (2 * torch.pi) ** 0.5
    dpre64 = dact64 * dgelu
    e = e_dact * dgelu.abs() + (2e-7 * (1 + p.abs()) + 16 * fb.U32) * dact64.abs() + 1e-30
    fb.assert_within(dpre, dpre64, e + fb.U16 * (dpre64.abs() + e), "dpre")
