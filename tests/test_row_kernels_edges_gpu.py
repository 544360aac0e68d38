"""Norm, loss, activation and data-movement kernels (csrc/norm.hip, loss.hip, elementwise.hip, l2norm_rows) element by element
against float64, at the widths, strides and inputs where such kernels go wrong.  Outputs start as NaN poison (the wrappers' own
allocations through poisoned_allocations, strided outputs as a window of a wider, taller poisoned buffer whose frame must stay
untouched); every element is compared with tests/fp64_bounds.py's bound for that kernel (tests/test_fp64_bounds_cpu.py shows
that a torch emulation passes each bound and that the plausible mistakes fail it).  Pure data movement is torch.equal.

Launch paths only these tests reach (each can only pass through the named kernel):
    rmsnorm_bwd_kernel<8>            test_rmsnorm_rows at D = 4100, 8192 (mh_rmsnorm_bwd launches <8> for every D > 4096)
    layernorm_bwd_kernel<4>/<8>,     test_layernorm_slab_backward_wide_rows at N = 3072 / 5120 (ops.gemm_layernorm_bwd is the only
      more than one slab             caller that hands the kernel split-K slabs; <4> for 2048 < N <= 4096, <8> above)
    clamp_ce_kernel (256 threads)    test_clamp_ce_edges: V = 50000 and 32772 (> 32768), the `ldl % 4 != 0` view and the
                                     4-byte-offset base at every V (the launcher's conditions for the register-resident kernel fail)

Math-function allowances (fp64_bounds.C_FN = 4 ulp for expf / logf / rsqrtf / sqrtf / division, (4 + 2 |a|) u32 for __expf) are
stated assumptions: no accuracy table of the HIP math functions is installed with the toolchain this was written against.

Worst err / bound per kernel, from one run of this module on an MI355X (the value assert_within returns; `-s` prints them):
    argmax margin                               0
    argmax p_max                                0.0242
    clamp_ce (256-thread) dlogits bf16          0.993
    clamp_ce (256-thread) row_loss              0.347
    clamp_ce dlogits bf16                       0.993
    clamp_ce row_loss                           0.347
    dropout_add_                                0.988
    dropout_bf16                                0.879
    gelu_bwd bf16                               0.996
    gelu_fwd bf16                               0.975
    l2norm_rows bf16                            0.996
    l2norm_rows f32                             0.153
    layernorm_bwd bf16                          0.996
    layernorm_bwd f32                           0.249
    layernorm_bwd_slab bf16                     0.996
    layernorm_bwd_slab f32                      0.249
    layernorm_fwd bf16                          0.996
    layernorm_fwd f32                           0.481
    layernorm_param_grads dbeta accumulate      0.39
    layernorm_param_grads dbeta f32             0.129
    layernorm_param_grads dgamma accumulate     0.683
    layernorm_param_grads dgamma f32            0.0533
    lowrank dA f32                              0.039
    lowrank dB f32                              0.0853
    lowrank dx f32                              0.288
    lowrank t f32                               0.021
    lowrank y f32                               0.298
    rmsnorm_bwd bf16                            0.996
    rmsnorm_bwd f32                             0.498
    rmsnorm_fwd bf16                            0.996
    silu_mul_bwd dgate bf16                     0.996
    silu_mul_bwd dup bf16                       0.996
    silu_mul_fwd bf16                           0.996
    sum_f32                                     0.0838
    rope_                                     bf16-valued reference: exact but for the ambiguous elements (at most 1 %, asserted)
Outputs rounded to bf16 reach ~1.0 by construction -- the bound's last term is the half-ulp of the correctly rounded result,
attained at the bottom of a binade -- so for them the factor-two head-room criterion cannot hold together with a bound that
still catches a one-ulp error (dropout_add_'s bound is likewise nothing but the half-ulps of its product and its sum, and an
accumulate form's is the half-ulp of the sum onto the earlier value wherever that value dwarfs what is added); every
other fp32 output, which shares the arithmetic of its bf16 twin, is held to <= 0.5 by note().
"""
import pytest
import torch

from myriad_amd import _lib, ops
from tests import fp64_bounds as fb
from tests.fp64_bounds import assert_frame_untouched, assert_untouched, assert_within, poisoned, poisoned_allocations

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
WORST = {}


# bounds whose last term is the half-ulp of one correct rounding (the bf16 output's, or the fp32 sum onto an earlier value where
# that value dwarfs what is added): err / bound approaches 1 by construction
HALF_ULP_ONLY = ("bf16", "dropout_add_", "accumulate")


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


# ------------------------------------------------------------------------------------------------------------------ norms
NORM_D = [4, 252, 256, 1028, 1408, 4096, 4100, 8192]
NORM_M = [1, 5, 300]
NORM_EPS = [1e-6, 1e-5, 1e-12]


def _norm_eps(M, D):
    """All three eps values where the rows are few (M = 5 holds the all-zero and the constant row), one in rotation elsewhere."""
    return NORM_EPS if M == 5 else [NORM_EPS[(NORM_D.index(D) + NORM_M.index(M)) % 3]]


def _norm_inputs(M, D):
    x, w = fb.norm_rows(M, D, seed=100 + D), fb.norm_weight(D, seed=200 + D)
    dy, dres = fb.rnd(M, D, seed=300 + D), fb.rnd(M, D, seed=400 + D)
    return dev(x), dev(w), dev(dy), dev(dres)


@pytest.mark.parametrize("D", NORM_D)
@pytest.mark.parametrize("M", NORM_M)
def test_rmsnorm_rows(M, D, monkeypatch):
    """Forward into a bordered window; backward with and without dres, f32 and bf16 outputs.  D > 4096 runs rmsnorm_bwd_kernel<8>."""
    x, w, dy, dres = _norm_inputs(M, D)
    for eps in _norm_eps(M, D):
        _rmsnorm_rows(M, D, eps, x, w, dy, dres, monkeypatch)


def _rmsnorm_rows(M, D, eps, x, w, dy, dres, monkeypatch):
    r = fb.rmsnorm_ref_bound(x, w, eps, dy=dy, dres=dres)
    buf = poisoned((M + 2, D + 72), BF16, DEV)
    rows, cols = slice(1, M + 1), slice(8, 8 + D)
    ops.rmsnorm_fwd(x, w, eps, out=buf[rows, cols])
    sync()
    note("rmsnorm_fwd bf16", assert_within(buf[rows, cols], r["y"], r["y_bf16_bound"], "rmsnorm_fwd"))
    assert_frame_untouched(buf, rows, cols, "rmsnorm_fwd")
    with poisoned_allocations(monkeypatch):
        y = ops.rmsnorm_fwd(x, w, eps)
        dx, dxb = ops.rmsnorm_bwd(dy, x, w, eps, dres=dres, want_bf16=True)
        dx0, none = ops.rmsnorm_bwd(dy, x, w, eps)
        _, dxb0 = ops.rmsnorm_bwd(dy, x, w, eps, dres=dres, want_f32=False, want_bf16=True)
    sync()
    assert none is None and torch.equal(y, buf[rows, cols]) and torch.equal(dxb0, dxb)
    note("rmsnorm_bwd f32", assert_within(dx, r["dx"], r["dx_bound"], "rmsnorm_bwd dx"))
    note("rmsnorm_bwd bf16", assert_within(dxb, r["dx"], r["dx_bf16_bound"], "rmsnorm_bwd dx bf16"))
    r0 = fb.rmsnorm_ref_bound(x, w, eps, dy=dy)
    note("rmsnorm_bwd f32", assert_within(dx0, r0["dx"], r0["dx_bound"], "rmsnorm_bwd dx (no dres)"))


@pytest.mark.parametrize("D", NORM_D)
@pytest.mark.parametrize("M", NORM_M)
def test_layernorm_rows(M, D, monkeypatch):
    x, w, dy, dres = _norm_inputs(M, D)
    for eps in _norm_eps(M, D):
        _layernorm_rows(M, D, eps, x, w, dy, dres, monkeypatch)


def _layernorm_rows(M, D, eps, x, w, dy, dres, monkeypatch):
    b = dev(0.1 * fb.rnd(D, seed=500 + D))
    r = fb.layernorm_ref_bound(x, w, b, eps, dy=dy, dres=dres)
    with poisoned_allocations(monkeypatch):
        yb, yf = ops.layernorm_fwd(x, w, b, eps, want_bf16=True, want_f32=True)
        yb1, none = ops.layernorm_fwd(x, w, b, eps)
        dx, dxb = ops.layernorm_bwd(dy, x, w, eps, dres=dres, want_bf16=True)
        dx0, _ = ops.layernorm_bwd(dy, x, w, eps)
    sync()
    assert none is None and torch.equal(yb1, yb)
    note("layernorm_fwd f32", assert_within(yf, r["y"], r["y_bound"], "layernorm_fwd f32"))
    note("layernorm_fwd bf16", assert_within(yb, r["y"], r["y_bf16_bound"], "layernorm_fwd bf16"))
    note("layernorm_bwd f32", assert_within(dx, r["dx"], r["dx_bound"], "layernorm_bwd dx"))
    note("layernorm_bwd bf16", assert_within(dxb, r["dx"], r["dx_bf16_bound"], "layernorm_bwd dx bf16"))
    r0 = fb.layernorm_ref_bound(x, w, None, eps, dy=dy)
    note("layernorm_bwd f32", assert_within(dx0, r0["dx"], r0["dx_bound"], "layernorm_bwd dx (no dres)"))


@pytest.mark.parametrize("M,N,K", [(1028, 3072, 4096), (1028, 5120, 4096)])
def test_layernorm_slab_backward_wide_rows(M, N, K, monkeypatch):
    """ops.gemm_layernorm_bwd with a split K at 2048 < N <= 4096 (layernorm_bwd_kernel<4>) and N > 4096 (<8>): the bits of
    gemm + layernorm_bwd (the same kernel with one slab), and that within the float64 bound given the dY the GEMM produced."""
    ops.ensure_workspace(DEV)
    assert ops.gemm_plan(M, N, K, out_f32=True)[1] > 1                      # K is split: the norm kernel reads the slabs
    a, bw = dev(fb.rnd(M, K, seed=1).to(BF16)), dev((fb.rnd(N, K, seed=2) * 0.05).to(BF16))
    x, w, dres = dev(fb.norm_rows(M, N, seed=3)), dev(fb.norm_weight(N, seed=4)), dev(fb.rnd(M, N, seed=5))
    with poisoned_allocations(monkeypatch):
        dx, dxb = ops.gemm_layernorm_bwd(a, bw, x, w, 1e-6, dres=dres)
        dy = ops.gemm(a, bw, out_dtype=F32)
        rx, rxb = ops.layernorm_bwd(dy, x, w, 1e-6, dres=dres, want_bf16=True)
    sync()
    assert torch.equal(dx, rx) and torch.equal(dxb, rxb)
    r = fb.layernorm_ref_bound(x, w, None, 1e-6, dy=dy, dres=dres)
    note("layernorm_bwd_slab f32", assert_within(dx, r["dx"], r["dx_bound"], "gemm_layernorm_bwd dx"))
    note("layernorm_bwd_slab bf16", assert_within(dxb, r["dx"], r["dx_bf16_bound"], "gemm_layernorm_bwd dx bf16"))


@pytest.mark.parametrize("D", [768, 1408, 2052, 8192])
def test_layernorm_backward_single_slab_every_instantiation(D, monkeypatch):
    """ops.layernorm_bwd (layernorm_bwd_kernel with one slab) with and without dres at the product's widths (768: Q-Former,
    1408: ViT; both <2>) and at the first width of <4> (2052) and the last of <8> (8192), against the float64 bound."""
    M, eps = 37, 1e-6
    x, w, dy, dres = _norm_inputs(M, D)
    with poisoned_allocations(monkeypatch):
        dx, dxb = ops.layernorm_bwd(dy, x, w, eps, dres=dres, want_bf16=True)
        dx0, dxb0 = ops.layernorm_bwd(dy, x, w, eps, want_bf16=True)
    sync()
    for got, gotb, r, what in ((dx, dxb, fb.layernorm_ref_bound(x, w, None, eps, dy=dy, dres=dres), "dres"),
                               (dx0, dxb0, fb.layernorm_ref_bound(x, w, None, eps, dy=dy), "no dres")):
        note("layernorm_bwd f32", assert_within(got, r["dx"], r["dx_bound"], f"layernorm_bwd dx ({what})"))
        note("layernorm_bwd bf16", assert_within(gotb, r["dx"], r["dx_bf16_bound"], f"layernorm_bwd dx bf16 ({what})"))


@pytest.mark.parametrize("D", NORM_D)
@pytest.mark.parametrize("M", NORM_M)
def test_layernorm_param_grads(M, D, monkeypatch):
    """dgamma / dbeta over the norm tests' rows: plain, accumulated onto earlier values, and with the output-dropout mask; the
    partial-sum scratch the wrapper allocates starts poisoned.  The kernel holds a column block in registers: D > 4096 must raise."""
    x, _, dy, _ = _norm_inputs(M, D)
    if D > 4096:
        dg, db = poisoned((D,), F32, DEV), poisoned((D,), F32, DEV)
        with pytest.raises(_lib.MyriadHipError):
            ops.layernorm_param_grads(dy, x, 1e-6, dg, db)
        sync()
        assert_untouched(dg), assert_untouched(db)
        return
    p, seed = 0.1, 4242 + D
    keep = ops.dropout_keep_mask(M * D, p, seed, DEV).view(M, D)
    for eps in _norm_eps(M, D):
        buf = poisoned((2, D + 8), F32, DEV)
        dg, db = buf[0, 4:4 + D], buf[1, 4:4 + D]
        with poisoned_allocations(monkeypatch):
            ops.layernorm_param_grads(dy, x, eps, dg, db)
        sync()
        rg, eg, rb, eb = fb.layernorm_param_grads_ref_bound(dy, x, eps)
        note("layernorm_param_grads dgamma f32", assert_within(dg, rg, eg, "dgamma"))
        note("layernorm_param_grads dbeta f32", assert_within(db, rb, eb, "dbeta"))
        prev = (dg.clone(), db.clone())
        with poisoned_allocations(monkeypatch):
            ops.layernorm_param_grads(dy, x, eps, dg, db, accumulate=True, p_out=p, seed_out=seed)
        sync()
        rg, eg, rb, eb = fb.layernorm_param_grads_ref_bound(dy, x, eps, keep=keep, prev=prev)
        note("layernorm_param_grads dgamma accumulate", assert_within(dg, rg, eg, "dgamma (accumulate, p_out)"))
        note("layernorm_param_grads dbeta accumulate", assert_within(db, rb, eb, "dbeta (accumulate, p_out)"))
        dg2, db2 = torch.empty_like(rg, dtype=F32), torch.empty_like(rb, dtype=F32)
        with poisoned_allocations(monkeypatch):                           # the dropout form on its own: nothing to round onto
            ops.layernorm_param_grads(dy, x, eps, dg2, db2, p_out=p, seed_out=seed)
        sync()
        rg, eg, rb, eb = fb.layernorm_param_grads_ref_bound(dy, x, eps, keep=keep)
        note("layernorm_param_grads dgamma f32", assert_within(dg2, rg, eg, "dgamma (p_out)"))
        note("layernorm_param_grads dbeta f32", assert_within(db2, rb, eb, "dbeta (p_out)"))
        assert_untouched(buf[:, :4]), assert_untouched(buf[:, 4 + D:])


@pytest.mark.parametrize("M,D,R", [(1, 68, 2), (5, 64, 1), (37, 300, 4), (130, 1000, 8), (514, 1408, 4)])
def test_lowrank_adaptor_rows(M, D, R, monkeypatch):
    """y, t, dx, dA, dB of the rank-R adaptor against float64: one row, widths that are no multiple of 64 (the ragged last
    column block of the weight-gradient kernel), fewer rows than row chunks, and a gradient that cancels over the rows.  Outputs
    and the dt / partial-slab scratch start poisoned."""
    x = dev(fb.rnd(M, D, seed=M))
    A, Bm = dev(fb.rnd(R, D, seed=M + 1) * 0.05), dev(fb.rnd(D, R, seed=M + 2) * 0.05)
    dyh = fb.rnd(M, D, seed=M + 3)
    dyh[1::2] = -dyh[::2][:M // 2] * (1 + 2 ** -10)
    dy = dev(dyh)
    dA, dB = poisoned((R, D), F32, DEV), poisoned((D, R), F32, DEV)
    with poisoned_allocations(monkeypatch):
        y, t = ops.lowrank_fwd(x, A, Bm)
        dx = ops.lowrank_bwd(dy, x, t, A, Bm, dA, dB, need_dx=True)
        dA2, dB2 = torch.empty_like(dA), torch.empty_like(dB)
        none = ops.lowrank_bwd(dy, x, t, A, Bm, dA2, dB2)
    sync()
    assert none is None and torch.equal(dA2, dA) and torch.equal(dB2, dB)
    r = fb.lowrank_ref_bound(x, A, Bm, dy, t_in=t)
    for k, got in (("t", t), ("y", y), ("dx", dx), ("dA", dA), ("dB", dB)):
        note(f"lowrank {k} f32", assert_within(got, r[k], r[k + "_bound"], "lowrank " + k))
    with pytest.raises(_lib.MyriadHipError):
        ops.lowrank_fwd(x, A[:1].repeat(3, 1), Bm[:, :1].repeat(1, 3))      # R = 3 is not a compiled rank


@pytest.mark.parametrize("M,D", [(1, 4), (5, 252), (300, 768), (7, 1028)])
def test_l2norm_rows(M, D, monkeypatch):
    x = fb.norm_rows(M, D, seed=D)
    wide = dev(torch.cat([x, fb.rnd(M, 12, seed=9)], 1))                  # a strided source
    with poisoned_allocations(monkeypatch):
        yb, yf = ops.l2norm_rows(wide[:, :D], want_bf16=True, want_f32=True)
    sync()
    ref, e, eb = fb.l2norm_ref_bound(x.to(DEV), 1e-12)
    note("l2norm_rows f32", assert_within(yf, ref, e, "l2norm f32"))
    note("l2norm_rows bf16", assert_within(yb, ref, eb, "l2norm bf16"))


def test_norm_launchers_reject_bad_widths_and_leave_the_output_alone():
    M = 3
    w, b = torch.ones(8200, device=DEV), torch.zeros(8200, device=DEV)
    x250, x8196 = torch.ones(M, 250, device=DEV), torch.ones(M, 8196, device=DEV)
    out = poisoned((M, 256), BF16, DEV)
    with pytest.raises(_lib.MyriadHipError):
        ops.rmsnorm_fwd(x250, w, 1e-6, out=out[:, :250])                 # D % 4
    x256 = torch.ones(M, 256, device=DEV)
    with pytest.raises(_lib.MyriadHipError):
        ops.rmsnorm_fwd(x256, w, 1e-6, out=out.view(-1)[:M * 252].view(M, 252))     # ldy < D
    with pytest.raises(_lib.MyriadHipError):
        ops.rmsnorm_fwd(x256, w, 1e-6, out=poisoned((M, 258), BF16, DEV)[:, :256])  # ldy % 4
    for fn in (lambda: ops.rmsnorm_bwd(x250, x250, w, 1e-6), lambda: ops.rmsnorm_bwd(x8196, x8196, w, 1e-6),
               lambda: ops.layernorm_fwd(x250, w, b, 1e-6), lambda: ops.layernorm_bwd(x250, x250, w, 1e-6),
               lambda: ops.l2norm_rows(x250)):
        with pytest.raises(_lib.MyriadHipError):
            fn()
    a = torch.zeros(M, 64, dtype=BF16, device=DEV)
    with pytest.raises(_lib.MyriadHipError):                                # the slab backward's D <= 8192
        ops.gemm_layernorm_bwd(a, torch.zeros(8256, 64, dtype=BF16, device=DEV), torch.ones(M, 8256, device=DEV),
                               torch.ones(8256, device=DEV), 1e-6)
    # mh_layernorm_bwd holds the row in registers: D > 8192 is MH_ERR_ARG (-1) at the entry itself, outputs untouched
    dx, dxb = poisoned((M, 8196), F32, DEV), poisoned((M, 8196), BF16, DEV)
    rc = ops._L().mh_layernorm_bwd(x8196.data_ptr(), x8196.data_ptr(), w.data_ptr(), 0, dx.data_ptr(), dxb.data_ptr(), M, 8196,
                                   1e-6, torch.cuda.current_stream().cuda_stream)
    assert rc == -1
    with pytest.raises(_lib.MyriadHipError):
        ops.layernorm_bwd(x8196, x8196, w, 1e-6)
    sync()
    assert_untouched(dx, "layernorm_bwd dx at D = 8196"), assert_untouched(dxb, "layernorm_bwd dx bf16 at D = 8196")
    assert_untouched(out, "rmsnorm_fwd out after rejected launches")


# --------------------------------------------------------------------------------------------------------------- clamp-CE
CE_V = [320, 1001, 32000, 32001, 32768, 32772, 50000]
CE_R = 12


def _clamp_ce_into(x, y, gs, ldd, want_grad=True):
    """mh_clamp_ce with row_loss and dlogits as the middle rows of taller poisoned buffers; returns (loss, dlog or None)."""
    R, V = x.shape
    lbuf = poisoned((R + 16,), F32, DEV)
    dbuf = poisoned((R + 2, ldd), BF16, DEV) if want_grad else None
    rc = ops._L().mh_clamp_ce(x.data_ptr(), x.stride(0), y.data_ptr(), lbuf[8:].data_ptr(), dbuf[1:].data_ptr() if want_grad else 0,
                              ldd, R, V, float(gs), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "mh_clamp_ce")
    sync()
    assert_untouched(lbuf[:8], "row_loss before")
    assert_untouched(lbuf[8 + R:], "row_loss after")
    if want_grad:
        assert_untouched(dbuf[0], "dlogits row above")
        assert_untouched(dbuf[R + 1], "dlogits row below")
    return lbuf[8:8 + R], dbuf[1:R + 1] if want_grad else None


@pytest.mark.parametrize("V", CE_V)
def test_clamp_ce_edges(V, monkeypatch):
    """Both kernels against float64 at every V: the register-resident one where the launcher allows it (V <= 32768, aligned),
    the 256-thread clamp_ce_kernel for V > 32768, for a logits view with ldl % 4 != 0 and for a base 4 bytes off 16-byte
    alignment (at V = 320 these last two can only pass through the 256-thread kernel)."""
    xh, yh = fb.ce_case(CE_R, V, seed=V)
    gs = 1.0 / 7
    x, y = dev(xh), dev(yh)
    losses = []
    for ldd in (V, ops.round_up(V, 64), V + 4):
        r = fb.clamp_ce_ref_bound(x, y, gs, ldd=ldd)
        assert int(r["amb"].sum()) == 0
        loss, d = _clamp_ce_into(x, y, gs, ldd)
        a, b = fb.clamp_ce_check(loss, d, r, f"clamp_ce V={V} ldd={ldd}")
        note("clamp_ce row_loss", a), note("clamp_ce dlogits bf16", b)
        losses.append(loss)
    r = fb.clamp_ce_ref_bound(x, y, gs, ldd=ops.round_up(V, 64))
    odd = poisoned((CE_R, V + 1 if (V + 1) % 4 else V + 2), F32, DEV)      # ldl % 4 != 0
    odd[:, :V] = x
    flat = poisoned((CE_R * (V + 4) + 1,), F32, DEV)                       # rows 16-byte strided, base 4 bytes off
    off = flat[1:].view(CE_R, V + 4)[:, :V]
    off.copy_(x)
    for name, view in (("ldl % 4", odd[:, :V]), ("offset base", off)):
        assert view.stride(0) % 4 or view.data_ptr() % 16
        loss, d = _clamp_ce_into(view, y, gs, ops.round_up(V, 64))
        a, b = fb.clamp_ce_check(loss, d, r, f"clamp_ce V={V} {name}")
        note("clamp_ce (256-thread) row_loss", a), note("clamp_ce (256-thread) dlogits bf16", b)
        # the two kernels sum in different orders: they agree within twice the bound, not bit for bit
        assert_within(loss, losses[1], 2 * r["loss_bound"], "the two clamp_ce kernels' row_loss")
    loss, none = _clamp_ce_into(x, y, gs, 0, want_grad=False)
    fb.clamp_ce_check(loss, None, r, "clamp_ce want_grad=False")
    with poisoned_allocations(monkeypatch):                                # the wrapper's own allocations
        wl, wd = ops.clamp_ce(x, y, gs)
        wl2, wd2 = ops.clamp_ce(x, y, gs, want_grad=False)
        total = ops.sum_f32(wl, 0.25)
    sync()
    assert wd2 is None and wd.shape == (CE_R, ops.round_up(V, 64))
    fb.clamp_ce_check(wl, wd, r, "ops.clamp_ce"), fb.clamp_ce_check(wl2, None, r, "ops.clamp_ce want_grad=False")
    sref, sb = fb.sum_ref_bound(wl, 0.25)
    note("sum_f32", assert_within(total, sref.reshape(1), sb.reshape(1), "sum_f32"))
    # saturated / unlabelled rows carry exactly zero gradient and the documented losses
    assert float(wd[[3, 4, 6, 7, 8]].float().abs().max()) == 0 and float(wl[3]) == 0 and float(wl[4]) == 0


def test_sum_f32_long_and_cancelling():
    x = fb.rnd(100003, seed=7)
    x[1::2] = -x[::2][:50001] * (1 + 2 ** -10)                              # nearly cancelling pairs: |sum| << sum |x|
    xd = dev(x)
    got = ops.sum_f32(xd, 3.0)
    ref, b = fb.sum_ref_bound(xd, 3.0)
    note("sum_f32", assert_within(got, ref.reshape(1), b.reshape(1), "sum_f32"))


def test_clamp_ce_rejects_a_short_gradient_stride():
    x, y = dev(fb.rnd(4, 320, seed=1)), torch.zeros(4, dtype=torch.long, device=DEV)
    loss, d = poisoned((4,), F32, DEV), poisoned((4, 320), BF16, DEV)
    rc = ops._L().mh_clamp_ce(x.data_ptr(), 320, y.data_ptr(), loss.data_ptr(), d.data_ptr(), 316, 4, 320, 1.0,
                              torch.cuda.current_stream().cuda_stream)
    sync()
    assert rc != 0
    assert_untouched(loss, "row_loss"), assert_untouched(d, "dlogits")


@pytest.mark.parametrize("V", CE_V)
def test_argmax_and_pmax_edges(V):
    R = 6
    xh = fb.rnd(R, V, seed=V + 1) * 3
    xh[0, V - 1] = xh[0].max() + 1.0                                       # the maximum in the last (partial) float4
    xh[1, V // 3] = xh[1].max() + 1.0
    xh[1, V // 3 + 7] = xh[1, V // 3]                                      # a tie: first index, margin 0
    ban = V - 2
    xh[2, ban] = xh[2].max() + 5.0                                         # the banned id would have won
    xh[3, 5] = float("-inf")
    x = dev(xh)
    odd = poisoned((R, V + 1), F32, DEV)
    odd[:, :V] = x
    for inv_temp in (1.0, 0.7):
        ids_r, mar_r, mar_b, pm_r, pm_b = (dev(t) for t in fb.argmax_ref(xh, ban, inv_temp))   # torch.argmax on the host
        for view in (x, odd[:, :V]):                                       # register-resident kernel / the two scans
            mar, pm = poisoned((R + 2,), F32, DEV), poisoned((R + 2,), F32, DEV)
            ids64 = torch.full((R + 2,), -7, dtype=torch.long, device=DEV)
            ops.argmax_pmax_rows(view, ids64[1:R + 1], mar[1:R + 1], pm[1:R + 1], ban_id=ban, inv_temp=inv_temp)
            sync()
            assert torch.equal(ids64[1:R + 1], ids_r) and ids64[0] == -7 and ids64[R + 1] == -7
            note("argmax margin", assert_within(mar[1:R + 1], mar_r, mar_b, "margin"))
            note("argmax p_max", assert_within(pm[1:R + 1], pm_r, pm_b, "p_max"))
            assert_untouched(mar[:1]), assert_untouched(mar[R + 1:]), assert_untouched(pm[:1]), assert_untouched(pm[R + 1:])
    ids_r, mar_r, mar_b, _, _ = (dev(t) for t in fb.argmax_ref(xh, ban))
    for view in (x, odd[:, :V]):
        ids, mar = ops.argmax_rows(view, ban_id=ban, want_margin=True)
        sync()
        assert torch.equal(ids, ids_r) and float(mar[1]) == 0.0
        assert_within(mar, mar_r, mar_b, "argmax_rows margin")


# ------------------------------------------------------------------------------------------------------------ elementwise
WRAP_ROWS = 132_113            # x 16 items a row = 2 113 808 items: two full sweeps of the 4096 x 256 grid and a ragged third


def _ew_values(*shape, seed):
    """bf16 values spanning +-30 (both saturation sides) among N(0, 1)."""
    x = fb.rnd(*shape, seed=seed)
    flat = x.view(-1)
    flat[::7] *= 10
    flat[0], flat[1], flat[2], flat[3] = 30.0, -30.0, 0.0, -0.0
    flat[-1], flat[-2] = -30.0, 30.0
    return x.to(BF16)


def _in_row_chunks(M, fn, step=16384):
    for r0 in range(0, M, step):
        fn(slice(r0, min(M, r0 + step)))


@pytest.mark.parametrize("M,I", [(1, 8), (5, 256), (WRAP_ROWS, 128)])
@pytest.mark.parametrize("blk", [0, 128])
def test_silu_mul_fwd_bwd(M, I, blk, monkeypatch):
    assert M * I // 8 > fb.EW_WRAP or M < 100
    if blk and I % blk:
        blk = 8                                                             # the tiny shape: blocks of 8 columns
    gu, dh = dev(_ew_values(M, 2 * I, seed=11)), dev(_ew_values(M, I, seed=12))
    with poisoned_allocations(monkeypatch):
        if blk:
            h, dgu = ops.silu_mul_fwd_blk(gu, blk), ops.silu_mul_bwd_blk(dh, gu, blk)
        else:
            h, dgu = ops.silu_mul_fwd(gu), ops.silu_mul_bwd(dh, gu)
    sync()
    c = torch.arange(I, device=DEV)
    gc = c if blk == 0 else (c // blk) * 2 * blk + c % blk
    us = I if blk == 0 else blk

    def check(rs):
        rh, bh, rg, bg, ru, bu = fb.silu_mul_ref_bound(gu[rs][:, gc], gu[rs][:, gc + us], dh[rs])
        note("silu_mul_fwd bf16", assert_within(h[rs], rh, bh, "silu_mul_fwd"))
        note("silu_mul_bwd dgate bf16", assert_within(dgu[rs][:, gc], rg, bg, "silu_mul_bwd dgate"))
        note("silu_mul_bwd dup bf16", assert_within(dgu[rs][:, gc + us], ru, bu, "silu_mul_bwd dup"))
    _in_row_chunks(M, check)


@pytest.mark.parametrize("M,N", [(1, 8), (WRAP_ROWS, 128)])
def test_gelu_fwd_bwd(M, N, monkeypatch):
    x, dy = dev(_ew_values(M, N, seed=13)), dev(_ew_values(M, N, seed=14))
    with poisoned_allocations(monkeypatch):
        y, dx = ops.gelu_fwd(x), ops.gelu_bwd(dy, x)
    sync()

    def check(rs):
        note("gelu_fwd bf16", assert_within(y[rs], *fb.gelu_ref_bound(x[rs]), "gelu_fwd"))
        note("gelu_bwd bf16", assert_within(dx[rs], *fb.gelu_ref_bound(x[rs], dy[rs]), "gelu_bwd"))
    _in_row_chunks(M, check)


@pytest.mark.parametrize("n_tok,nh,d,col0,extra", [(3, 1, 64, 0, 0), (37, 3, 88, 8, 24), (70, 2, 128, 128, 8), (16520, 8, 128, 0, 64)])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_rope_rows(n_tok, nh, d, col0, extra, sign):
    """In place on the heads' columns only: the columns before col0 and after the heads (the v part of a qkv row) keep their bits."""
    ld = col0 + nh * d + extra
    xh = fb.rnd(n_tok, ld, seed=21).to(BF16)
    cos, sin = fb.rope_tables(d, 96)
    pos = torch.randint(0, 96, (n_tok,), generator=torch.Generator().manual_seed(3)).int()     # non-monotone, repeated
    pos[:2] = 0
    x = dev(xh)
    refs = [fb.rope_rows_ref(x[t0:t0 + 4096], col0, nh, d, dev(pos[t0:t0 + 4096]), dev(cos), dev(sin), sign)
            for t0 in range(0, n_tok, 4096)]                                # in token chunks: the float64 temporaries stay small
    ref, amb = torch.cat([r[0].float() for r in refs]), torch.cat([r[1].float() for r in refs])
    del refs
    share = float((amb > 0).double().mean())
    assert share <= 0.01, share
    ops.rope_(x, col0, nh, d, dev(pos), dev(cos), dev(sin), sign)
    sync()
    assert_within(x[:, col0:col0 + nh * d], ref, amb, "rope_")
    assert torch.equal(x[:, :col0].cpu(), xh[:, :col0]) and torch.equal(x[:, col0 + nh * d:].cpu(), xh[:, col0 + nh * d:])
    if n_tok > 10000:
        assert n_tok * nh * d // 8 > fb.EW_WRAP


def test_rope_rejects_bad_shapes_and_leaves_the_rows_alone():
    cos, sin = (dev(t) for t in fb.rope_tables(64, 16))
    pos = torch.zeros(4, dtype=I32, device=DEV)
    for ld, col0, d in ((3 * 68 + 8, 0, 68), (206, 0, 64), (208, 6, 64)):   # head_dim % 8, ld % 4, col0 % 4
        x = poisoned((4, ld), BF16, DEV)
        with pytest.raises(_lib.MyriadHipError):
            ops.rope_(x, col0, 3, d, pos, cos, sin)
        sync()
        assert_untouched(x, "rope_ after a rejected launch")


def test_dropout_kernels_match_the_library_mask(monkeypatch):
    rows, cols, p, seed = WRAP_ROWS, 128, 0.1, 1234567
    src = dev(fb.rnd(rows, cols + 8, seed=31).to(BF16))
    mask = ops.dropout_keep_mask(rows * cols, p, seed, DEV).view(rows, cols)
    with poisoned_allocations(monkeypatch):
        y = ops.dropout_bf16(src[:, :cols], p, seed)
        ones = ops.dropout_bf16(torch.ones(64, cols, dtype=BF16, device=DEV), p, seed)
    sync()
    assert torch.equal(ones, mask[:64].to(BF16)) and 0.85 < float((mask > 0).float().mean()) < 0.95
    ref = src[:, :cols].double() * mask.double()
    note("dropout_bf16", assert_within(y, ref, fb.bf16_out(ref, fb.U32 * ref.abs()), "dropout_bf16"))
    rows4, cols4 = WRAP_ROWS, 64
    dy = dev(fb.rnd(rows4, cols4 + 4, seed=32))
    buf = poisoned((rows4 + 2, cols4 + 8), F32, DEV)
    acc0 = dev(fb.rnd(rows4, cols4, seed=33))
    rs, cs = slice(1, rows4 + 1), slice(4, 4 + cols4)
    buf[rs, cs] = acc0
    m4 = ops.dropout_keep_mask(rows4 * cols4, p, seed + 1, DEV).view(rows4, cols4)
    ops.dropout_add_(dy[:, :cols4], buf[rs, cs], p, seed + 1)
    sync()
    add = dy[:, :cols4].double() * m4.double()
    ref = acc0.double() + add
    note("dropout_add_", assert_within(buf[rs, cs], ref, fb.U32 * (add.abs() + ref.abs()), "dropout_add_"))   # product, then sum
    assert_frame_untouched(buf, rs, cs, "dropout_add_")
    for bad_p in (1.0, 1.5):
        with pytest.raises(_lib.MyriadHipError):
            ops.dropout_add_(dy[:, :cols4], buf[rs, cs], bad_p, seed)
        with pytest.raises(_lib.MyriadHipError):
            ops.dropout_bf16(src[:, :cols], bad_p, seed)
    sync()
    assert_frame_untouched(buf, rs, cs, "dropout_add_ after rejected launches")


# ---------------------------------------------------------------------------------------------------------- data movement
def _ids(n, hi, seed):
    """Row indices with duplicates, out of order."""
    t = torch.randint(0, hi, (n,), generator=torch.Generator().manual_seed(seed)).int()
    t[:3] = torch.tensor([hi - 1, 0, hi - 1])[:min(3, n)]
    return dev(t)


@pytest.mark.parametrize("rows", [2, WRAP_ROWS])
def test_copy2d_copy3d_and_casts(rows):
    cols = 64
    src = dev(fb.rnd(rows, cols + 12, seed=41))
    buf = poisoned((rows + 2, cols + 20), F32, DEV)
    rs, cs = slice(1, rows + 1), slice(8, 8 + cols)
    ops.copy2d(src[:, 4:4 + cols], buf[rs, cs])
    sync()
    assert torch.equal(buf[rs, cs], src[:, 4:4 + cols])
    for k in (2, 3):                                                        # accumulate twice
        ops.copy2d(src[:, 4:4 + cols], buf[rs, cs], accumulate=True)
        sync()
        assert torch.equal(buf[rs, cs], k * src[:, 4:4 + cols])             # x + x and 2x + x: one rounding each, as torch
    assert_frame_untouched(buf, rs, cs, "copy2d")
    with pytest.raises(_lib.MyriadHipError):
        ops.copy2d(src[:, :62], buf[rs, 8:70])
    nb = 3
    r3 = -(-rows // nb)
    s3 = dev(fb.rnd(nb, r3 + 2, cols + 4, seed=42))
    b3 = poisoned((nb, r3 + 3, cols + 8), F32, DEV)
    ops.copy3d(s3[:, 1:r3 + 1, :cols], b3[:, 2:r3 + 2, 4:4 + cols])
    ops.copy3d(s3[:, 1:r3 + 1, :cols], b3[:, 2:r3 + 2, 4:4 + cols], accumulate=True)
    sync()
    assert torch.equal(b3[:, 2:r3 + 2, 4:4 + cols], 2 * s3[:, 1:r3 + 1, :cols])
    assert_frame_untouched(b3, slice(2, r3 + 2), slice(4, 4 + cols), "copy3d")
    sb = dev(fb.rnd(nb, r3 + 2, 136, seed=43).to(BF16))
    bb = poisoned((nb, r3 + 3, 144), BF16, DEV)
    ops.copy3d_bf16(sb[:, 1:r3 + 1, 8:136], bb[:, 2:r3 + 2, 8:136])
    sync()
    assert torch.equal(bb[:, 2:r3 + 2, 8:136], sb[:, 1:r3 + 1, 8:136])
    assert_frame_untouched(bb, slice(2, r3 + 2), slice(8, 136), "copy3d_bf16")
    with pytest.raises(_lib.MyriadHipError):
        ops.copy3d_bf16(sb[:, 1:r3 + 1, 8:132], bb[:, 2:r3 + 2, 8:132])
    dense = src[:, :cols].contiguous()
    dense[0, :4] = torch.tensor([1 + 2 ** -8, 1 + 3 * 2 ** -8, -(1 + 2 ** -8), 3.0e38], device=DEV)   # ties to even, near overflow
    ob, of = poisoned((rows * cols + 8,), BF16, DEV), poisoned((rows * cols + 8,), F32, DEV)
    ops.to_bf16(dense, out=ob[4:4 + rows * cols].view(rows, cols))
    ops.to_f32(ob[4:4 + rows * cols].view(rows, cols), out=of[4:4 + rows * cols].view(rows, cols))
    sync()
    assert torch.equal(ob[4:-4].view(rows, cols), dense.to(BF16)) and torch.equal(of[4:-4].view(rows, cols), dense.to(BF16).float())
    assert_untouched(ob[:4]), assert_untouched(ob[-4:]), assert_untouched(of[:4]), assert_untouched(of[-4:])
    x = dense.clone()
    ops.scale_(x.view(-1)[4:-4], -0.3)
    sync()
    assert torch.equal(x.view(-1)[4:-4], dense.view(-1)[4:-4] * torch.tensor(-0.3, device=DEV)) and \
        torch.equal(x.view(-1)[:4], dense.view(-1)[:4]) and torch.equal(x.view(-1)[-4:], dense.view(-1)[-4:])


@pytest.mark.parametrize("n", [5, WRAP_ROWS])
def test_row_gathers_and_scatters(n, monkeypatch):
    S = 50
    src = dev(fb.rnd(S, 64 + 12, seed=51))[:, 4:68]                         # f32, strided rows
    srcb = dev(fb.rnd(S, 128 + 8, seed=52).to(BF16))[:, 8:136]
    rows = _ids(n, S, 5)
    inv = rows.clone()
    inv[1::3] = -1
    dsrc, dsrcb = src.contiguous(), srcb.contiguous()
    with poisoned_allocations(monkeypatch):
        g_bf = ops.gather_rows_bf16(src, rows)
        g32 = ops.gather_rows_f32(src, rows)
        g16f, g16b = ops.gather_rows(src, rows), ops.gather_rows(srcb, rows)
        ex_f, ex_b = ops.expand_rows(dsrc, inv, n), ops.expand_rows(dsrcb, inv, n)
    sync()
    pick = src[rows.long()]
    assert torch.equal(g_bf, pick.to(BF16)) and torch.equal(g32, pick) and torch.equal(g16f, pick)
    assert torch.equal(g16b, srcb[rows.long()])
    live = (inv >= 0)[:, None]
    assert torch.equal(ex_f, torch.where(live, dsrc[inv.clamp_min(0).long()], torch.zeros((), device=DEV)))
    assert torch.equal(ex_b, torch.where(live, dsrcb[inv.clamp_min(0).long()], torch.zeros((), dtype=BF16, device=DEV)))
    # scatter: unique destination rows, out of order, into a strided window; then accumulate twice
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(6)).int()
    permd = dev(perm)
    vals = dev(fb.rnd(n, 64, seed=53))
    buf = poisoned((n + 2, 64 + 16), F32, DEV)
    rs, cs = slice(1, n + 1), slice(8, 72)
    ops.scatter_rows(vals, permd, buf[rs, cs])
    sync()
    want = torch.empty_like(vals)
    want[permd.long()] = vals
    assert torch.equal(buf[rs, cs], want)
    ops.scatter_rows(vals, permd, buf[rs, cs], accumulate=True)
    ops.scatter_rows(vals, permd, buf[rs, cs], accumulate=True)
    sync()
    assert torch.equal(buf[rs, cs], want + want + want)
    assert_frame_untouched(buf, rs, cs, "scatter_rows")
    # embedding gather into a window, with and without destination rows
    table = dev(fb.rnd(S, 128, seed=54).to(BF16))
    ids = rows.long()
    ebuf = poisoned((n + 2, 128 + 16), F32, DEV)
    ecs = slice(8, 136)
    ops.embed_gather(table, ids, ebuf[rs, ecs], permd)
    sync()
    ewant = torch.empty(n, 128, device=DEV)
    ewant[permd.long()] = table[ids].float()
    assert torch.equal(ebuf[rs, ecs], ewant)
    assert_frame_untouched(ebuf, rs, ecs, "embed_gather")
    ops.embed_gather(table, ids, ebuf[rs, ecs])
    sync()
    assert torch.equal(ebuf[rs, ecs], table[ids].float())
    assert_frame_untouched(ebuf, rs, ecs, "embed_gather (identity rows)")
    for fn in (lambda: ops.gather_rows(src[:, :62], rows), lambda: ops.expand_rows(dsrc[:, :62].contiguous(), inv, n),
               lambda: ops.gather_rows_f32(src[:, :62], rows), lambda: ops.gather_rows_bf16(src[:, :62], rows),
               lambda: ops.scatter_rows(vals[:, :62].contiguous(), permd, buf[rs, 8:70]),
               lambda: ops.embed_gather(table[:, :124].contiguous(), ids, ebuf[rs, 8:132])):
        with pytest.raises(_lib.MyriadHipError):
            fn()
    sync()
    assert_frame_untouched(buf, rs, cs, "scatter_rows after rejected launches")


@pytest.mark.parametrize("R,C,dt", [(70, 200, F32), (70, 200, BF16), (64, 64, F32), (3, 5, F32), (130, 67, BF16)])
def test_transpose_to_bf16_window_and_padding(R, C, dt):
    x = dev(fb.rnd(R, C + 3, seed=61).to(dt))[:, :C]                        # ld = C + 3: the scalar path where it is odd
    ldo = ops.round_up(R, 64)
    buf = poisoned((C + 2, ldo), BF16, DEV)
    ops.transpose_to_bf16(x, 64, out=buf[1:C + 1])
    sync()
    assert torch.equal(buf[1:C + 1, :R], x.to(BF16).T) and float(buf[1:C + 1, R:].float().abs().max() if ldo > R else 0) == 0
    assert_untouched(buf[0]), assert_untouched(buf[C + 1])
    y = ops.transpose_to_bf16(x.contiguous(), 64)
    assert torch.equal(y, buf[1:C + 1])


def test_kv_append_writes_one_row_of_the_cache():
    """B * cols / 8 items: no batch a decode loop runs (B <= 16 rows of 2 x 4096 columns: 16 384 items) comes near the 2 M items
    of a second grid-stride sweep, so only the single sweep is exercised here."""
    B, T, cols = 3, 6, 256
    src = dev(fb.rnd(B, cols + 8, seed=71).to(BF16))
    cache = poisoned((B, T, cols + 16), BF16, DEV)
    pos = torch.tensor([4], dtype=I32, device=DEV)
    ops.kv_append(src[:, 8:], cache[:, :, 8:8 + cols], pos)
    sync()
    assert torch.equal(cache[:, 4, 8:8 + cols], src[:, 8:])
    assert_frame_untouched(cache, slice(4, 5), slice(8, 8 + cols), "kv_append")
    with pytest.raises(_lib.MyriadHipError):
        ops.kv_append(src[:, 8:8 + 252], cache[:, :, 8:8 + 252], pos)


@pytest.mark.parametrize("B,C,H,W,P", [(2, 3, 28, 42, 14), (1, 1, 8, 8, 4), (3, 3, 1400, 1400, 14)])
def test_patchify_rows_in_conv_weight_order(B, C, H, W, P, monkeypatch):
    img = dev(fb.rnd(B, C, H, W, seed=81))
    with poisoned_allocations(monkeypatch):
        out = ops.patchify(img, P)
    sync()
    K = C * P * P
    want = img.view(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // P) * (W // P), K).to(BF16)
    assert out.shape[1] == ops.round_up(K, 64) and torch.equal(out[:, :K], want)
    assert out.shape[1] == K or float(out[:, K:].float().abs().max()) == 0
    if H > 1000:
        assert out.numel() > fb.EW_WRAP
    with pytest.raises(_lib.MyriadHipError):
        ops.patchify(img[:, :, :H - 1].contiguous(), P)


@pytest.mark.parametrize("R", [1, 5, 70])
def test_decode_records_and_counters(R):
    """decode_record / decode_advance / decode_advance_kept / add_i32_: exact, and nothing next to the records moves."""
    g = torch.Generator().manual_seed(R)
    nxt = dev(torch.randint(0, 32000, (R,), generator=g))
    margin, pmax = dev(fb.rnd(R, seed=1).abs()), dev(fb.rnd(R, seed=2).abs())
    kept = dev(torch.randint(-1, 900, (R,), generator=g).int())
    for kind in ("record", "advance", "kept"):
        nrec = 4 if kind == "kept" else 3
        rec = poisoned((nrec * R + 8,), F32, DEV)
        nid = torch.full((R + 2,), -7, dtype=torch.long, device=DEV)
        cnt = poisoned((2 * R + 6,), I32, DEV)
        step, pos, kv = cnt[1:2], cnt[3:3 + R], cnt[4 + R:4 + 2 * R]
        step.fill_(11), pos.copy_(torch.arange(R, dtype=I32) + 3), kv.copy_(torch.arange(R, dtype=I32) * 2 + 1)
        if kind == "record":
            ops.decode_record(nxt, margin, pmax, rec[4:4 + nrec * R], nid[1:R + 1], step)
        elif kind == "advance":
            ops.decode_advance(nxt, margin, pmax, rec[4:4 + nrec * R], nid[1:R + 1], step, pos, kv)
        else:
            ops.decode_advance_kept(nxt, margin, pmax, kept, rec[4:4 + nrec * R], nid[1:R + 1], step, pos, kv)
        sync()
        want = [nxt.float(), margin, pmax] + ([kept.float()] if kind == "kept" else [])
        assert torch.equal(rec[4:4 + nrec * R], torch.cat(want))
        assert_untouched(rec[:4]), assert_untouched(rec[4 + nrec * R:])
        assert torch.equal(nid[1:R + 1], nxt) and nid[0] == -7 and nid[R + 1] == -7 and int(step) == 12
        adv = 0 if kind == "record" else 1
        assert torch.equal(pos.cpu(), torch.arange(R, dtype=I32) + 3 + adv)
        assert torch.equal(kv.cpu(), torch.arange(R, dtype=I32) * 2 + 1 + adv)
        for part in (cnt[:1], cnt[2:3], cnt[3 + R:4 + R], cnt[4 + 2 * R:]):
            assert_untouched(part, "counters' neighbours")
    c = poisoned((R + 600,), I32, DEV)
    c[3:R + 597] = torch.arange(R + 594, dtype=I32, device=DEV)
    ops.add_i32_(c[3:R + 597], -5)
    sync()
    assert torch.equal(c[3:R + 597].cpu(), torch.arange(R + 594, dtype=I32) - 5)
    assert_untouched(c[:3]), assert_untouched(c[R + 597:])
