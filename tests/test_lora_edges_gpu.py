"""The LoRA kernels (csrc/lora.hip) at their edges against fp64 references (tests/fp64_bounds.py, LoRA section), element by
element: every output and every buffer the wrappers allocate starts poisoned, the split-K workspace is filled with 0xFF before
each fused call, every frame (rows past M, border groups past G, pad columns, the cells of W_ext the refresh does not own) must
keep its poison, and the dropout mask comes from keep_mask_ref -- an integer restatement of the hash -- never from the library.

Shapes: rank 16 (R2 = 32), D on both sides of the launcher's group fall-back (4 -> 2 -> 1 border groups), waves without a k-step,
the UN = 4 tail, M % 16 != 0, empty and ragged row chunks of both weight-gradient kernels, D % 128 != 0, strided operands, the
ROWS = 1..5 instances of the fused dx + norm kernel with ragged last row groups, three and more than three slabs of either type.

The fused entries (mh_gemm_lora_dx, mh_gemm_lora_rmsnorm_bwd) run on a dgrad GEMM made exact -- 24 non-zeros of +-1 / +-2 per dqkv
row against integers in -2..2, so every partial sum is an integer <= 96, exact in bf16 and fp32 slabs -- and a dropped or doubled
slab is wrong by at least 1.  The weight gradients those entries queue are launched from the queued border pointer and stride
with dq / dv operands of their own ([M, D] each): LoraQV._wgrad reads dq and dv out of a [M, 3D] dqkv, and most of the table's K are
shorter than 3D.

Each test prints `RATIO <kernel> <worst err / bound>` (information; the assertion is assert_within's)."""
import contextlib
import functools

import pytest
import torch

from myriad_amd import _lib, ops
from myriad_amd.lora import BORDER, V_TAG, LoraQV, lora_param_specs
from tests import fp64_bounds as fb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
SEED = 0x7A5C3E1F90B2D486                 # 63 bits, high bits set
S = 2.0                                   # alpha / r = 16 / 8
PS = (0.25, 0.0)
OK, ARG, UNSUPPORTED = 0, -1, -3


def _ratio(name, *vals):
    print(f"RATIO {name} {max(vals):.4g}")


@functools.lru_cache(maxsize=8)
def _masks(M, D, p):
    return fb.keep_mask_ref(SEED, M, D, p).to(DEV), fb.keep_mask_ref(SEED, M, D, p, second=True).to(DEV)


def _guarded(vals, ld, dtype, guard=1e4):
    """[M, ld] buffer holding vals in its first columns and +-guard after them (an over-read past the row is decisive)."""
    M, C = vals.shape
    buf = torch.empty(M, ld)
    buf[:, :C] = vals
    buf[:, C:] = guard * torch.where(torch.arange(ld - C) % 2 == 0, 1.0, -1.0)
    return buf.to(dtype).to(DEV)


@contextlib.contextmanager
def _recorded_allocations(monkeypatch):
    """fb.poisoned_allocations, and a list of every tensor torch.empty returned meanwhile."""
    made = []
    with fb.poisoned_allocations(monkeypatch):
        inner = torch.empty
        with monkeypatch.context() as m:
            def rec(*a, **k):
                t = inner(*a, **k)
                made.append(t)
                return t
            m.setattr(torch, "empty", rec)
            yield made


# ---------------------------------------------------------------------------------------------------------------- mask
def test_keep_mask_equals_the_integer_restatement(monkeypatch):
    M, D = 70, 2052
    n = M * D
    for p in (0.25, 0.05):
        with fb.poisoned_allocations(monkeypatch):
            q = ops.dropout_keep_mask(n, p, SEED, DEV)
            v = ops.dropout_keep_mask(n, p, SEED | V_TAG, DEV)
        assert torch.equal(q, fb.keep_mask_ref(SEED, M, D, p).reshape(-1).to(DEV)), f"q draw, p = {p}"
        assert torch.equal(v, fb.keep_mask_ref(SEED, M, D, p, second=True).reshape(-1).to(DEV)), f"v draw, p = {p}"
        assert not torch.equal(q, v)
    with fb.poisoned_allocations(monkeypatch):
        one = ops.dropout_keep_mask(n, 0.0, SEED | V_TAG, DEV)
    assert torch.equal(one, fb.keep_mask_ref(SEED, M, D, 0.0, second=True).reshape(-1).to(DEV)) and bool((one == 1).all())


# ---------------------------------------------------------------------------------------------------------------- lora_down
DOWN_CASES = [(1, 32, 16), (5, 64, 16), (17, 96, 32), (33, 1152, 16), (3, 5120, 16), (16, 2048, 32)]
DOWN_GROUPS = {(1, 32, 16): 1, (5, 64, 16): 2, (17, 96, 32): 1, (33, 1152, 16): 4, (3, 5120, 16): 4, (16, 2048, 32): 2}


@pytest.mark.parametrize("M,D,R2", DOWN_CASES)
def test_lora_down_partials_per_group(M, D, R2):
    lib = _lib.load()
    G = fb.lora_groups(D, R2)
    assert G == DOWN_GROUPS[(M, D, R2)]
    ldx = D + BORDER + 8
    x = fb.lora_rows(M, D, seed=100 + M).to(BF16)
    xbuf = _guarded(x.float(), ldx, BF16)
    before = xbuf.clone()
    A = fb.lora_adaptor(R2, D, seed=200 + D).to(DEV)
    worst = []
    for p in PS:
        kq, kv = _masks(M, D, p)
        out = fb.poisoned((M + 3, BORDER + 8), BF16, DEV)
        rc = lib.mh_lora_down(xbuf.data_ptr(), ldx, A.data_ptr(), out.data_ptr(), out.stride(0), M, D, R2, S, p, SEED, ops._s())
        torch.cuda.synchronize()
        assert rc == OK
        r = fb.lora_down_ref_bound(xbuf[:, :D], A, S, p, kq, kv, R2, G)
        what = f"lora_down {M}x{D} R2={R2} p={p}"
        worst.append(fb.assert_within(out[:M, :G * R2], r["part"], r["part_bound"], what + " partials"))
        worst.append(fb.assert_within(out[:M, :G * R2].double().reshape(M, G, R2).sum(1), r["total"], r["total_bound"], what + " sum of groups"))
        fb.assert_untouched(out[M:], what + " rows past M")
        fb.assert_untouched(out[:M, G * R2:], what + " groups past G and the pad columns")      # the caller zeroes the border once
        assert torch.equal(xbuf, before), what + ": x changed"
    _ratio("lora_down", *worst)


NORM_DOWN_CASES = [(1, 32, 16), (2, 96, 32), (2, 1152, 16), (1, 4096, 16), (2, 2048, 32)]


@pytest.mark.parametrize("M,D,R2", NORM_DOWN_CASES)
def test_rmsnorm_lora_down_in_one_launch(M, D, R2):
    lib = _lib.load()
    G = fb.lora_groups(D, R2)
    ldh, ldx, eps = D + 4, D + BORDER + 8, 1e-6
    h = _guarded(fb.norm_rows(M, D, seed=300 + D), ldh, F32)
    w = fb.norm_weight(D, seed=301).to(DEV)
    A = fb.lora_adaptor(R2, D, seed=302 + D).to(DEV)
    h0 = h.clone()
    xe = fb.poisoned((M + 1, ldx), BF16, DEV)
    rc = lib.mh_rmsnorm_lora_down(h.data_ptr(), ldh, w.data_ptr(), eps, A.data_ptr(), xe.data_ptr(), ldx, M, D, R2, S, ops._s())
    torch.cuda.synchronize()
    assert rc == OK
    what = f"rmsnorm_lora_down {M}x{D} R2={R2}"
    n = fb.rmsnorm_ref_bound(h[:, :D], w, eps)
    r_y = fb.assert_within(xe[:M, :D], n["y"], n["y_bf16_bound"], what + " x_ext")
    ones = torch.ones(M, D, device=DEV)
    r = fb.lora_down_ref_bound(xe[:M, :D], A, S, 0.0, ones, ones, R2, G)          # of the rows the kernel itself wrote
    r_b = fb.assert_within(xe[:M, D:D + G * R2], r["part"], r["part_bound"], what + " border")
    fb.assert_within(xe[:M, D:D + G * R2].double().reshape(M, G, R2).sum(1), r["total"], r["total_bound"], what + " sum of groups")
    fb.assert_untouched(xe[M:], what + " row past M")
    fb.assert_untouched(xe[:M, D + G * R2:], what + " groups past G and the pad columns")
    assert torch.equal(h, h0), what + ": h changed"
    # the two launches it replaces, on the same inputs
    two = fb.poisoned((M + 1, ldx), BF16, DEV)
    hd = h[:, :D].contiguous()
    ops.rmsnorm_fwd(hd, w, eps, out=two[:M, :D])
    assert lib.mh_lora_down(two.data_ptr(), ldx, A.data_ptr(), two[:, D:].data_ptr(), ldx, M, D, R2, S, 0.0, 0, ops._s()) == OK
    torch.cuda.synchronize()
    assert torch.equal(fb.untouched(two), fb.untouched(xe)), what + ": the two forms own different cells"
    own = ~fb.untouched(xe)
    assert torch.equal(xe.view(torch.int16)[own], two.view(torch.int16)[own]), what + ": not the bits of rmsnorm_fwd + lora_down"
    _ratio("rmsnorm_lora_down", r_y, r_b)


# ---------------------------------------------------------------------------------------------------------------- lora_dx
@pytest.mark.parametrize("M,D,R2", [(1, 4, 16), (3, 1028, 16), (600, 64, 32), (70, 2052, 32)])
def test_lora_dx_direct(M, D, R2):
    lib = _lib.load()
    ld = D + BORDER + 4
    ext = _guarded(fb.lora_rows(M, D + R2, seed=400 + M), ld, F32)
    before = ext.clone()
    A = fb.lora_adaptor(R2, D, seed=401 + D).to(DEV)
    worst = []
    for p in PS:
        kq, kv = _masks(M, D, p)
        out = fb.poisoned((M + 1, D), F32, DEV)
        rc = lib.mh_lora_dx(ext.data_ptr(), ld, A.data_ptr(), out.data_ptr(), M, D, R2, S, p, SEED, ops._s())
        torch.cuda.synchronize()
        assert rc == OK
        ref, bnd = fb.lora_dx_ref_bound(ext[:, :D], ext[:, D:D + R2], A, S, p, kq, kv)
        what = f"lora_dx {M}x{D} R2={R2} p={p}"
        worst.append(fb.assert_within(out[:M], ref, bnd, what))
        fb.assert_untouched(out[M:], what + " row past M")
        assert torch.equal(ext, before), what + ": dx_ext changed"
    _ratio("lora_dx", *worst)


# ------------------------------------------------------------------------- the dgrad GEMM + lora_dx (+ norm backward) entries
GEMM_CASES = [  # M, D, K, plan
    (5, 256, 64, (0, 1)),             # decode-row route, dense buffer
    (70, 768, 256, (6, 1)),           # unsplit, three live waves
    (37, 256, 4096, (1, 16)),         # fp32 slabs, more than three, one live wave, ROWS 1
    (514, 256, 4096, (1, 4)),         # fp32, four slabs, ROWS 3 ragged
    (1027, 512, 4096, (1, 4)),        # fp32, ROWS 5 ragged
    (257, 4096, 768, (1, 3)),         # fp32, exactly three slabs, ROWS 2 ragged
    (130, 1024, 4096, (5, 8)),        # bf16 slabs, more than three
    (770, 4096, 2048, (2, 2)),        # bf16, ROWS 4 ragged
    (1027, 4096, 2048, (2, 2)),       # bf16, ROWS 5 ragged
]
R8 = 8


def _int_choice(shape, gen):
    return torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, shape, generator=gen)]


@functools.lru_cache(maxsize=1)
def _gemm_case(M, D, K):
    """Inputs and the fp64 product of one case, on the device (shared by the fused / unfused runs and both p)."""
    gen = torch.Generator().manual_seed(500 + M + D + K)
    dqkv = torch.zeros(M, K)
    idx = torch.rand(M, K, generator=gen).argsort(1)[:, :24]
    dqkv.scatter_(1, idx, _int_choice((M, 24), gen))
    wT = _int_choice((D + BORDER, K), gen) * (torch.rand(D + BORDER, K, generator=gen) < 0.5)
    dqkv, wT = dqkv.to(BF16).to(DEV), wT.to(BF16).to(DEV)
    assert bool(((dqkv != 0).sum(1) == 24).all())
    P = dqkv.double() @ wT.double().T
    mag = float((dqkv.double().abs() @ wT.double().abs().T).max())
    assert mag <= 256, mag                                   # every partial sum is an integer, exact in bf16 and fp32
    x_ext = torch.cat([fb.lora_rows(M, D, seed=501), fb.rnd(M, BORDER, seed=502)], 1).to(BF16).to(DEV)
    return dict(dqkv=dqkv, wT=wT, P=P, x_ext=x_ext, A=fb.lora_adaptor(2 * R8, D, seed=503 + D).to(DEV),
                dq=_guarded(fb.rnd(M, D, seed=504), D + 8, BF16), dv=_guarded(fb.rnd(M, D, seed=505), D + 8, BF16),
                h=fb.norm_rows(M, D, seed=506).to(DEV), w=fb.norm_weight(D, seed=507).to(DEV), dres=fb.rnd(M, D, seed=508).to(DEV))


def _new_lora(D, p, A):
    from myriad_amd.myriad import ParamStore
    st = ParamStore(lora_param_specs(1, D, R8), DEV)
    lora = LoraQV(1, D, R8, 16.0, p, st.p, st.g, DEV)
    assert lora.s == S
    lora._aqv(st.p, 0).copy_(A)
    return lora


def _check_border(lora, c, M, D, splits, what):
    keep = lora._deferred[-1][1][0]
    if splits > 1:
        assert tuple(keep.shape) == (M, BORDER)
        assert torch.equal(keep[:, :2 * R8].double(), c["P"][:, D:D + 2 * R8]), what + ": border_out is not the integer border"
        fb.assert_untouched(keep[:, 2 * R8:], what + " border_out columns past R2")
    else:
        assert tuple(keep.shape) == (M, D + BORDER)
        assert torch.equal(keep.double(), c["P"]), what + ": the dense product is not the integer product"


def _queued_wgrad(lora, c, M, D, p, what):
    """Launch the queued weight gradient from its own (pointer, stride) of the border gradient; dq / dv are [M, D] operands."""
    lib = _lib.load()
    _, g, _, x_ext, p_q, seed_q = lora._deferred.pop()
    assert (p_q, seed_q) == (p, SEED) and not lora._deferred
    dA = fb.poisoned((2 * R8 + 1, D), F32, DEV)
    dBq, dBv = fb.poisoned((D + 1, R8), F32, DEV), fb.poisoned((D + 1, R8), F32, DEV)
    fb.assert_untouched(lora._ws, what + " wgrad scratch before the launch")
    rc = lib.mh_lora_wgrad(x_ext.data_ptr(), x_ext.stride(0), g[1], g[2], c["dq"].data_ptr(), c["dv"].data_ptr(), c["dq"].stride(0),
                           x_ext[:, D:].data_ptr(), x_ext.stride(0), dA.data_ptr(), dBq.data_ptr(), dBv.data_ptr(),
                           lora._ws.data_ptr(), M, D, 2 * R8, S, p, SEED, ops._s())
    torch.cuda.synchronize()
    assert rc == OK
    kq, kv = _masks(M, D, p)
    mfma = D % 128 == 0 and lib.mh_get_option(b"lora_wgrad_mfma") == 1
    ref = fb.lora_wgrad_ref_bound(x_ext[:, :D], kq, kv, c["P"][:, D:D + 2 * R8], x_ext[:, D:], c["dq"][:, :D], c["dv"][:, :D], S, 2 * R8, mfma)
    worst = [fb.assert_within(dA[:R8], ref["dA"][:R8], ref["dA_bound"][:R8], what + " dA_q"),
             fb.assert_within(dA[R8:2 * R8], ref["dA"][R8:], ref["dA_bound"][R8:], what + " dA_v"),
             fb.assert_within(dBq[:D], ref["dBq"], ref["dBq_bound"], what + " dB_q"),
             fb.assert_within(dBv[:D], ref["dBv"], ref["dBv_bound"], what + " dB_v")]
    for t, nm in ((dA[2 * R8:], "dA"), (dBq[D:], "dB_q"), (dBv[D:], "dB_v")):
        fb.assert_untouched(t, what + f" {nm} row past the end")
    return max(worst)


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("M,D,K,plan", GEMM_CASES)
def test_gemm_lora_dx_and_norm_backward_on_an_exact_dgrad(M, D, K, plan, fused, monkeypatch):
    assert ops.gemm_plan(M, D + BORDER, K) == plan
    splits = plan[1]
    ws = ops.ensure_workspace(torch.device(DEV))
    c = _gemm_case(M, D, K)
    P, eps = c["P"], 1e-6
    r_dxn, r_dh, r_dhb, r_wg = [], [], [], []
    with fb.lib_options(lora_norm_fused=fused):
        for p in PS:
            kq, kv = _masks(M, D, p)
            dxn_ref, dxn_bnd = fb.lora_dx_ref_bound(P[:, :D], P[:, D:D + 2 * R8], c["A"], S, p, kq, kv)
            n = fb.rmsnorm_ref_bound(c["h"], c["w"], eps, dy=dxn_ref, dres=c["dres"], dy_err=dxn_bnd)
            what = f"M={M} D={D} K={K} fused={fused} p={p}"
            inputs = [c[k].clone() for k in ("dqkv", "wT", "x_ext", "h", "w", "dres")]
            with _recorded_allocations(monkeypatch) as made:
                lora = _new_lora(D, p, c["A"])
                if fused:                                       # mh_gemm_lora_dx; the option does not reach it
                    ws.fill_(255)
                    dxn = lora.backward_from_dqkv(0, c["dqkv"], c["wT"], c["x_ext"], p, SEED, defer_wgrad=True)
                    torch.cuda.synchronize()
                    r_dxn.append(fb.assert_within(dxn, dxn_ref, dxn_bnd, what + " dxn (mh_gemm_lora_dx)"))
                    _check_border(lora, c, M, D, splits, what + " mh_gemm_lora_dx")
                    r_wg.append(_queued_wgrad(lora, c, M, D, p, what))
                del made[:]
                ws.fill_(255)
                dh, dhb = lora.backward_from_dqkv_norm(0, c["dqkv"], c["wT"], c["x_ext"], p, SEED, c["h"], c["w"], eps, c["dres"],
                                                       defer_wgrad=True)
                torch.cuda.synchronize()
                if not fused:                                   # the two launches go through a [M, D] fp32 buffer: the first allocation
                    dxn = made[0]
                    assert tuple(dxn.shape) == (M, D) and dxn.dtype == F32
                    r_dxn.append(fb.assert_within(dxn, dxn_ref, dxn_bnd, what + " dxn (unfused buffer)"))
                r_dh.append(fb.assert_within(dh, n["dx"], n["dx_bound"], what + " dh"))
                r_dhb.append(fb.assert_within(dhb, n["dx"], n["dx_bf16_bound"], what + " dh bf16"))
                _check_border(lora, c, M, D, splits, what + " mh_gemm_lora_rmsnorm_bwd")
                if fused:
                    lora._deferred.pop()
                else:
                    r_wg.append(_queued_wgrad(lora, c, M, D, p, what))
            for k, t in zip(("dqkv", "wT", "x_ext", "h", "w", "dres"), inputs):
                assert torch.equal(c[k], t), what + f": input {k} changed"
    _ratio("gemm_lora_dx.dxn", *r_dxn)
    _ratio("gemm_lora_rmsnorm_bwd.dh", *r_dh)
    _ratio("gemm_lora_rmsnorm_bwd.dh_bf16", *r_dhb)
    _ratio("gemm_lora.wgrad", *r_wg)


# ---------------------------------------------------------------------------------------------------------------- lora_wgrad
WGRAD_CASES = [(1, 128, 16), (37, 256, 16), (530, 384, 16), (70, 132, 16), (200, 2052, 32), (2100, 64, 32)]


@pytest.mark.parametrize("mfma_opt", [1, 0])
@pytest.mark.parametrize("M,D,R2", WGRAD_CASES)
def test_lora_wgrad_direct(M, D, R2, mfma_opt):
    lib = _lib.load()
    r = R2 // 2
    ldx, ldq, ldg, ldb = D + 8, D + 8, D + BORDER + 4, BORDER + 8
    x = _guarded(fb.lora_rows(M, D, seed=600 + M).to(BF16).float(), ldx, BF16)
    dq, dv = _guarded(fb.rnd(M, D, seed=601), ldq, BF16), _guarded(fb.rnd(M, D, seed=602), ldq, BF16)
    ext = torch.full((M, ldg), 1e4)
    ext[:, D:D + R2] = fb.rnd(M, R2, seed=603) * 0.1
    ext = ext.to(DEV)
    border = _guarded(fb.rnd(M, BORDER, seed=604), ldb, BF16)
    assert bool((border[:, :BORDER] != 0).all())
    inputs = [t.clone() for t in (x, dq, dv, ext, border)]
    # the launcher's own condition for the MFMA kernel, on these operands
    al16 = all(t.data_ptr() % 16 == 0 for t in (x, dq, dv)) and ldx % 8 == 0 and ldq % 8 == 0 and ldg % 2 == 0
    mfma = bool(mfma_opt) and R2 == 16 and D % 128 == 0
    assert al16 or not mfma
    worst = []
    with fb.lib_options(lora_wgrad_mfma=mfma_opt):
        for p in PS:
            kq, kv = _masks(M, D, p)
            dA = fb.poisoned((R2 + 1, D), F32, DEV)
            dBq, dBv = fb.poisoned((D + 1, r), F32, DEV), fb.poisoned((D + 1, r), F32, DEV)
            nws = lib.mh_lora_wgrad_ws_floats(D, R2)
            ws = fb.poisoned((nws + 64,), F32, DEV)
            rc = lib.mh_lora_wgrad(x.data_ptr(), ldx, ext.data_ptr(), ldg, dq.data_ptr(), dv.data_ptr(), ldq, border.data_ptr(), ldb,
                                   dA.data_ptr(), dBq.data_ptr(), dBv.data_ptr(), ws.data_ptr(), M, D, R2, S, p, SEED, ops._s())
            torch.cuda.synchronize()
            assert rc == OK
            ref = fb.lora_wgrad_ref_bound(x[:, :D], kq, kv, ext[:, D:D + R2], border[:, :BORDER], dq[:, :D], dv[:, :D], S, R2, mfma)
            what = f"lora_wgrad {M}x{D} R2={R2} mfma={int(mfma)} p={p}"
            worst += [fb.assert_within(dA[:r], ref["dA"][:r], ref["dA_bound"][:r], what + " dA_q"),
                      fb.assert_within(dA[r:R2], ref["dA"][r:], ref["dA_bound"][r:], what + " dA_v"),
                      fb.assert_within(dBq[:D], ref["dBq"], ref["dBq_bound"], what + " dB_q"),
                      fb.assert_within(dBv[:D], ref["dBv"], ref["dBv_bound"], what + " dB_v")]
            for t, nm in ((dA[R2:], "dA"), (dBq[D:], "dB_q"), (dBv[D:], "dB_v"), (ws[nws:], "scratch")):
                fb.assert_untouched(t, what + f" {nm} past the end")
            for t, t0 in zip((x, dq, dv, ext, border), inputs):
                assert torch.equal(t, t0), what + ": an input changed"
    _ratio("lora_wgrad.mfma" if mfma else "lora_wgrad.thread", *worst)


# ---------------------------------------------------------------------------------------------------------------- refresh
@pytest.mark.parametrize("W,D,r", [(12, 32, 8), (100, 64, 16), (128, 128, 8)])
def test_lora_refresh_border_and_borders(W, D, r):
    lib = _lib.load()
    ld_ext, ld_extT = D + BORDER + 8, 3 * W + 8

    def frames():
        return fb.poisoned((3 * W + 1, ld_ext), BF16, DEV), fb.poisoned((D + BORDER + 1, ld_extT), BF16, DEV)

    Bs = [(fb.rnd(W, r, seed=700 + 2 * i).to(DEV), fb.rnd(W, r, seed=701 + 2 * i).to(DEV)) for i in range(3)]
    for with_T in (True, False):
        ext, extT = frames()
        rc = lib.mh_lora_refresh_border(Bs[0][0].data_ptr(), Bs[0][1].data_ptr(), ext.data_ptr(), ld_ext,
                                        extT.data_ptr() if with_T else None, ld_extT, W, D, r, ops._s())
        torch.cuda.synchronize()
        assert rc == OK
        fb.lora_refresh_check(ext, extT if with_T else None, Bs[0][0], Bs[0][1], W, D, r, f"refresh_border W={W} D={D} r={r}")
        if not with_T:
            fb.assert_untouched(extT, "W_ext^T not given")
    for with_T in (True, False):
        bufs = [frames() for _ in range(3)]
        ptrs = []
        for (bq, bv), (ext, extT) in zip(Bs, bufs):
            ptrs += [bq.data_ptr(), bv.data_ptr(), ext.data_ptr(), extT.data_ptr() if with_T else 0]
        tab = torch.tensor(ptrs, dtype=torch.int64).to(DEV)
        rc = lib.mh_lora_refresh_borders(tab.data_ptr(), 3, ld_ext, ld_extT, W, D, r, ops._s())
        torch.cuda.synchronize()
        assert rc == OK
        for i, ((bq, bv), (ext, extT)) in enumerate(zip(Bs, bufs)):
            fb.lora_refresh_check(ext, extT if with_T else None, bq, bv, W, D, r, f"refresh_borders layer {i} W={W} D={D} r={r}")
            if not with_T:
                fb.assert_untouched(extT, "W_ext^T not given")
        assert torch.equal(tab.cpu(), torch.tensor(ptrs, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_lora_down_refusals():
    lib = _lib.load()
    M, D = 4, 64
    x = _guarded(fb.rnd(M, D, seed=800), D + BORDER + 8, BF16)
    A = fb.lora_adaptor(32, D, seed=801).to(DEV)
    out = fb.poisoned((M + 3, BORDER + 8), BF16, DEV)

    def call(M=M, D=D, ldx=x.stride(0), R2=16, p=0.25):
        rc = lib.mh_lora_down(x.data_ptr(), ldx, A.data_ptr(), out.data_ptr(), out.stride(0), M, D, R2, S, p, SEED, ops._s())
        torch.cuda.synchronize()
        fb.assert_untouched(out, "a refused mh_lora_down")
        return rc

    assert call(D=48) == ARG
    assert call(ldx=D + BORDER + 4) == ARG                     # % 4 == 0 but % 8 != 0
    assert call(p=1.0) == ARG and call(p=-0.25) == ARG
    assert call(R2=0) == ARG
    assert call(R2=24) == UNSUPPORTED
    assert call(M=0) == OK


def test_lora_dx_refusals():
    lib = _lib.load()
    M, D = 3, 64
    ext = _guarded(fb.rnd(M, D + 32, seed=810), D + BORDER + 4, F32)
    A = fb.lora_adaptor(32, D, seed=811).to(DEV)
    out = fb.poisoned((M + 1, D), F32, DEV)

    def call(D=D, ld=ext.stride(0), R2=16, p=0.25):
        rc = lib.mh_lora_dx(ext.data_ptr(), ld, A.data_ptr(), out.data_ptr(), M, D, R2, S, p, SEED, ops._s())
        torch.cuda.synchronize()
        fb.assert_untouched(out, "a refused mh_lora_dx")
        return rc

    assert call(D=62) == ARG
    assert call(ld=D + BORDER + 2) == ARG
    assert call(ld=D + 8) == ARG                                # shorter than D + R2
    assert call(p=1.0) == ARG
    assert call(R2=8) == UNSUPPORTED


def test_lora_wgrad_refusals():
    lib = _lib.load()
    M, D = 5, 64
    x, dq, dv = (_guarded(fb.rnd(M, D, seed=820 + i), D + 8, BF16) for i in range(3))
    ext = _guarded(fb.rnd(M, D + 32, seed=823), D + BORDER + 4, F32)
    border = _guarded(fb.rnd(M, BORDER, seed=824), BORDER + 8, BF16)
    outs = [fb.poisoned((33, D), F32, DEV), fb.poisoned((D + 1, 16), F32, DEV), fb.poisoned((D + 1, 16), F32, DEV)]
    ws = fb.poisoned((lib.mh_lora_wgrad_ws_floats(D, 32),), F32, DEV)

    def call(D=D, ldx=x.stride(0), ldq=dq.stride(0), R2=16, p=0.25):
        rc = lib.mh_lora_wgrad(x.data_ptr(), ldx, ext.data_ptr(), ext.stride(0), dq.data_ptr(), dv.data_ptr(), ldq, border.data_ptr(),
                               border.stride(0), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), ws.data_ptr(), M, D, R2,
                               S, p, SEED, ops._s())
        torch.cuda.synchronize()
        for t in outs + [ws]:
            fb.assert_untouched(t, "a refused mh_lora_wgrad")
        return rc

    assert call(p=1.0) == ARG
    assert call(D=62) == ARG
    assert call(ldx=D + 6) == ARG
    assert call(ldq=D + 6) == ARG
    assert call(R2=24) == UNSUPPORTED


def test_rmsnorm_lora_down_refusals():
    lib = _lib.load()
    D = 64
    big = 8192
    h = _guarded(fb.rnd(3, big, seed=830), big + 4, F32)
    w = fb.norm_weight(big, seed=831).to(DEV)
    A = fb.lora_adaptor(16, big, seed=832).to(DEV)
    xe = fb.poisoned((4, big + BORDER + 8), BF16, DEV)

    def call(M=2, D=D, ldh=h.stride(0), ldx=xe.stride(0), hp=h.data_ptr()):
        rc = lib.mh_rmsnorm_lora_down(hp, ldh, w.data_ptr(), 1e-6, A.data_ptr(), xe.data_ptr(), ldx, M, D, 16, S, ops._s())
        torch.cuda.synchronize()
        fb.assert_untouched(xe, "a refused mh_rmsnorm_lora_down")
        return rc

    assert call(hp=None) == ARG
    assert call(ldx=D + BORDER - 8) == ARG
    assert call(ldh=h.stride(0) + 2) == ARG
    assert call(M=3) == UNSUPPORTED
    assert call(D=big) == UNSUPPORTED


def test_lora_refresh_borders_refusals():
    lib = _lib.load()
    W, D, r = 12, 32, 8
    bq, bv = fb.rnd(W, r, seed=840).to(DEV), fb.rnd(W, r, seed=841).to(DEV)
    ext, extT = fb.poisoned((3 * W, D + BORDER), BF16, DEV), fb.poisoned((D + BORDER, 3 * W), BF16, DEV)
    tab = torch.tensor([bq.data_ptr(), bv.data_ptr(), ext.data_ptr(), extT.data_ptr()], dtype=torch.int64).to(DEV)

    def call(table=tab.data_ptr(), n=1, W=W, r=r):
        rc = lib.mh_lora_refresh_borders(table, n, D + BORDER, 3 * W if W else 8, W, D, r, ops._s())
        torch.cuda.synchronize()
        fb.assert_untouched(ext, "a refused mh_lora_refresh_borders")
        fb.assert_untouched(extT, "a refused mh_lora_refresh_borders")
        return rc

    assert call(table=None) == ARG
    assert call(W=0) == ARG
    assert call(r=0) == ARG
    assert call(n=0) == OK


def test_backward_from_dqkv_refuses_a_k_the_slab_launch_cannot_take(monkeypatch):
    M, D, K = 37, 256, 4104                                     # K % 64 != 0 at a shape the plan splits: no dense buffer is given
    assert ops.gemm_plan(M, D + BORDER, K)[1] > 1
    ops.ensure_workspace(torch.device(DEV))
    dqkv = fb.rnd(M, K, seed=850).to(BF16).to(DEV)
    wT = fb.rnd(D + BORDER, K, seed=851).to(BF16).to(DEV)
    x_ext = fb.rnd(M, D + BORDER, seed=852).to(BF16).to(DEV)
    A = fb.lora_adaptor(2 * R8, D, seed=853).to(DEV)
    with _recorded_allocations(monkeypatch) as made:
        lora = _new_lora(D, 0.25, A)
        with pytest.raises(_lib.MyriadHipError):
            lora.backward_from_dqkv(0, dqkv, wT, x_ext, 0.25, SEED)
        torch.cuda.synchronize()
        assert not lora._deferred
        shapes = [tuple(t.shape) for t in made if t.is_cuda]
        assert (M, D) in shapes and (M, BORDER) in shapes
        for t in made:
            if t.is_cuda and t.dtype in fb.POISON:
                fb.assert_untouched(t, f"refused backward_from_dqkv: allocation {tuple(t.shape)}")
    assert bool((lora.G[lora.names(0)[0]] == 0).all())
