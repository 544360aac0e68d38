"""The packed weight-streaming product at 17 to 64 rows (mh_gemv_packed_wide / _fp8_wide / _fp4_wide, ops.gemv_packed_wide) on the
MI355X.  Its contract is bit equality with the 16-row kernel on the same packed copy, row by row: every 16-row chunk of `a` through
ops.gemv_packed must give the bits of those rows of ONE wide call, for every weight kind, output type, bias / residual / alpha and
leading dimension.  One case per kind is also held against float64 of the dequantised weights with the fp32-summation bound of
tests/test_fp8_decode_gpu.py and tests/test_fp4_decode_gpu.py, so the comparison does not rest on the sibling kernel alone."""
import pytest
import torch

from myriad_amd import _lib, ops
from tests import fp8_ref as F8
from tests import mxfp4_ref as M4

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
KINDS = ("bf16", "fp8", "fp4")
ROWS = (17, 32, 33, 48, 64)
# (N, K for bf16 / fp8, K for fp4).  The kernel groups 1, 2 or 4 column blocks per workgroup by N / 16 and the weight kind (the
# largest group that leaves 384 workgroups on bf16, 192 on fp8 / fp4), and batches 4 steps with groups of 4, else 2 (fp4: 4):
#   N = 40     a padded last column block, three steps (two for fp4) over 8 waves; groups of 1
#   N = 1000   65 steps (33 for fp4): they do not divide among the 8 waves; groups of 1
#   N = 6160   385 blocks, still 8 waves: groups of 1 on bf16, of 2 on fp8 / fp4, the last group holding one block
#   N = 8208   N / 16 = 513 >= 512: the 4-wave variant, the last block partial; groups of 1 on bf16, of 2 on fp8 / fp4 with the
#              last group holding one block
#   N = 16400  1025 blocks: groups of 2 on bf16, of 4 on fp8 / fp4, the last group holding one block; one step
#   N = 24592  1537 blocks: groups of 4 on every kind, the last one holding one block; 17 steps over 4 waves: a whole 4-step batch,
#              a remainder of one and a last wave clipped at K
SHAPES = ((40, 192, 256), (1000, 4160, 4224), (6160, 256, 256), (8208, 256, 256), (16400, 64, 128), (24592, 1088, 2176))
PACK = dict(bf16=ops.gemv_pack, fp8=ops.gemv_pack_fp8, fp4=ops.gemv_pack_fp4)


def _weights(kind, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * 0.03
    w[::97, ::31] *= 40.0                                           # outliers spread the fp8 row scales and the fp4 block scales
    return w.to(BF16), g


@pytest.fixture(scope="module", params=[(k, s) for k in KINDS for s in SHAPES], ids=lambda p: f"{p[0]}_N{p[1][0]}")
def case(request):
    kind, (N, K8, K4) = request.param
    K = K4 if kind == "fp4" else K8
    w, g = _weights(kind, N, K, N + K)
    pw = PACK[kind](w.to(DEV))
    a_full = (torch.randn(64, K + 64, generator=g) * 0.5).to(BF16).to(DEV)       # a[:, :K]: a leading dimension above K
    return dict(kind=kind, N=N, K=K, pw=pw, w=w, a_full=a_full, bias=(torch.randn(N, generator=g) * 0.1).to(DEV),
                res=torch.randn(64, N, generator=g).to(DEV))


def _chunks(a, pw, res, **kw):
    """`a` through the 16-row kernel, 16 rows at a time (the last chunk shorter)."""
    outs = []
    for i in range(0, a.shape[0], 16):
        r = None if res is None else res[i:i + 16]
        outs.append(ops.gemv_packed(a[i:i + 16], pw, residual=r, **kw))
    return torch.cat(outs)


def test_wide_rows_carry_the_bits_of_the_16_row_kernel(case):
    c = case
    pw, K = c["pw"], c["K"]
    strided = c["a_full"][:, :K]
    assert strided.stride(0) == K + 64
    contig = strided.contiguous()
    for M in ROWS:
        for a in (contig[:M], strided[:M]):
            for out_dtype in (BF16, F32):
                for extra in (False, True):
                    kw = dict(out_dtype=out_dtype)
                    res = None
                    if extra:
                        kw.update(bias=c["bias"], alpha=0.5)
                        res = c["res"][:M]
                    wide = ops.gemv_packed_wide(a, pw, residual=res, **kw)
                    want = _chunks(a, pw, res, **kw)
                    assert wide.shape == (M, c["N"]) and wide.dtype == out_dtype
                    same = torch.equal(wide, want)
                    if not same:
                        bad = (wide != want).nonzero()
                        print(c["kind"], c["N"], K, "M", M, out_dtype, "extra", extra, "first mismatches (row, col):", bad[:8].tolist(),
                              "count", bad.shape[0])
                    assert same, (c["kind"], c["N"], K, M, out_dtype, extra)


@pytest.mark.parametrize("kind", KINDS)
def test_rows_past_m_and_columns_past_n_keep_the_poison(kind):
    for N, K8, K4 in SHAPES[:2] + SHAPES[4:5]:                       # groups of 1; of 2 (bf16) and 4 with a partial last group
        K = K4 if kind == "fp4" else K8
        w, g = _weights(kind, N, K, 5 + N)
        pw = PACK[kind](w.to(DEV))
        for M in (17, 33, 64):
            a = (torch.randn(M, K, generator=g) * 0.5).to(BF16).to(DEV)
            for dt, poison in ((F32, -12345.0), (BF16, -12288.0)):
                buf = torch.full((M + 3, N + 8), poison, dtype=dt, device=DEV)
                out = ops.gemv_packed_wide(a, pw, out=buf[:M, :N])
                torch.cuda.synchronize()
                assert out.data_ptr() == buf.data_ptr()
                assert bool((buf[M:] == poison).all()) and bool((buf[:, N:] == poison).all()), (kind, N, M, dt)
                assert torch.equal(buf[:M, :N], _chunks(a, pw, None, out_dtype=dt)), (kind, N, M, dt)
                assert not bool((buf[:M, :N] == poison).any())


def _dequantised(kind, w):
    if kind == "fp8":
        q, s = F8.quantize_rows(w)
        return F8.decode_codes(q).double() * s.double()[:, None]
    if kind == "fp4":
        return M4.dequantize(*M4.quantize_blocks(w))
    return w.double()


@pytest.mark.parametrize("kind", KINDS)
def test_wide_product_against_float64(kind):
    """f32 out within the fp32-summation bound the 16-row fp8 / fp4 tests state, of float64 alpha * x @ dq(W)^T (+bias)(+residual):
        |err| <= 2^-16 * |alpha| * sum_k |x dq| + 2^-22 * (|bias| + |res|)
    (exact bf16 products, fp32 accumulation); bf16 out within one bf16 ulp of the f32 out.  33 rows: three row tiles, the last
    one holding a single valid row."""
    N, K = 1000, 4224 if kind == "fp4" else 4160
    w, g = _weights(kind, N, K, 91)
    pw = PACK[kind](w.to(DEV))
    wd = _dequantised(kind, w)
    M = 33
    x = (torch.randn(M, K, generator=g) * 0.5).to(BF16)
    bias = torch.randn(N, generator=g) * 0.1
    res = torch.randn(M, N, generator=g)
    xd = x.double()
    prod, bound_prod = xd @ wd.t(), xd.abs() @ wd.abs().t()
    for alpha, extra in ((1.0, False), (0.37, True)):
        ref = alpha * prod + ((bias.double()[None, :] + res.double()) if extra else 0.0)
        tol = 2.0 ** -16 * abs(alpha) * bound_prod + 2.0 ** -22 * ((bias.double().abs()[None, :] + res.double().abs()) if extra else 0.0) + 1e-30
        kw = dict(bias=bias.to(DEV), residual=res.to(DEV)) if extra else {}
        o32 = torch.full((M, N), float("nan"), dtype=F32, device=DEV)
        out32 = ops.gemv_packed_wide(x.to(DEV), pw, out=o32, alpha=alpha, **kw).cpu().double()
        err = (out32 - ref).abs()
        print(kind, "alpha", alpha, "max err / bound", float((err / tol).max()))
        assert bool((err <= tol).all()), (kind, alpha, float((err / tol).max()))
        out16 = ops.gemv_packed_wide(x.to(DEV), pw, out_dtype=BF16, alpha=alpha, **kw).cpu().double()
        assert bool(((out16 - out32).abs() <= F8.bf16_ulp(out32)).all()), (kind, alpha)


@pytest.mark.parametrize("kind", KINDS)
def test_wide_refusals(kind):
    N, K = 40, 256
    w, _ = _weights(kind, N, K, 7)
    pw = PACK[kind](w.to(DEV))
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_packed_wide(torch.zeros(65, K, dtype=BF16, device=DEV), pw)            # M > 64
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_packed_wide(torch.zeros(20, K - 64, dtype=BF16, device=DEV), pw)       # K is not the packed K
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_packed(torch.zeros(17, K, dtype=BF16, device=DEV), pw)                 # the 16-row entry still refuses 17 rows
    # the C ABI itself: M = 65 and a K off the step size are MH_ERR_ARG; M = 0 and N = 0 are MH_OK; none of them writes
    L, st = _lib.load(), ops._s()
    a = torch.zeros(65, K, dtype=BF16, device=DEV)
    o = torch.full((65, N), 7.0, dtype=F32, device=DEV)
    fn = getattr(L, ops._packed_entry("_wide", pw))
    wargs = (pw.data.data_ptr(),) if kind == "bf16" else (pw.data.data_ptr(), pw.scales.data_ptr())
    args = lambda M_, N_, K_: (a.data_ptr(), K, *wargs, o.data_ptr(), N, M_, N_, K_, None, None, 0, 1, 1.0, st)   # noqa: E731
    assert fn(*args(65, N, K)) == -1
    assert fn(*args(20, N, K - 32)) == -1
    assert fn(*args(0, N, K)) == 0 and fn(*args(20, 0, K)) == 0 and fn(*args(-1, N, K)) == 0
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())
    assert fn(*args(20, N, K)) == 0                                                      # and the good call does write
    torch.cuda.synchronize()
    assert bool((o[:20] == 0.0).all()) and bool((o[20:] == 7.0).all())
