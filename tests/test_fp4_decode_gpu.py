"""MXFP4 weight-only decode on the MI355X: mh_gemv_pack_fp4 against the bit-arithmetic quantiser of tests/mxfp4_ref.py (codes and
scale bytes bit-equal), the in-register widening of every (code, scale byte) pair, the fp4 GEMV and its fused forms, and
LlamaHIP.decode_fp4 against the reference decode loop (prefill on bf16 weights, every later step on the dequantised copies).
The tiny model is llama_tiny's recipe at D = 128 (every K a multiple of 128: 128, and the intermediate size 172 padded to 256)."""
import pytest
import torch

from myriad_amd import _lib, ops
from myriad_amd.llama import DecodeSession, LlamaHIP
from tests import fp8_ref as F8
from tests import golden_utils as gu
from tests import lora_merge_ref as LM
from tests import mxfp4_ref as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32


def _check_pack(w_dev: torch.Tensor):
    N, K = w_dev.shape
    pw = ops.gemv_pack_fp4(w_dev)
    torch.cuda.synchronize()
    c_ref, b_ref = M.quantize_blocks(w_dev.cpu())
    L = _lib.load()
    assert pw.data.dtype == torch.uint8 and pw.data.numel() == L.mh_gemv_pack_fp4_elems(N, K)
    assert pw.scales.dtype == torch.uint8 and pw.scales.numel() == L.mh_gemv_pack_fp4_scale_elems(N, K)
    codes, sb, pad = M.unpack_fp4(pw.data.cpu(), pw.scales.cpu(), N, K)
    assert torch.equal(sb[:N, :K // 32], b_ref), (N, K)
    assert torch.equal(codes[:N, :K], c_ref), (N, K)
    if codes.shape[1] > K:                                                            # steps past K: zero blocks
        assert int(codes[:, K:].max()) == 0 and bool((sb[:, K // 32:] == 2).all())
    assert bool((pad == 2).all())                                                     # and the bytes that pad a scale dword
    assert bool((codes[N:] == codes[N - 1]).all()) and bool((sb[N:] == sb[N - 1]).all())   # rows past N repeat row N - 1
    return pw, c_ref, b_ref


# --------------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("N,K", [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)])
def test_pack_full_size_shapes_bit_equal(N, K):
    g = torch.Generator().manual_seed(N + K)
    w = (torch.randn(N, K, generator=g) * 0.02).to(BF16).to(DEV)
    _check_pack(w)


def test_pack_odd_rows_outliers_zero_blocks_and_subnormals():
    N, K = 1000, 640                                   # N not a multiple of 16; a strided source (ldb > K); 5 steps over 8 waves
    g = torch.Generator().manual_seed(3)
    base = torch.randn(N, K + 64, generator=g) * 0.05
    base[5, 17] = 3000.0                               # an outlier: the rest of its block lands on 0 / 0.5
    base[6] = 0.0                                      # an all-zero row: b = 2, zero codes
    base[7, 64:128] = 0.0                              # zero blocks inside a normal row
    base[7, 70] = -0.0
    base[8] = torch.randn(K + 64, generator=g) * 2.0 ** -129      # subnormal and smallest-normal blocks (the clamp b = 2)
    base[9] = -base[9].abs()                           # an all-negative row
    base[10] = torch.randn(K + 64, generator=g) * 2.0 ** 125      # exponent fields up to 254
    base[10].clamp_(-3.0e38, 3.0e38)
    base[11, ::2] = 2.0 ** -133                        # the smallest subnormal beside ordinary values
    src = base.to(BF16).to(DEV)
    assert bool(torch.isfinite(src.float()).all())
    w = src[:, :K]
    assert w.stride(0) == K + 64
    _, c, b = _check_pack(w)
    assert int(b[6].max()) == 2 and int((c[6] & 7).max()) == 0
    assert b[7, 2:4].tolist() == [2, 2] and int(c[7, 70]) == 8
    assert int(b[8].min()) == 2 and int(b[10].max()) >= 250


def test_pack_refusals_leave_the_outputs_untouched():
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_pack_fp4(torch.zeros(32, 192, dtype=BF16, device=DEV))                # K % 128 != 0
    pw = ops.gemv_pack_fp4(torch.zeros(32, 256, dtype=BF16, device=DEV))
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_pack_fp4(torch.zeros(32, 128, dtype=BF16, device=DEV), out=pw)
    L, st = _lib.load(), ops._s()
    w = torch.ones(32, 320, dtype=BF16, device=DEV)
    q = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device=DEV)
    s = torch.full((1 << 12,), 0x5A, dtype=torch.uint8, device=DEV)
    for N, K, ldb, sp in ((32, 192, 320, s.data_ptr()), (32, 64, 320, s.data_ptr()), (0, 256, 320, s.data_ptr()),
                          (32, 256, 128, s.data_ptr()), (32, 256, 324, s.data_ptr()), (32, 256, 320, None)):
        assert L.mh_gemv_pack_fp4(w.data_ptr(), ldb, N, K, q.data_ptr(), sp, st) == -1, (N, K, ldb)
    torch.cuda.synchronize()
    assert bool((q == 0xA5).all()) and bool((s == 0x5A).all())


# ------------------------------------------------------------------------------------------------------ exact widening
def test_every_code_and_scale_byte_reads_back_exactly():
    """Row n, block j carries the scale byte 2 + (n + 63 j) % 251 -- all of 2..252, and the bytes of neighbouring lanes (rows n,
    n + 1 and blocks j, j + 1) always differ, so a lane / scale mix-up shows -- and all 16 codes twice, rotated by n + j so every
    code meets every nibble and byte_sel.  A block that holds +-6 pins its own scale byte, so the packer must give these codes
    and bytes back; a one-hot x row then reads column k: out[m, n] = code * 2^(b-127) exactly (2 steps per wave: bytes 0 and 1
    of a scale dword)."""
    N, K = 256, 2048
    n_i, j_i = torch.arange(N)[:, None], torch.arange(K // 32)[None, :]
    b_want = (2 + (n_i + 63 * j_i) % 251).to(torch.uint8)
    pos = torch.arange(K)[None, :]
    c_want = ((pos % 32 + n_i + pos // 32) % 16).to(torch.uint8)
    want = M.dequantize(c_want, b_want)                              # float64, exact
    w = want.float()
    assert torch.equal(w.double(), want) and torch.equal(w.to(BF16).float(), w)
    assert set(b_want.flatten().tolist()) == set(range(2, 253))
    pw, c, b = _check_pack(w.to(BF16).to(DEV))
    assert torch.equal(b, b_want) and torch.equal(c, c_want)
    x = torch.zeros(16, K, dtype=BF16, device=DEV)
    out = torch.empty(16, N, dtype=F32, device=DEV)
    idx = torch.arange(16, device=DEV)
    for k0 in range(0, K, 16):
        x[idx, k0 + idx] = 1.0
        out.fill_(float("nan"))
        ops.gemv_packed(x, pw, out=out)
        x[idx, k0 + idx] = 0.0
        assert torch.equal(out.cpu(), w[:, k0:k0 + 16].t().contiguous()), k0


# ---------------------------------------------------------------------------------------------------------------- GEMV
# nw8_K11008 / nw4_K4352: partial batches only (11 and 9 steps per wave, the last wave clipped at K); nw8_K19456: 19 steps per
# wave, one whole 16-step batch and a remainder of 3
@pytest.fixture(scope="module", params=[(1000, 11008), (8200, 4352), (48, 19456)], ids=["nw8_K11008", "nw4_K4352", "nw8_K19456"])
def packed_case(request):
    N, K = request.param
    g = torch.Generator().manual_seed(N)
    w = torch.randn(N, K, generator=g) * 0.03
    w[::97, ::31] *= 40.0                                           # outliers spread the block scales
    w = w.to(BF16).to(DEV)
    pw = ops.gemv_pack_fp4(w)
    wd = M.dequantize(*M.quantize_blocks(w.cpu()))                  # exact float64 dq(W)
    return dict(N=N, K=K, pw=pw, wd=wd, g=g)


@pytest.mark.parametrize("M_", [1, 2, 5, 16])
def test_fp4_gemv_against_float64(packed_case, M_):
    """f32 out within the fp32-summation bound test_fp8_gemv_against_float64 states, of float64 alpha * x @ dq(W)^T (+bias)
    (+residual):   |err| <= 2^-16 * |alpha| * sum_k |x dq| + 2^-22 * (|bias| + |res|)
    (the products are exact here too: bf16 x times a bf16 dq; there is no epilogue scale); bf16 out within one bf16 ulp of the
    f32 out.  Outputs are poisoned with NaN first: an element the kernel leaves out fails the bound."""
    c = packed_case
    N, K, pw = c["N"], c["K"], c["pw"]
    x = (torch.randn(M_, K, generator=c["g"]) * 0.5).to(BF16)
    bias = torch.randn(N, generator=c["g"]) * 0.1
    res = torch.randn(M_, N, generator=c["g"])
    xd = x.double()
    prod = xd @ c["wd"].t()
    bound_prod = xd.abs() @ c["wd"].abs().t()
    o32 = torch.empty(M_, N, dtype=F32, device=DEV)
    o16 = torch.empty(M_, N, dtype=BF16, device=DEV)
    for alpha in (1.0, 0.37):
        for with_bias, with_res in ((False, False), (True, False), (False, True), (True, True)):
            b = bias.to(DEV) if with_bias else None
            r = res.to(DEV) if with_res else None
            ref = alpha * prod + (bias.double()[None, :] if with_bias else 0.0) + (res.double() if with_res else 0.0)
            tol = 2.0 ** -16 * abs(alpha) * bound_prod + 2.0 ** -22 * ((bias.double().abs()[None, :] if with_bias else 0.0)
                                                                         + (res.double().abs() if with_res else 0.0)) + 1e-30
            o32.fill_(float("nan"))
            o16.fill_(float("nan"))
            out32 = ops.gemv_packed(x.to(DEV), pw, out=o32, bias=b, residual=r, alpha=alpha).cpu().double()
            err = (out32 - ref).abs()
            assert bool((err <= tol).all()), (M_, alpha, with_bias, with_res, float((err / tol).max()))
            out16 = ops.gemv_packed(x.to(DEV), pw, out=o16, bias=b, residual=r, alpha=alpha).cpu().double()
            assert bool(((out16 - out32).abs() <= M.bf16_ulp(out32)).all()), (M_, alpha, with_bias, with_res)


def test_fp4_gemv_refusals(packed_case):
    c = packed_case
    pw, K = c["pw"], c["K"]
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_packed(torch.zeros(17, K, dtype=BF16, device=DEV), pw)                 # M > 16
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_packed(torch.zeros(2, K - 128, dtype=BF16, device=DEV), pw)            # K mismatch
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_packed_rmsnorm(torch.zeros(2, K + 128, dtype=F32, device=DEV), torch.ones(K + 128, device=DEV), 1e-6, pw)
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_packed_silu(torch.zeros(2, K, dtype=BF16, device=DEV), pw)             # gu must be [M, 2K]
    # the C ABI itself: M > 16, K % 128 != 0 and a missing scale pointer are MH_ERR_ARG
    L = _lib.load()
    a = torch.zeros(17, K, dtype=BF16, device=DEV)
    o = torch.empty(17, pw.N, dtype=F32, device=DEV)
    st = ops._s()
    args = lambda M_, K_, sp: (a.data_ptr(), K, pw.data.data_ptr(), sp, o.data_ptr(), pw.N, M_, pw.N, K_, None, None, 0, 1, 1.0, st)
    assert L.mh_gemv_packed_fp4(*args(17, K, pw.scales.data_ptr())) == -1
    assert L.mh_gemv_packed_fp4(*args(1, K - 64, pw.scales.data_ptr())) == -1
    assert L.mh_gemv_packed_fp4(*args(1, K, None)) == -1


def test_fp4_four_waves_with_a_whole_batch():
    """N = 8200 runs four waves; K = 8576 is 67 steps: 17 in waves 0-2 (a whole 16-step batch and a remainder of one) and 16 in
    the last wave, a whole batch clipped at K -- deeper than any decoder matrix is on four waves.  The weights are fp4 values
    already (e2m1 magnitudes, a 6 in every block: scale byte 127), so dq(W) = W and the reference needs no host quantiser: the
    16-row kernel within test_fp4_gemv_against_float64's bound of float64 x @ W^T, the fused SiLU form equal to the two launches."""
    N, K = 8200, 8576
    g = torch.Generator().manual_seed(N + K)
    mags = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
    w = mags[torch.randint(0, 8, (N, K), generator=g)] * (1.0 - 2.0 * torch.randint(0, 2, (N, K), generator=g))
    w[:, ::32] = 6.0
    w = w.to(BF16).to(DEV)
    pw = ops.gemv_pack_fp4(w)
    wd = w.double()
    for M_ in (1, 16):
        x = (torch.randn(M_, K, generator=g) * 0.5).to(BF16).to(DEV)
        out = torch.full((M_, N), float("nan"), dtype=F32, device=DEV)
        ops.gemv_packed(x, pw, out=out)
        err = (out.double() - x.double() @ wd.t()).abs()
        tol = 2.0 ** -16 * (x.double().abs() @ wd.abs().t()) + 1e-30
        assert bool((err <= tol).all()), (M_, float((err / tol).max()))
    gu_ = (torch.randn(1, 2 * K, generator=g) * 2.0).to(BF16).to(DEV)
    res = torch.randn(1, N, generator=g).to(DEV)
    for kw in (dict(), dict(residual=res, out_dtype=F32)):
        fused = ops.gemv_packed_silu(gu_, pw, **kw)
        assert fused is not None
        assert torch.equal(fused, ops.gemv_packed(ops.silu_mul_fwd_blk(gu_), pw, **kw)), kw


# (1000, 256): 2 steps over eight waves, waves 2-7 with an empty range
@pytest.fixture(scope="module", params=[(1000, 4096), (8200, 1024), (1000, 256)], ids=["nw8", "nw4", "nw8_empty_waves"])
def fused_case(request):
    N, K = request.param
    g = torch.Generator().manual_seed(K)
    w = (torch.randn(N, K, generator=g) * 0.03).to(BF16).to(DEV)
    return dict(N=N, K=K, pw=ops.gemv_pack_fp4(w), g=g)


@pytest.mark.parametrize("M_", [1, 2])
def test_fp4_fused_forms_bit_identical_to_the_unfused_launches(fused_case, M_):
    c = fused_case
    N, K, pw, g = c["N"], c["K"], c["pw"], c["g"]
    h = (torch.randn(M_, K, generator=g) * 3.0).to(DEV)
    nw = (1.0 + 0.1 * torch.randn(K, generator=g)).to(DEV)
    res = torch.randn(M_, N, generator=g).to(DEV)
    gu_ = (torch.randn(M_, 2 * K, generator=g) * 2.0).to(BF16).to(DEV)
    for kw in (dict(), dict(residual=res, out_dtype=F32), dict(out_dtype=F32, alpha=0.5)):
        fused = ops.gemv_packed_rmsnorm(h, nw, 1e-6, pw, **kw)
        assert fused is not None
        two = ops.gemv_packed(ops.rmsnorm_fwd(h, nw, 1e-6), pw, **kw)
        assert torch.equal(fused, two), kw
        fused = ops.gemv_packed_silu(gu_, pw, **kw)
        assert fused is not None
        two = ops.gemv_packed(ops.silu_mul_fwd_blk(gu_), pw, **kw)
        assert torch.equal(fused, two), kw


def test_fp4_fused_silu_with_a_whole_batch_and_the_lds_budget():
    """K = 19456 at 8 waves: 19 steps per wave, one whole 16-step batch and a remainder of 3, in the fused kernel too (one row:
    38 KiB of LDS).  Two rows pass the 64 KiB budget and the norm form holds at most K = 4096: both return None."""
    N, K = 48, 19456
    g = torch.Generator().manual_seed(K)
    pw = ops.gemv_pack_fp4((torch.randn(N, K, generator=g) * 0.03).to(BF16).to(DEV))
    gu_ = (torch.randn(1, 2 * K, generator=g) * 2.0).to(BF16).to(DEV)
    fused = ops.gemv_packed_silu(gu_, pw, out_dtype=F32)
    assert fused is not None
    assert torch.equal(fused, ops.gemv_packed(ops.silu_mul_fwd_blk(gu_), pw, out_dtype=F32))
    assert ops.gemv_packed_silu(torch.ones(2, 2 * K, dtype=BF16, device=DEV), pw) is None
    assert ops.gemv_packed_rmsnorm(torch.ones(1, K, device=DEV), torch.ones(K, device=DEV), 1e-6, pw) is None


def test_fp4_fused_forms_return_none_above_two_rows(fused_case):
    c = fused_case
    K, pw = c["K"], c["pw"]
    assert ops.gemv_packed_rmsnorm(torch.ones(3, K, device=DEV), torch.ones(K, device=DEV), 1e-6, pw) is None
    assert ops.gemv_packed_silu(torch.ones(3, 2 * K, dtype=BF16, device=DEV), pw) is None
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_packed_rmsnorm(torch.ones(17, K, device=DEV), torch.ones(K, device=DEV), 1e-6, pw)


# --------------------------------------------------------------------------------------------------------------- model
TINY = dict(D=128, layers=2, heads=4, inter=172, V=320, seed=401)


def _tiny():
    """llama_tiny's flat-logit recipe (std-0.2 random weights, V = 320) at D = 128, with its own embeddings [3, 12, 128]."""
    t = TINY
    sd = {k: (v.to(BF16).float() if v.is_floating_point() and v.dim() == 2 else v)
          for k, v in gu.llama_weights(t["D"], t["layers"], t["inter"], t["V"], seed=t["seed"], std=0.2).items()}
    emb = torch.randn(3, 12, t["D"], generator=torch.Generator().manual_seed(t["seed"] + 1)) * 0.5
    return emb, sd, t["heads"]


def _lora_model(seed=77, r=8):
    from myriad_amd.lora import PEFT_PREFIX, LoraQV, lora_param_specs
    from myriad_amd.myriad import ParamStore
    emb, sd, heads = _tiny()
    D, layers = TINY["D"], TINY["layers"]
    gen = torch.Generator().manual_seed(seed)
    st = ParamStore(lora_param_specs(layers, D, r), DEV)
    osd = dict(sd)
    for name, ishape, _ in st.specs:
        t = (torch.randn(ishape, generator=gen) * (0.05 if "lora_A" in name else 0.1)).to(BF16).float()
        st.p[name].copy_(t)
        osd[name.replace(PEFT_PREFIX, "llama_model.model.layers.")] = t
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    lm.attach_lora(LoraQV(layers, D, r, 16.0, 0.0, st.p, st.g, DEV))
    return emb, osd, heads, lm


def _expected_bytes(lm, kind, merged=False):
    """Weight bytes of one packed token step, from the shapes: fp4 codes + scale bytes (fp8 codes + row scales) of the decoder
    matrices, the bordered qkv and lm_head bf16."""
    L = _lib.load()
    total = 2 * L.mh_gemv_pack_elems(*lm.lm_head.shape)
    for layer in lm.layers:
        for k in ("wqkv", "wo", "wgu", "wd"):
            bordered = k == "wqkv" and lm.lora is not None and not merged
            if k == "wqkv" and lm.lora is not None:                   # attach_lora replaces wqkv by [W | B], 64 columns wider
                N, K = layer["wqkv_ext"].shape
                K -= 0 if bordered else 64
            else:
                N, K = layer[k].shape
            if kind == "bf16" or bordered:
                total += 2 * L.mh_gemv_pack_elems(N, K)
            elif kind == "fp8":
                total += L.mh_gemv_pack_fp8_elems(N, K) + 4 * N
            else:
                total += L.mh_gemv_pack_fp4_elems(N, K) + L.mh_gemv_pack_fp4_scale_elems(N, K)
    return total


def _compare_flat(lm, emb, sd, sd_step, sd_bf16_step, sd_fp8_step, heads, lora=None):
    """ids equal the fp4 reference loop's at every step before its first two-ulp near tie, per prompt (single-row batches);
    returns (steps compared, longest run, smallest step-1 |fp4 ref - other ref| logit gap over the two-ulp tolerance, against the
    bf16 and the fp8 reference)."""
    checked, longest, gap = 0, 0, float("inf")
    for r in range(emb.shape[0]):
        for s0 in (5, 7, 9):
            e = emb[r:r + 1, :s0]
            with torch.no_grad():
                ids_ref, lg4, margins, scales = M.greedy_decode(sd, sd_step, e, heads, 40, lora=lora)
                others = [M.greedy_decode(sd, o, e, heads, 2, lora=lora)[1] for o in (sd_bf16_step, sd_fp8_step)]
            ids = lm.greedy_generate(e.to(DEV), max_new_tokens=40, stop_ids=())
            assert lm.last_generate_stats["decode_weights"] == "fp4"
            first = M.two_ulp_horizon(margins, scales)
            assert ids.shape[1] >= first, (r, s0, ids.shape, first)
            assert torch.equal(ids[:, :first].cpu(), ids_ref[:, :first]), (r, s0, first, ids[:, :first + 1], ids_ref[:, :first + 1])
            checked += first
            longest = max(longest, first)
            for lo in others:                                        # step 1 is the first one on the fp4 weights
                gap = min(gap, float((lg4[:, 1] - lo[:, 1]).abs().max() / (2.0 * 2.0 ** -7 * scales[:, 1].max())))
    return checked, longest, gap


def test_flat_logit_fp4_decode_ids_equal_the_fp4_reference():
    """The reference's margins admit 97 comparable steps (40 on the longest run); floors are asserted so the test cannot pass on a
    handful.  The fp4 reference's step-1 logits differ from the bf16 and from the fp8 reference's by at least 13x the two-ulp
    tolerance on this fixture (3x is asserted), so a token step that silently streamed another kind would not pass."""
    emb, sd, heads = _tiny()
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    lm.decode_fp4 = True
    checked, longest, gap = _compare_flat(lm, emb, sd, M.fp4_state_dict(sd), sd, F8.fp8_state_dict(sd), heads)
    assert checked >= 80 and longest >= 30, (checked, longest)
    assert gap >= 3.0, gap
    st = lm.last_generate_stats
    assert all(isinstance(P[k], ops.PackedFp4Weight) for P in lm._packed["layers"] for k in ("wqkv", "wo", "wgu", "wd"))
    assert isinstance(lm._packed["lm_head"], ops.PackedWeight)
    assert st["decode_weight_bytes"] == _expected_bytes(lm, "fp4")
    lm.decode_fp4 = False
    lm.greedy_generate(emb[:1, :5].to(DEV), max_new_tokens=4, stop_ids=())
    st16 = lm.last_generate_stats
    assert st16["decode_weights"] == "bf16" and st16["decode_weight_bytes"] == _expected_bytes(lm, "bf16")
    assert st["decode_weight_bytes"] < st16["decode_weight_bytes"]


def test_flat_logit_fp4_decode_with_lora_bordered():
    """LoRA on q/v, bordered: the qkv product stays bf16 (+LoRA), wo / gate|up / down stream fp4.  The reference admits 49 steps
    (8 on the longest run)."""
    emb, osd, heads, lm = _lora_model()
    lm.decode_fp4 = True
    lora = dict(r=8, alpha=16.0, dropout_mask=None)
    checked, longest, gap = _compare_flat(lm, emb, osd, M.fp4_state_dict(osd, qkv=False), osd, F8.fp8_state_dict(osd, qkv=False),
                                          heads, lora=lora)
    assert checked >= 40 and longest >= 6, (checked, longest)
    assert gap >= 3.0, gap
    P = lm._packed["layers"][0]
    assert isinstance(P["wqkv"], ops.PackedWeight) and isinstance(P["wd"], ops.PackedFp4Weight)
    st = lm.last_generate_stats
    assert st["lora_merged"] is False and st["decode_weight_bytes"] == _expected_bytes(lm, "fp4")


def test_flat_logit_fp4_decode_with_lora_merged():
    """LoRA merged into the step's qkv copy: gemv_pack_fp4 of the row-major merge.  The reference (exact LoRA in the prefill, the
    fp4 round trip of the merged rows in every later step) admits 100 steps (21 on the longest run)."""
    emb, osd, heads, lm = _lora_model()
    lm.decode_fp4 = lm.decode_merge_lora = True
    lora = dict(r=8, alpha=16.0, dropout_mask=None)
    merged = LM.merged_step_state_dict(osd, TINY["layers"], 2.0)
    checked, longest, gap = _compare_flat(lm, emb, osd, M.fp4_state_dict(merged), merged, F8.fp8_state_dict(merged), heads, lora=lora)
    assert checked >= 80 and longest >= 16, (checked, longest)
    assert gap >= 3.0, gap
    st = lm.last_generate_stats
    assert st["lora_merged"] is True and st["lora_merges"] == 9        # no version given: re-merged at every call
    for P in lm._packed["layers"]:
        assert isinstance(P["wqkv"], ops.PackedFp4Weight) and (P["wqkv"].N, P["wqkv"].K) == (3 * TINY["D"], TINY["D"])
    assert st["decode_weight_bytes"] == _expected_bytes(lm, "fp4", merged=True) < _expected_bytes(lm, "fp4", merged=False)
    # the merged copy is the packer's output on ops.lora_merge's rows, bit for bit
    for i, L in enumerate(lm.layers):
        ref = ops.gemv_pack_fp4(lm.lora.merge_layer(i, L, "rows"))
        assert torch.equal(ref.data, lm._packed["layers"][i]["wqkv"].data)
        assert torch.equal(ref.scales, lm._packed["layers"][i]["wqkv"].scales)


def test_both_kinds_on_and_an_unpackable_matrix_raise():
    emb, sd, heads = _tiny()
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    lm.decode_fp4 = lm.decode_fp8 = True
    with pytest.raises(ValueError, match="decode_fp8.*decode_fp4"):
        lm.greedy_generate(emb[:1, :5].to(DEV), max_new_tokens=4, stop_ids=())
    with pytest.raises(ValueError, match="decode_fp8.*decode_fp4"):
        DecodeSession(lm, 64).generate(emb[:1, :5].to(DEV), [[("x", p) for p in range(5)]], weights_version=0, max_new_tokens=4,
                                       stop_ids=(), eos_id=2, min_length=1)
    # llama_tiny itself has D = 64: the packer does not take K = 64, and the model says which matrix
    small = {k: (v.to(BF16).float() if v.is_floating_point() and v.dim() == 2 else v)
             for k, v in gu.llama_weights(64, 2, 172, 320, seed=401, std=0.2).items()}
    lm64 = LlamaHIP(small, 4, DEV, need_backward=False)
    lm64.decode_fp4 = True
    with pytest.raises(_lib.MyriadHipError, match=r"layer 0 wo has K = 64"):
        lm64.greedy_generate(torch.randn(1, 5, 64).to(DEV), max_new_tokens=4, stop_ids=())
    lm64.decode_fp4 = False                                          # and nothing half-built is left behind
    lm64.greedy_generate(torch.randn(1, 5, 64).to(DEV), max_new_tokens=4, stop_ids=())
    assert lm64.last_generate_stats["decode_weights"] == "bf16"


def test_beam_search_sampling_and_penalty_run_on_fp4():
    emb, sd, heads = _tiny()
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    lm.decode_fp4 = True
    x = emb[:, :7].to(DEV)                                           # 3 items x 4 beams = 12 rows: the packed fp4 step
    kw = dict(max_new_tokens=10, stop_ids=(), eos_id=2, min_length=1, length_penalty=1.0, early_stopping=False,
              num_return_sequences=2, return_scores=True)
    ids, scores = lm.beam_generate(x, 4, **kw)
    st = lm.last_generate_stats
    assert st["decode_weights"] == "fp4" and st["graph_replays"] > 0
    assert ids.shape[0] == 6 and bool(torch.isfinite(torch.as_tensor(scores)).all())
    ids2, _ = lm.beam_generate(x, 4, **kw)                           # replayed graph, same answer
    assert torch.equal(ids, ids2)
    # above 16 rows the step is the GEMM path on bf16 weights whatever the switch says
    lm.beam_generate(emb[:, :7].repeat(2, 1, 1).to(DEV), 3, **kw)
    assert lm.last_generate_stats["decode_weights"] == "bf16"
    # the device sampler and the repetition penalty ride the same step
    lm.device_sampling = True
    skw = dict(max_new_tokens=12, stop_ids=(), do_sample=True, top_p=0.9, top_k=50, repetition_penalty=1.3)
    a = lm.greedy_generate(x, generator=torch.Generator().manual_seed(5), **skw)
    st = lm.last_generate_stats
    assert st["decode_weights"] == "fp4" and st.get("device_sampled_rows", 0) > 0
    b = lm.greedy_generate(x, generator=torch.Generator().manual_seed(5), **skw)
    assert torch.equal(a, b)


def test_switching_among_the_three_kinds_shares_no_graph_or_workspace():
    """bf16, fp4, fp8, fp4, bf16 in one model: every run gives the ids of a fresh model of its kind that never switched -- the
    bf16 ones bit for bit after the detour -- and a chat session drops its cache when the kind changes."""
    emb, sd, heads = _tiny()
    x = emb[:2, :9].to(DEV)
    kw = dict(max_new_tokens=24, stop_ids=())

    def set_kind(m, kind):
        m.decode_fp8, m.decode_fp4 = kind == "fp8", kind == "fp4"

    fresh = {}
    for kind in ("bf16", "fp8", "fp4"):
        m = LlamaHIP(sd, heads, DEV, need_backward=False)
        set_kind(m, kind)
        fresh[kind] = m.greedy_generate(x, **kw)
    assert not torch.equal(fresh["fp4"], fresh["bf16"]) and not torch.equal(fresh["fp4"], fresh["fp8"])
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    ids_of = set()
    for kind in ("bf16", "fp4", "fp8", "fp4", "bf16"):
        set_kind(lm, kind)
        got = lm.greedy_generate(x, **kw)
        st = lm.last_generate_stats
        assert st["decode_weights"] == kind and st["graph_replays"] > 0
        assert torch.equal(got, fresh[kind]), kind
        ids_of.add(id(lm._packed))
    assert len(ids_of) == 3 and set(lm._packs) == {"bf16", "fp8", "fp4"}
    assert lm._packs["fp4"]["lm_head"] is lm._packs["bf16"]["lm_head"]              # one lm_head copy for all kinds
    keys = lambda n: [[("x", p) for p in range(n)]]
    skw = dict(max_new_tokens=8, stop_ids=(), eos_id=2, min_length=1)
    sess = DecodeSession(lm, 64)
    set_kind(lm, "fp4")
    sess.generate(emb[:1, :6].to(DEV), keys(6), weights_version=0, **skw)
    sess.generate(emb[:1, :8].to(DEV), keys(8), weights_version=0, **skw)
    assert sess.last_stats["reused_tokens"] > 0
    for kind in ("fp8", "fp4", "bf16"):
        set_kind(lm, kind)
        sess.generate(emb[:1, :10].to(DEV), keys(10), weights_version=0, **skw)
        assert sess.last_stats["reused_tokens"] == 0 and sess.last_stats["full_reprefill_reason"] == "decode weights changed", kind
