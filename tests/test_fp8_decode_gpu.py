"""FP8 (e4m3fn) weight-only decode on the MI355X: mh_gemv_pack_fp8 against the reference quantiser (bytes and scales bit-equal),
the in-register widening of every finite code, the fp8 GEMV and its fused forms, and LlamaHIP.decode_fp8 against the reference
decode loop of tests/fp8_ref.py (prefill on bf16 weights, every later step on the dequantised copies)."""
import numpy as np
import pytest
import torch

from myriad_amd import _lib, ops
from myriad_amd.llama import LlamaHIP
from tests import fp8_ref as F
from tests import golden_utils as gu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32


def _load_tiny():
    g = np.load(__file__.rsplit("/", 1)[0] + "/golden/llama_tiny.npz")
    return {k: torch.from_numpy(np.asarray(v)) for k, v in g.items()}


def _bf16_all(sd):
    """Every matrix bf16-representable: the HIP model holds them in bf16, so the reference sees the same values."""
    return {k: (v.to(BF16).float() if v.is_floating_point() and v.dim() == 2 else v) for k, v in sd.items()}


def _check_pack(w_dev: torch.Tensor):
    N, K = w_dev.shape
    pw = ops.gemv_pack_fp8(w_dev)
    torch.cuda.synchronize()
    q_ref, s_ref = F.quantize_rows(w_dev.cpu())
    assert pw.data.dtype == torch.uint8 and pw.data.numel() == _lib.load().mh_gemv_pack_fp8_elems(N, K)
    assert torch.equal(pw.scales.cpu(), s_ref), (N, K)
    full = F.unpack_fp8(pw.data.cpu(), N, K)
    assert torch.equal(full[:N, :K], q_ref), (N, K)
    if full.shape[1] > K:
        assert int(full[:, K:].max()) == 0                                           # k past K: zero codes
    assert bool((full[N:] == full[N - 1]).all())                                      # rows past N repeat row N - 1
    return pw, q_ref, s_ref


# --------------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("N,K", [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)])
def test_pack_full_size_shapes_bit_equal(N, K):
    g = torch.Generator().manual_seed(N + K)
    w = (torch.randn(N, K, generator=g) * 0.02).to(BF16).to(DEV)
    _check_pack(w)


def test_pack_odd_rows_outliers_zero_row_and_subnormals():
    N, K = 1000, 640                                   # N not a multiple of 16; a strided source (ldb > K)
    g = torch.Generator().manual_seed(3)
    base = torch.randn(N, K + 64, generator=g) * 0.05
    base[5, 17] = 3000.0                               # one huge outlier: the rest of the row lands in e4m3's subnormals / zero
    base[6] = 0.0                                      # an all-zero row: scale 1, zero codes
    base[7] = torch.randn(K + 64, generator=g) * 1e-5  # after scaling by this row's own amax ...
    base[7, 3] = 1.0                                   # ... every other value sits below 2^-6: subnormal codes
    base[8, 9] = -7.0e-30                              # tiny values in a normal row flush to +-0
    base[9] = -base[9].abs()                           # an all-negative row
    src = base.to(BF16).to(DEV)
    w = src[:, :K]
    assert w.stride(0) == K + 64
    _, q, s = _check_pack(w)
    assert float(s[6]) == 1.0 and int(q[6].max()) == 0
    sub = q[7][(q[7] & 0x7F) != 0]
    assert bool(((sub & 0x78) == 0).any()), "row 7 should carry subnormal codes"


def test_pack_refuses_bad_dims():
    w = torch.zeros(32, 96, dtype=BF16, device=DEV)
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_pack_fp8(w)                          # K % 64 != 0
    pw = ops.gemv_pack_fp8(torch.zeros(32, 128, dtype=BF16, device=DEV))
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_pack_fp8(torch.zeros(32, 64, dtype=BF16, device=DEV), out=pw)


# ------------------------------------------------------------------------------------------------------ exact widening
def test_every_finite_code_reads_back_exactly():
    """One matrix carries all 254 finite codes (every row in its own rotation); with row scales that are powers of two (amax =
    448 * 2^j) q is the code itself, and a one-hot x row reads column k back: out[m, n] = code(n, k) * 2^j exactly."""
    codes = F.FINITE_CODES
    vals = F.decode_codes(codes)                                     # the 254 values, 448 and -448 among them
    N, K = 48, 256
    rows = []
    for n in range(N):
        r = torch.zeros(K)
        r[:254] = torch.roll(vals, 7 * n)
        rows.append(r * 2.0 ** (n % 5 - 2))
    w = torch.stack(rows)
    assert torch.equal(w.to(BF16).float(), w)                       # exact in bf16
    pw, q, s = _check_pack(w.to(BF16).to(DEV))
    assert torch.equal(s, torch.tensor([2.0 ** (n % 5 - 2) for n in range(N)]))
    assert torch.equal(F.decode_codes(q), torch.stack([torch.cat([torch.roll(vals, 7 * n), torch.zeros(2)]) for n in range(N)]))
    want = F.dequantize(q, s)                                        # exact: code * power of two
    for k0 in range(0, K, 16):
        x = torch.zeros(16, K, dtype=BF16, device=DEV)
        x[torch.arange(16), k0 + torch.arange(16)] = 1.0
        out = ops.gemv_packed(x, pw, out_dtype=F32)
        assert torch.equal(out.cpu(), want[:, k0:k0 + 16].t().contiguous()), k0


# ---------------------------------------------------------------------------------------------------------------- GEMV
@pytest.fixture(scope="module", params=[(1000, 11008), (8200, 4352)], ids=["nw8_K11008", "nw4_K4352"])
def packed_case(request):
    N, K = request.param
    g = torch.Generator().manual_seed(N)
    w = torch.randn(N, K, generator=g) * 0.03
    w[::97, ::31] *= 40.0                                           # outliers spread the row scales
    w = w.to(BF16).to(DEV)
    pw = ops.gemv_pack_fp8(w)
    q, s = F.quantize_rows(w.cpu())
    wd = F.decode_codes(q).double() * s.double()[:, None]           # exact float64 q * s
    return dict(N=N, K=K, pw=pw, wd=wd, qabs=F.decode_codes(q).double().abs(), s=s.double(), g=g)


@pytest.mark.parametrize("M", [1, 2, 3, 8, 16])
def test_fp8_gemv_against_float64(packed_case, M):
    """f32 out within the stated fp32-summation bound of float64 alpha * x @ (q*s)^T (+bias)(+residual):
        |err| <= 2^-16 * |alpha| * s_n * sum_k |x q| + 2^-22 * (|bias| + |res|)
    (exact bf16 products; <= 172 steps of fp32 accumulation, the cross-wave sum and the two scalings each lose at most 2^-24 of
    the partial magnitudes); bf16 out within one bf16 ulp of the f32 out."""
    c = packed_case
    N, K, pw = c["N"], c["K"], c["pw"]
    x = (torch.randn(M, K, generator=c["g"]) * 0.5).to(BF16)
    bias = torch.randn(N, generator=c["g"]) * 0.1
    res = torch.randn(M, N, generator=c["g"])
    xd = x.double()
    prod = xd @ c["wd"].t()
    bound_prod = (xd.abs() @ c["qabs"].t()) * c["s"][None, :]
    for alpha in (1.0, 0.37):
        for with_bias, with_res in ((False, False), (True, False), (False, True), (True, True)):
            b = bias.to(DEV) if with_bias else None
            r = res.to(DEV) if with_res else None
            ref = alpha * prod + (bias.double()[None, :] if with_bias else 0.0) + (res.double() if with_res else 0.0)
            tol = 2.0 ** -16 * abs(alpha) * bound_prod + 2.0 ** -22 * ((bias.double().abs()[None, :] if with_bias else 0.0)
                                                                         + (res.double().abs() if with_res else 0.0)) + 1e-30
            out32 = ops.gemv_packed(x.to(DEV), pw, bias=b, residual=r, out_dtype=F32, alpha=alpha).cpu().double()
            err = (out32 - ref).abs()
            assert bool((err <= tol).all()), (M, alpha, with_bias, with_res, float((err / tol).max()))
            out16 = ops.gemv_packed(x.to(DEV), pw, bias=b, residual=r, out_dtype=BF16, alpha=alpha).cpu().double()
            assert bool(((out16 - out32).abs() <= F.bf16_ulp(out32)).all()), (M, alpha, with_bias, with_res)


def test_fp8_gemv_refusals(packed_case):
    c = packed_case
    pw, K = c["pw"], c["K"]
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_packed(torch.zeros(17, K, dtype=BF16, device=DEV), pw)                 # M > 16
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_packed(torch.zeros(2, K - 64, dtype=BF16, device=DEV), pw)             # K mismatch
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_packed_rmsnorm(torch.zeros(2, K + 64, dtype=F32, device=DEV), torch.ones(K + 64, device=DEV), 1e-6, pw)
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_packed_silu(torch.zeros(2, K, dtype=BF16, device=DEV), pw)             # gu must be [M, 2K]
    # the C ABI itself: M > 16 and a missing scale pointer are MH_ERR_ARG
    L = _lib.load()
    a = torch.zeros(17, K, dtype=BF16, device=DEV)
    o = torch.empty(17, pw.N, dtype=F32, device=DEV)
    st = ops._s()
    assert L.mh_gemv_packed_fp8(a.data_ptr(), K, pw.data.data_ptr(), pw.scales.data_ptr(), o.data_ptr(), pw.N, 17, pw.N, K,
                                None, None, 0, 1, 1.0, st) == -1
    assert L.mh_gemv_packed_fp8(a.data_ptr(), K, pw.data.data_ptr(), None, o.data_ptr(), pw.N, 1, pw.N, K,
                                None, None, 0, 1, 1.0, st) == -1


# (8200, 4096): the smallest N on four waves at the production K: 16 steps per wave, one whole batch and no remainder;
# (1000, 256): 4 steps over eight waves, waves 4-7 with an empty range
@pytest.fixture(scope="module", params=[(1000, 4096), (8200, 1024), (8200, 4096), (1000, 256)],
                ids=["nw8", "nw4", "nw4_whole_batch", "nw8_empty_waves"])
def fused_case(request):
    N, K = request.param
    g = torch.Generator().manual_seed(K)
    w = (torch.randn(N, K, generator=g) * 0.03).to(BF16).to(DEV)
    return dict(N=N, K=K, pw=ops.gemv_pack_fp8(w), g=g)


@pytest.mark.parametrize("M", [1, 2])
def test_fp8_fused_forms_bit_identical_to_the_unfused_launches(fused_case, M):
    c = fused_case
    N, K, pw, g = c["N"], c["K"], c["pw"], c["g"]
    h = (torch.randn(M, K, generator=g) * 3.0).to(DEV)
    nw = (1.0 + 0.1 * torch.randn(K, generator=g)).to(DEV)
    res = torch.randn(M, N, generator=g).to(DEV)
    gu_ = (torch.randn(M, 2 * K, generator=g) * 2.0).to(BF16).to(DEV)
    for kw in (dict(), dict(residual=res, out_dtype=F32), dict(out_dtype=F32, alpha=0.5)):
        fused = ops.gemv_packed_rmsnorm(h, nw, 1e-6, pw, **kw)
        assert fused is not None
        two = ops.gemv_packed(ops.rmsnorm_fwd(h, nw, 1e-6), pw, **kw)
        assert torch.equal(fused, two), kw
        fused = ops.gemv_packed_silu(gu_, pw, **kw)
        assert fused is not None
        two = ops.gemv_packed(ops.silu_mul_fwd_blk(gu_), pw, **kw)
        assert torch.equal(fused, two), kw


@pytest.mark.parametrize("M", [1, 2])
def test_fp8_fused_silu_whole_batch_remainder_and_clipped_last_wave(M):
    """The down projection's depth on eight waves: K = 11008 is 172 steps, 22 per wave (one whole batch of 16 and a remainder of
    6) and 18 in the last wave, clipped at K.  Two rows of operand are 44 KiB of LDS."""
    N, K = 48, 11008
    g = torch.Generator().manual_seed(N + K)
    pw = ops.gemv_pack_fp8((torch.randn(N, K, generator=g) * 0.03).to(BF16).to(DEV))
    res = torch.randn(M, N, generator=g).to(DEV)
    gu_ = (torch.randn(M, 2 * K, generator=g) * 2.0).to(BF16).to(DEV)
    act = ops.silu_mul_fwd_blk(gu_)
    for out_dtype in (BF16, F32):
        for residual in (None, res):
            fused = ops.gemv_packed_silu(gu_, pw, residual=residual, out_dtype=out_dtype)
            assert fused is not None
            assert torch.equal(fused, ops.gemv_packed(act, pw, residual=residual, out_dtype=out_dtype)), (out_dtype, residual is None)


def test_fp8_fused_forms_return_none_above_two_rows(fused_case):
    c = fused_case
    K, pw = c["K"], c["pw"]
    assert ops.gemv_packed_rmsnorm(torch.ones(3, K, device=DEV), torch.ones(K, device=DEV), 1e-6, pw) is None
    assert ops.gemv_packed_silu(torch.ones(3, 2 * K, dtype=BF16, device=DEV), pw) is None
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_packed_rmsnorm(torch.ones(17, K, device=DEV), torch.ones(K, device=DEV), 1e-6, pw)


# --------------------------------------------------------------------------------------------------------------- model
def _tiny():
    g = _load_tiny()
    D, layers, heads, inter, V, seed = [int(x) for x in g["meta"]]
    sd = _bf16_all(gu.llama_weights(D, layers, inter, V, seed=seed, std=0.2))
    return g, sd, heads, (D, layers, inter)


def _expected_bytes(lm, kind):
    """Weight bytes of one packed token step, from the shapes: fp8 copies (+ scales) of the decoder matrices, bf16 lm_head."""
    L = _lib.load()
    qkv_key = "wqkv" if lm.lora is None else "wqkv_ext"
    total = 2 * L.mh_gemv_pack_elems(*lm.lm_head.shape)
    for layer in lm.layers:
        for k in (qkv_key, "wo", "wgu", "wd"):
            N, K = layer[k].shape
            fp8 = kind == "fp8" and not (k == "wqkv_ext")
            total += (L.mh_gemv_pack_fp8_elems(N, K) + 4 * N) if fp8 else 2 * L.mh_gemv_pack_elems(N, K)
    return total


def _compare_flat(lm, sd, sd_step, g, heads, lora=None):
    """ids equal the fp8 reference loop's at every step before its first two-ulp near tie, per prompt (single-row batches);
    returns (steps compared, longest run, smallest step-1 |fp8 ref - bf16 ref| logit gap over the tolerance)."""
    emb = g["emb"]
    checked, longest, gap = 0, 0, float("inf")
    for r in range(emb.shape[0]):
        for s0 in (5, 7, 9):
            e = emb[r:r + 1, :s0]
            with torch.no_grad():
                ids_ref, lg8, margins, scales = F.greedy_decode(sd, sd_step, e, heads, 40, lora=lora)
                _, lgb, _, _ = F.greedy_decode(sd, sd, e, heads, 2, lora=lora)
            ids = lm.greedy_generate(e.to(DEV), max_new_tokens=40, stop_ids=())
            assert lm.last_generate_stats["decode_weights"] == "fp8"
            first = F.two_ulp_horizon(margins, scales)
            assert ids.shape[1] >= first, (r, s0, ids.shape, first)
            assert torch.equal(ids[:, :first].cpu(), ids_ref[:, :first]), (r, s0, first, ids[:, :first + 1], ids_ref[:, :first + 1])
            checked += first
            longest = max(longest, first)
            if lgb.shape[1] > 1 and lg8.shape[1] > 1:               # step 1 is the first one on the fp8 weights
                gap = min(gap, float((lg8[:, 1] - lgb[:, 1]).abs().max() / (2.0 * 2.0 ** -7 * scales[:, 1].max())))
    return checked, longest, gap


def test_flat_logit_fp8_decode_ids_equal_the_fp8_reference():
    """The flat llama_tiny fixture (std-0.2 random weights, V = 320).  The reference's margins admit 48 comparable steps (17 on the
    longest run); the floor is asserted so the test cannot pass on a handful.  The fp8 reference's step-1 logits differ from the
    bf16 reference's by 3x the two-ulp tolerance or more, so a token step that silently streamed bf16 would not pass."""
    g, sd, heads, _ = _tiny()
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    lm.decode_fp8 = True
    checked, longest, gap = _compare_flat(lm, sd, F.fp8_state_dict(sd), g, heads)
    assert checked >= 40 and longest >= 12, (checked, longest)
    assert gap > 1.0, gap
    st = lm.last_generate_stats
    assert isinstance(lm._packed["layers"][0]["wo"], ops.PackedFp8Weight)
    assert st["decode_weight_bytes"] == _expected_bytes(lm, "fp8")
    lm.decode_fp8 = False
    lm.greedy_generate(g["emb"][:1, :5].to(DEV), max_new_tokens=4, stop_ids=())
    st16 = lm.last_generate_stats
    assert st16["decode_weights"] == "bf16" and st16["decode_weight_bytes"] == _expected_bytes(lm, "bf16")
    lm_bytes = 2 * _lib.load().mh_gemv_pack_elems(*lm.lm_head.shape)
    scale_bytes = sum(4 * L[k].shape[0] for L in lm.layers for k in ("wqkv", "wo", "wgu", "wd"))
    assert 2 * (st["decode_weight_bytes"] - lm_bytes - scale_bytes) == st16["decode_weight_bytes"] - lm_bytes   # half the matrices


def test_flat_logit_fp8_decode_with_lora_attached():
    """LoRA on q/v: the bordered qkv product stays bf16 (+LoRA), wo / gate|up / down stream fp8."""
    from myriad_amd.lora import PEFT_PREFIX, LoraQV, lora_param_specs
    from myriad_amd.myriad import ParamStore
    g, sd, heads, (D, layers, _) = _tiny()
    r = 8
    gen = torch.Generator().manual_seed(77)
    st = ParamStore(lora_param_specs(layers, D, r), DEV)
    osd = dict(sd)
    for name, ishape, _ in st.specs:
        t = (torch.randn(ishape, generator=gen) * (0.05 if "lora_A" in name else 0.1)).to(BF16).float()
        st.p[name].copy_(t)
        osd[name.replace(PEFT_PREFIX, "llama_model.model.layers.")] = t
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    lm.attach_lora(LoraQV(layers, D, r, 16.0, 0.0, st.p, st.g, DEV))
    lm.decode_fp8 = True
    lora = dict(r=r, alpha=16.0, dropout_mask=None)
    checked, longest, gap = _compare_flat(lm, osd, F.fp8_state_dict(osd, qkv=False), g, heads, lora=lora)
    assert checked >= 30 and longest >= 8, (checked, longest)         # the reference admits 42 (10 on the longest run)
    assert gap > 1.0, gap
    P = lm._packed["layers"][0]
    assert isinstance(P["wqkv"], ops.PackedWeight) and isinstance(P["wd"], ops.PackedFp8Weight)
    assert lm.last_generate_stats["decode_weight_bytes"] == _expected_bytes(lm, "fp8")


def test_beam_search_runs_on_fp8_up_to_16_rows():
    g, sd, heads, _ = _tiny()
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    lm.decode_fp8 = True
    x = g["emb"][:, :7].to(DEV)                                      # 3 items x 4 beams = 12 rows: the packed fp8 step
    kw = dict(max_new_tokens=10, stop_ids=(), eos_id=2, min_length=1, length_penalty=1.0, early_stopping=False,
              num_return_sequences=2, return_scores=True)
    ids, scores = lm.beam_generate(x, 4, **kw)
    st = lm.last_generate_stats
    assert st["decode_weights"] == "fp8" and st["graph_replays"] > 0
    assert ids.shape[0] == 6 and bool(torch.isfinite(torch.as_tensor(scores)).all())
    ids2, scores2 = lm.beam_generate(x, 4, **kw)                     # replayed graph, same answer
    assert torch.equal(ids, ids2)
    # above 16 rows the step is the GEMM path on bf16 weights whatever the switch says
    lm.beam_generate(g["emb"][:, :7].repeat(2, 1, 1).to(DEV), 3, **kw)
    assert lm.last_generate_stats["decode_weights"] == "bf16"


def test_switching_kinds_shares_no_graph_or_workspace():
    """bf16, then fp8, then bf16 again in one model: both bf16 runs give the ids of a fresh model that never switched, and the
    fp8 run those of a fresh fp8 model."""
    g, sd, heads, _ = _tiny()
    x = g["emb"][:2, :9].to(DEV)
    kw = dict(max_new_tokens=24, stop_ids=())
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    lm.decode_fp8 = False
    a = lm.greedy_generate(x, **kw)
    assert lm.last_generate_stats["decode_weights"] == "bf16" and lm.last_generate_stats["graph_replays"] > 0
    lm.decode_fp8 = True
    f = lm.greedy_generate(x, **kw)
    assert lm.last_generate_stats["decode_weights"] == "fp8" and lm.last_generate_stats["graph_replays"] > 0
    lm.decode_fp8 = False
    b = lm.greedy_generate(x, **kw)
    assert lm.last_generate_stats["decode_weights"] == "bf16"
    fresh = LlamaHIP(sd, heads, DEV, need_backward=False)
    fresh.decode_fp8 = False
    fresh = fresh.greedy_generate(x, **kw)
    fresh8 = LlamaHIP(sd, heads, DEV, need_backward=False)
    fresh8.decode_fp8 = True
    f2 = fresh8.greedy_generate(x, **kw)
    assert torch.equal(a, fresh) and torch.equal(b, fresh), (a, b, fresh)
    assert torch.equal(f, f2), (f, f2)
