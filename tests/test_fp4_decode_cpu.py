"""MXFP4 weight-only decode, host side: the bit-arithmetic quantiser of tests/mxfp4_ref.py against known answers worked out by
hand (e2m1: sign, then {0, 0.5, 1, 1.5, 2, 3, 4, 6}; one scale byte b = max(2, E - 2) per 32 k, X = 2^(b-127)), its error
properties, the stream-order reader, and the built library's host-side entries and the model's switch."""
import re
import types

import pytest
import torch

from myriad_amd import _lib
from tests import mxfp4_ref as M

BF16 = torch.bfloat16


def _block(vals, fill=0.0):
    """A one-row, one-block matrix holding `vals` first, `fill` after."""
    w = torch.full((1, 32), fill, dtype=torch.float32)
    w[0, :len(vals)] = torch.tensor(vals, dtype=torch.float32)
    assert torch.equal(w.to(BF16).float(), w)
    return w


def _q(vals, fill=0.0):
    c, b = M.quantize_blocks(_block(vals, fill))
    return c[0, :len(vals)].tolist(), int(b[0, 0])


# with 4.0 in the block: E = 129, b = 127, X = 1, so the ratio is the value itself
@pytest.mark.parametrize("x,code", [
    (0.0, 0), (0.5, 1), (1.0, 2), (1.5, 3), (2.0, 4), (3.0, 5), (4.0, 6),
    (0.25, 0), (0.75, 2), (1.25, 2), (1.75, 4), (2.5, 4), (3.5, 6),          # ties: to the even code
    (0.2578125, 1), (0.74609375, 1), (1.2578125, 3), (1.7421875, 3), (2.515625, 5), (3.484375, 5),   # one bf16 step off a tie
    (0.2490234375, 0),
])
def test_known_codes_at_scale_one(x, code):
    for sign, bit in ((1.0, 0), (-1.0, 8)):
        codes, b = _q([4.0, sign * x])
        assert b == 127
        assert codes == [6, bit | code], (x, codes)


def test_tie_at_five_and_saturation_between_six_and_eight():
    # the block maximum sets X, so ratios in [4, 8) come only from the maximum's own binade: 5 -> 4 (tie to the even code 6),
    # above 5 -> 6, and everything in (6, 8) saturates at 6
    for x, code in ((4.0, 6), (4.5, 6), (5.0, 6), (5.0625, 7), (5.5, 7), (6.0, 7), (6.5, 7), (7.0, 7), (7.96875, 7)):
        for sign, bit in ((1.0, 0), (-1.0, 8)):
            codes, b = _q([sign * x, 1.0])
            assert b == 127 and codes == [bit | code, 2], (x, codes)
    # 7.96875 = 255/32 is the largest bf16 below 8: dq = 6, error 1.96875 < 2 X
    c, b = M.quantize_blocks(_block([7.96875]))
    assert float(M.dequantize(c, b)[0, 0]) == 6.0


def test_signed_zeros_keep_their_sign():
    codes, b = _q([1.0, 0.0, -0.0, -(2.0 ** -100)])
    assert b == 125 and codes == [6, 0, 8, 8]                     # 1 / 2^-2 = 4 -> code 6; -2^-100 rounds to -0


def test_all_zero_block_has_scale_byte_two():
    codes, b = _q([0.0, -0.0, 0.0])
    assert b == 2 and codes == [0, 8, 0]
    c, bb = M.quantize_blocks(torch.zeros(3, 96))
    assert bb.tolist() == [[2, 2, 2]] * 3 and int(c.max()) == 0


def test_subnormal_maximum_block():
    # bf16 subnormals are m * 2^-133 (m < 128): E = 0, b = 2, X = 2^-125, ratio = m / 256: below 1/2, so the codes are 0 or 1,
    # the tie 64 / 256 = 0.25 going to 0
    sub = lambda m: m * 2.0 ** -133
    codes, b = _q([sub(127), sub(65), sub(64), sub(1), -sub(100)])
    assert b == 2 and codes == [1, 1, 0, 0, 9]
    # the smallest normals share b = 2 up to E = 4: 2^-126 / 2^-125 = 0.5, 2^-123 -> 4
    codes, b = _q([2.0 ** -123, 2.0 ** -126, sub(127)])
    assert b == 2 and codes == [6, 1, 1]
    dq = M.dequantize(*M.quantize_blocks(_block([sub(127), 2.0 ** -126])))
    assert float(dq[0, 0]) == 2.0 ** -126 and float(dq[0, 1]) == 2.0 ** -126      # the smallest non-zero dq: a normal bf16


def test_exponent_field_254_block():
    big = 2.0 ** 127                                                 # exponent field 254
    top = 255 * 2.0 ** 120                                           # the largest finite bf16
    codes, b = _q([big, top, -1.5 * big, 2.0 ** 125, 2.0 ** 124, 1.0])
    assert b == 252                                                  # X = 2^125
    assert codes == [6, 7, 8 | 7, 2, 1, 0]                           # 4, 7.97 -> 6, -6, 1, 0.5, 2^-125 -> 0
    dq = M.dequantize(*M.quantize_blocks(_block([top])))
    assert float(dq[0, 0]) == 6 * 2.0 ** 125 and torch.isfinite(dq.float()).all()


def test_blocks_are_independent_and_32_wide():
    w = torch.zeros(2, 128)
    w[0, 31], w[0, 32], w[1, 64], w[1, 127] = 1.0, 1024.0, -3.0, 0.5
    c, b = M.quantize_blocks(w)
    assert b.tolist() == [[125, 135, 2, 2], [2, 2, 126, 124]]
    assert int(c[0, 31]) == 6 and int(c[0, 32]) == 6 and int(c[1, 64]) == (8 | 7) and int(c[1, 127]) == 6   # -3 / 2^-1 = -6


def _bf16_ok(dq: torch.Tensor) -> bool:
    """Every value is zero or a normal bf16 (exactly representable, magnitude at least 2^-126)."""
    f = dq.float()
    exact = torch.equal(f.double(), dq) and torch.equal(f.to(BF16).float(), f)
    nz = dq[dq != 0].abs()
    return exact and (nz.numel() == 0 or float(nz.min()) >= 2.0 ** -126)


def test_error_bounds_and_normal_dequantised_values():
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(96, 512, generator=g) * torch.logspace(-40, 36, 96, base=10.0)[:, None]).to(BF16)
    w[3, 7] = 1000.0
    w[5, 40:72] = 0.0
    w[9] = (torch.randn(512, generator=g) * 2.0 ** -128).to(BF16)   # subnormal-heavy rows
    w[10] = (torch.randn(512, generator=g) * 2.0 ** -131).to(BF16)
    c, b = M.quantize_blocks(w)
    assert int(b.min()) >= 2 and int(b.max()) <= 252
    dq = M.dequantize(c, b)
    assert _bf16_ok(dq)
    X = M.scale_values(b).repeat_interleave(32, dim=1)
    ratio = w.double().abs() / X
    err = (dq - w.double()).abs()
    idx = (c & 7).long()
    sat = ratio > 6.0
    assert bool(sat.any()) and bool((err[sat] < 2.0 * X[sat]).all())
    assert bool((idx[sat] == 7).all())
    # a non-saturated element: at most half the spacing between the two codes that bracket it
    grid = torch.tensor(M.E2M1, dtype=torch.float64)
    lo = (ratio[..., None] >= grid).sum(-1).clamp(1, 7) - 1          # bracket [grid[lo], grid[lo + 1]]
    half = (grid[lo + 1] - grid[lo]) / 2.0
    ns = ~sat
    assert bool((err[ns] <= half[ns] * X[ns]).all())
    assert bool((((c & 8) != 0) == (w.view(torch.int16) < 0))[:, :].all())          # the sign bit is w's
    # every block's largest element lands on 4 or 6 unless the clamp b = 2 holds it lower
    amax_code = (idx.view(96, 16, 32).max(-1).values)
    assert bool((amax_code[b > 2] >= 6).all())


def test_every_code_and_scale_round_trips():
    # quantising dq values gives the codes back when the block holds a 4 or a 6 (which pin the scale byte)
    for bb in (2, 3, 100, 127, 200, 252):
        X = 2.0 ** (bb - 127)
        vals = [s * v * X for s in (1.0, -1.0) for v in M.E2M1]
        codes, b = _q(vals)
        assert b == bb and codes == list(range(16)), (bb, codes)


def test_unpack_order_is_the_packed_stream_order():
    # synthetic streams whose bytes name their own place: the reader must put each where the header's formula says
    for N, K in ((40, 1280), (16, 128)):                             # per = 2 and per = 1 at nw = 8: a padded scale dword
        nblk, nw, per, per4 = M.packed_dims(N, K)
        data = torch.zeros(nblk * nw * per * 1024, dtype=torch.uint8)
        sc = torch.full((nblk * nw * per4 * 256,), 255, dtype=torch.uint8)
        want_codes = torch.zeros(nblk * 16, nw * per * 128, dtype=torch.uint8)
        want_sc = torch.zeros(nblk * 16, nw * per * 4, dtype=torch.uint8)
        for blk in range(nblk):
            for w in range(nw):
                for t in range(per):
                    for lane in range(64):
                        lr, lg = lane & 15, lane >> 4
                        row, k0 = blk * 16 + lr, 128 * (w * per + t) + 32 * lg
                        for j in range(16):
                            lo_c, hi_c = (row + k0 + 2 * j) % 16, (3 * row + k0 + 2 * j + 1) % 16
                            data[((blk * nw + w) * per + t) * 1024 + lane * 16 + j] = lo_c | (hi_c << 4)
                            want_codes[row, k0 + 2 * j], want_codes[row, k0 + 2 * j + 1] = lo_c, hi_c
                        v = (7 * row + k0 // 32) % 251
                        sc[((blk * nw + w) * per4 + t // 4) * 256 + lane * 4 + t % 4] = v
                        want_sc[row, k0 // 32] = v
        codes, sb, pad = M.unpack_fp4(data, sc, N, K)
        assert torch.equal(codes, want_codes) and torch.equal(sb, want_sc)
        assert pad.numel() == nblk * 16 * nw * 4 * (per4 * 4 - per) and bool((pad == 255).all())


# ------------------------------------------------------------------------------------------------ the built library
def test_pack_elems_values_and_refusals():
    L = _lib.load()
    for N, K in ((12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008), (1000, 640), (17, 128)):
        nblk, nw, per, per4 = M.packed_dims(N, K)
        assert L.mh_gemv_pack_fp4_elems(N, K) == nblk * nw * per * 1024, (N, K)
        assert L.mh_gemv_pack_fp4_scale_elems(N, K) == nblk * nw * per4 * 256, (N, K)
    assert L.mh_gemv_pack_fp4_elems(4096, 4096) == 4096 * 4096 // 2                  # no padding: half a byte per weight
    assert L.mh_gemv_pack_fp4_scale_elems(4096, 4096) == 4096 * 4096 // 32
    for N, K in ((32, 64), (32, 192), (32, 4160), (0, 128), (-1, 128), (32, 0), (32, -128)):
        assert L.mh_gemv_pack_fp4_elems(N, K) == -1, (N, K)
        assert L.mh_gemv_pack_fp4_scale_elems(N, K) == -1, (N, K)


def test_entries_are_exported_and_declared():
    names = ["mh_gemv_pack_fp4_elems", "mh_gemv_pack_fp4_scale_elems", "mh_gemv_pack_fp4", "mh_gemv_packed_fp4",
             "mh_gemv_packed_fp4_rmsnorm", "mh_gemv_packed_fp4_silu"]
    sigs = _lib.signatures()
    L = _lib.load()
    for n in names:
        assert n in sigs, n
        assert getattr(L, n) is not None
    # the fp4 products take the fp8 forms' arguments
    for tail in ("", "_rmsnorm", "_silu"):
        assert sigs["mh_gemv_packed_fp4" + tail] == sigs["mh_gemv_packed_fp8" + tail]
    txt = open(_lib.HEADER_PATH).read()
    rule = txt[txt.index("MXFP4 weight-only copy"):txt.index("long mh_gemv_pack_fp4_elems")]
    for must in ("max(2, E - 2)", "ties to the even code", "lower k in the low nibble", "outside the contract"):
        assert must in re.sub(r"\s*\n \*\s*", " ", rule), must


def test_switch_defaults_to_off_reads_the_variable_and_excludes_fp8(monkeypatch):
    from myriad_amd import llama
    monkeypatch.delenv("MYRIAD_DECODE_FP4", raising=False)
    assert llama.decode_fp4_from_env() is False
    monkeypatch.setenv("MYRIAD_DECODE_FP4", "1")
    assert llama.decode_fp4_from_env() is True
    monkeypatch.setenv("MYRIAD_DECODE_FP4", "0")
    assert llama.decode_fp4_from_env() is False
    kind = llama.LlamaHIP._decode_kind
    assert kind(types.SimpleNamespace(decode_fp8=False, decode_fp4=False)) == "bf16"
    assert kind(types.SimpleNamespace(decode_fp8=True, decode_fp4=False)) == "fp8"
    assert kind(types.SimpleNamespace(decode_fp8=False, decode_fp4=True)) == "fp4"
    with pytest.raises(ValueError, match="decode_fp8.*decode_fp4"):
        kind(types.SimpleNamespace(decode_fp8=True, decode_fp4=True))
