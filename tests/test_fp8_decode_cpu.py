"""FP8 weight-only decode, host side: the quantiser of tests/fp8_ref.py against known answers worked out by hand (e4m3fn: sign,
4 exponent bits with bias 7, 3 mantissa bits, exponent 0 subnormal in steps of 2^-9, largest finite 448 = 0x7E, no infinities),
the exact dequantisation of every finite code, and the switch's default."""
import pytest
import torch

from tests import fp8_ref as F


def _code(x: float) -> int:
    """The e4m3fn code of one value through the reference rule with s = 1 (a row [448, x]: amax 448)."""
    q, s = F.quantize_rows(torch.tensor([[448.0, x]], dtype=torch.float32))
    assert float(s[0]) == 1.0
    return int(q[0, 1])


@pytest.mark.parametrize("x,code", [
    (1.0, 0x38), (448.0, 0x7E), (-448.0, 0xFE),
    (2.0 ** -6, 0x08),                       # smallest normal
    (2.0 ** -9, 0x01),                       # smallest subnormal
    (1.0625, 0x38), (1.1875, 0x3A),          # halfway between 1.0 / 1.125 and 1.125 / 1.25: ties to even
    (3 * 2.0 ** -10, 0x02), (2.0 ** -10, 0x00),   # subnormal ties: 1.5 -> 2, 0.5 -> 0 (in units of 2^-9)
    (-0.0, 0x80),
])
def test_known_codes(x, code):
    assert _code(x) == code
    # and torch's own cast agrees where it is defined (the reference only adds the clamp in front of it)
    assert int(torch.tensor([x]).to(torch.float8_e4m3fn).view(torch.uint8)[0]) == code


def test_449_saturates_to_448():
    assert F.to_e4m3fn(torch.tensor([448.0, 449.0, 500.0, -1e6])).tolist() == [0x7E, 0x7E, 0x7E, 0xFE]
    # the clamp matters: torch's cast alone gives NaN (0x7F) from 464 up
    assert int(torch.tensor([500.0]).to(torch.float8_e4m3fn).view(torch.uint8)[0]) & 0x7F == 0x7F


def test_row_whose_amax_over_s_rounds_above_448_saturates_not_nan():
    # find an amax for which fp32 (amax / (amax / 448)) > 448: the clamp must catch it
    found = None
    for i in range(1, 200000):
        a = torch.tensor(1.0 + i * 2.0 ** -23, dtype=torch.float32)
        s = a / 448.0
        if float(a / s) > 448.0:
            found = float(a)
            break
    assert found is not None
    w = torch.tensor([[found, -found, 0.5 * found]], dtype=torch.float32)
    q, s = F.quantize_rows(w)
    assert float(w[0, 0] / s[0]) > 448.0
    assert q.tolist() == [[0x7E, 0xFE, int(F.quantize_rows(torch.tensor([[448.0, 224.0]]))[0][0, 1])]]
    assert not torch.isnan(F.dequantize(q, s)).any()


def test_all_zero_row_gets_scale_one():
    w = torch.zeros(3, 64, dtype=torch.bfloat16)
    w[1, 5] = -3.0
    q, s = F.quantize_rows(w)
    assert torch.equal(s, torch.tensor([1.0, float(torch.tensor(3.0) / 448.0), 1.0]))
    assert int(q[0].max()) == 0 and int(q[2].max()) == 0
    assert int(q[1, 5]) == 0xFE


def test_every_finite_code_dequantizes_exactly():
    codes = F.FINITE_CODES
    assert codes.numel() == 254
    vals = F.decode_codes(codes)
    hand = torch.tensor([F.e4m3_value(int(c)) for c in codes], dtype=torch.float64)
    assert torch.equal(vals.double(), hand)
    # ... exactly bf16 (what the kernel widens to), and scaled by a power of two exactly
    assert torch.equal(vals.to(torch.bfloat16).float(), vals)
    for s in (1.0, 2.0 ** -12, 2.0 ** 7):
        assert torch.equal(F.dequantize(codes[None], torch.full((1,), s))[0].double(), hand * s)
    # and quantising the decoded values with s = 1 gives the codes back
    row = torch.cat([torch.tensor([448.0]), vals])
    q, s = F.quantize_rows(row[None])
    assert float(s[0]) == 1.0 and torch.equal(q[0, 1:], codes)


def test_quantizer_matches_the_torch_expression_on_random_rows():
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(64, 256, generator=g) * torch.logspace(-6, 3, 64)[:, None]).to(torch.bfloat16)
    w[3, 7] = 1000.0                                  # an outlier row
    q, s = F.quantize_rows(w)
    amax = w.float().abs().amax(1)
    ref = (w.float() / (amax / 448.0)[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(q, ref) and torch.equal(s, amax / 448.0)
    # the round trip is within half an e4m3 step: 2^-4 relative for normals, 2^-10 * s absolute below 2^-6 * s
    back = F.dequantize(q, s)
    err = (back - w.float()).abs()
    assert bool((err <= torch.maximum(w.float().abs() * 2.0 ** -4, 2.0 ** -10 * s[:, None])).all())


def test_unpack_order_is_the_packed_stream_order():
    # a synthetic packed buffer whose bytes name their own (row, k): the reader must put each where the kernel reads it
    N, K = 40, 320
    nw = F.packed_nw(N)
    per = (K // 64 + nw - 1) // nw
    nblk = (N + 15) // 16
    data = torch.zeros(nblk * nw * per * 1024, dtype=torch.int64)
    for blk in range(nblk):
        for w in range(nw):
            for t in range(per):
                for lane in range(64):
                    lr, lg = lane & 15, lane >> 4
                    for e in range(16):
                        off = ((blk * nw + w) * per + t) * 1024 + lane * 16 + e
                        data[off] = (blk * 16 + lr) * 100000 + (64 * (w * per + t) + 16 * lg + e)
    u = F.unpack_fp8(data, N, K)
    rows = torch.arange(u.shape[0])[:, None] * 100000
    ks = torch.arange(u.shape[1])[None, :]
    assert torch.equal(u, rows + ks)


def test_switch_defaults_to_off_and_reads_the_variable(monkeypatch):
    from myriad_amd import llama
    monkeypatch.delenv("MYRIAD_DECODE_FP8", raising=False)
    assert llama.decode_fp8_from_env() is False
    monkeypatch.setenv("MYRIAD_DECODE_FP8", "1")
    assert llama.decode_fp8_from_env() is True
    monkeypatch.setenv("MYRIAD_DECODE_FP8", "0")
    assert llama.decode_fp8_from_env() is False
