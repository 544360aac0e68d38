"""Packed prefill on top of a cached prefix: the kernel mh_attn_prefill_ragged_past bit for bit against the three launches of a solo
prefill with `past`, against the existing entry where every past is 0, independently against fp64, and its argument refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from tests import fp64_bounds as fb  # noqa: E402
from tests import ragged_case as rc  # noqa: E402
from tests.ragged_past_case import (FREE_SLOT, GAP, H, ONE_ROW_SLOTS, TAIL, cache_frame, one_row_inputs,  # noqa: E402
                                    past_inputs)

DEV = "cuda:0"
BF16, I32 = torch.bfloat16, torch.int32


def _bits(t):
    return t.contiguous().view(torch.int16)


def _launch(D, inputs):
    W, scale = H * D, D ** -0.5
    qkv, prefixes, seg, M, pos = inputs
    qkv0 = qkv.clone()
    cos, sin = fb.rope_tables(D, device=DEV)
    o = fb.poisoned((M, W), BF16, DEV)
    cache = cache_frame(D, prefixes, seg, DEV)
    seg_host = torch.tensor(seg, dtype=I32)
    pos_dev = pos.clamp_min(0).to(DEV)
    out = ops.attn_prefill_ragged_past(qkv, pos_dev, seg_host.to(DEV), seg_host, cache, cos, sin, H, D, scale, out=o)
    torch.cuda.synchronize()
    assert out is o
    return dict(D=D, W=W, scale=scale, qkv=qkv, qkv0=qkv0, prefixes=prefixes, seg=seg, M=M, pos=pos_dev, cos=cos, sin=sin, o=o,
                cache=cache)


@pytest.fixture(scope="module", params=[16, 128])
def past_case(request):
    """One launch of the kernel per head dim on the poisoned frames, shared by the bit-equality and the fp64 test."""
    return _launch(request.param, past_inputs(request.param, DEV))


@pytest.fixture(scope="module", params=[16, 128])
def one_row_case(request):
    """The same for the one-row segments on long prefixes (ragged_past_case.ONE_ROW_SEGS)."""
    return _launch(request.param, one_row_inputs(request.param, DEV))


def test_kernel_equals_rope_copy_attention_with_past_per_segment_bit_for_bit(past_case):
    _check_bits(past_case, [FREE_SLOT], GAP + TAIL)


def test_one_row_segments_on_long_prefixes_equal_the_three_launches_bit_for_bit(one_row_case):
    """For Sq = 1 the third launch is mh_attn_fwd's decode kernel; the sizes turn every loop of the kernel's copy of it."""
    _check_bits(one_row_case, sorted(set(range(8)) - set(ONE_ROW_SLOTS)), GAP + TAIL)


def _check_bits(c, free_slots, unowned):
    D, W, qkv, o, cache = c["D"], c["W"], c["qkv"], c["o"], c["cache"]
    assert torch.equal(_bits(qkv), _bits(c["qkv0"]))                 # qkv is only read
    owned = torch.zeros(c["M"], dtype=torch.bool)
    for (r0, n, slot, past), pre in zip(c["seg"], c["prefixes"]):
        owned[r0:r0 + n] = True
        # the segment as a B = 1 chunk through the prefill branch of _decode_block, on a clean copy of its slot
        x = c["qkv0"][r0:r0 + n].clone()
        ops.rope_(x, 0, 2 * H, D, c["pos"][r0:r0 + n].contiguous(), c["cos"], c["sin"], 1.0)
        q3 = x.view(1, n, x.shape[1])
        kv = torch.zeros((1, past + n, 2 * W), dtype=BF16, device=DEV)
        kv[0, :past] = pre
        ops.copy3d_bf16(q3[:, :, W:3 * W], kv[:, past:past + n])
        o_ref, _ = ops.attn_fwd(q3[:, :, :W], kv[:, :, :W], kv[:, :, W:], H, D, c["scale"], causal=True, need_lse=False)
        what = (D, past, n)
        assert torch.equal(_bits(o[r0:r0 + n]), _bits(o_ref[0])), (what, "o")
        assert torch.equal(_bits(cache[slot, past:past + n]), _bits(kv[0, past:])), (what, "new cache rows")
        assert torch.equal(_bits(cache[slot, :past]), _bits(pre)), (what, "cache rows < past")
        fb.assert_untouched(cache[slot, past + n:], f"D={D} cache rows >= past + len of slot {slot}")
    fb.assert_untouched(o[~owned.to(DEV)], f"D={D} gap and padding rows of o")
    assert int((~owned).sum()) == unowned
    for s in free_slots:
        fb.assert_untouched(cache[s], f"D={D} the unnamed slot {s}")


@pytest.mark.parametrize("D", [16, 128])
def test_all_past_zero_equals_the_existing_entry_bit_for_bit(D):
    W, scale = H * D, D ** -0.5
    qkv, seg, M, pos = rc.ragged_inputs(D, DEV)
    cos, sin = fb.rope_tables(D, device=DEV)
    pos_dev = pos.clamp_min(0).to(DEV)
    got = []
    for past in (False, True):
        o = fb.poisoned((M, W), BF16, DEV)
        cache = fb.poisoned((rc.N_SLOTS, rc.T_CAP, 2 * W), BF16, DEV)
        seg_host = torch.tensor([s + (0,) for s in seg] if past else seg, dtype=I32)
        fn = ops.attn_prefill_ragged_past if past else ops.attn_prefill_ragged
        fn(qkv, pos_dev, seg_host.to(DEV), seg_host, cache, cos, sin, H, D, scale, out=o)
        got.append((o, cache))
    torch.cuda.synchronize()
    assert not bool(fb.untouched(got[0][0]).all())                   # the existing entry did run
    assert torch.equal(_bits(got[0][0]), _bits(got[1][0])) and torch.equal(_bits(got[0][1]), _bits(got[1][1]))


def _heads(t, n, D):
    return t.reshape(1, n, H, D).transpose(1, 2)


def _tok(t):
    return t.transpose(1, 2).reshape(t.shape[2], -1)


def test_kernel_is_within_the_fp64_bound_per_segment(past_case):
    """Independent of the tiled kernel: fp64 attention (fp64_bounds.attn_ref_bound) of the new queries over K = the cached rows,
    exact, followed by the bf16-rounded fp64 rotation of the new rows with its rounding ambiguities as k_err (q_err likewise).
    The exempt share is a condition: tests/test_ragged_past_cpu.py."""
    _check_fp64(past_case)


def test_one_row_segments_on_long_prefixes_are_within_the_fp64_bound(one_row_case):
    _check_fp64(one_row_case)


def _check_fp64(c):
    D, W = c["D"], c["W"]
    for (r0, n, slot, past), pre in zip(c["seg"], c["prefixes"]):
        x = c["qkv0"][r0:r0 + n].float()
        q, k, v = (_heads(x[:, i * W:(i + 1) * W], n, D) for i in range(3))
        pl = c["pos"][r0:r0 + n].long()[None]
        qr, qe = fb.rope_bf16(q, pl, c["cos"], c["sin"])
        kr, ke = fb.rope_bf16(k, pl, c["cos"], c["sin"])
        kp, vp = _heads(pre[:, :W].double(), past, D), _heads(pre[:, W:].float(), past, D)
        K, Ke = torch.cat([kp, kr], 2), torch.cat([torch.zeros_like(kp), ke], 2)
        r = fb.attn_ref_bound(qr, K, torch.cat([vp, v], 2), c["scale"], fb.attn_mask(1, n, past + n, True, None, DEV), q_err=qe,
                              k_err=Ke)
        worst = fb.assert_within(c["o"][r0:r0 + n], _tok(r["o"]), _tok(r["o_bound"]), f"D={D} past={past} len={n} o")
        fb.assert_within(c["cache"][slot, past:past + n, :W], _tok(kr), _tok(ke), f"D={D} past={past} len={n} cached k")
        assert torch.equal(c["cache"][slot, past:past + n, W:], c["qkv0"][r0:r0 + n, 2 * W:3 * W])
        print(f"D={D} past={past} len={n}: o max err / bound {worst:.3f}")


@pytest.mark.parametrize("D,seg,code", [
    (16, [(0, 10, 0, -1)], "MH_ERR_ARG"),                            # past < 0
    (16, [(0, 10, 0, 55)], "MH_ERR_ARG"),                            # past + len = T_cap + 1
    (16, [(0, 10, 1, 3), (10, 10, 1, 0)], "MH_ERR_ARG"),             # a duplicate slot
    (16, [(0, 10, 0, 3), (9, 10, 1, 3)], "MH_ERR_ARG"),              # overlapping rows
    (16, [(0, 10, 0)], "must be a contiguous"),                      # a [R, 3] table
    (88, [(0, 10, 0, 3)], "MH_ERR_UNSUPPORTED"),
])
def test_bad_arguments_are_refused_before_any_launch(D, seg, code):
    W = H * D
    qkv = (fb.rnd(64, 3 * W + 64, seed=D) * 0.5).to(BF16).to(DEV)
    cos, sin = fb.rope_tables(D, device=DEV)
    pos = torch.arange(64, dtype=I32, device=DEV) % 16
    o = fb.poisoned((64, W), BF16, DEV)
    cache = fb.poisoned((3, 64, 2 * W), BF16, DEV)
    seg_host = torch.tensor(seg, dtype=I32)
    with pytest.raises(_lib.MyriadHipError, match=code):
        ops.attn_prefill_ragged_past(qkv, pos, seg_host.to(DEV), seg_host, cache, cos, sin, H, D, D ** -0.5, out=o)
    torch.cuda.synchronize()
    fb.assert_untouched(o, "o"), fb.assert_untouched(cache, "cache")
