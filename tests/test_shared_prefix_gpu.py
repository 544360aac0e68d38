"""Shared-prefix ragged attention: the kernel mh_attn_prefill_ragged_shared bit for bit per segment against
mh_attn_prefill_ragged_past launched for that segment alone on a private copy of its slot, the cache byte for byte unchanged,
independently against fp64, against the _past entry where all slots are distinct, and its argument refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from tests import fp64_bounds as fb  # noqa: E402
from tests.ragged_past_case import GAP, TAIL, cache_frame, past_inputs  # noqa: E402
from tests.shared_prefix_case import (H, N_SLOTS, T_CAP, one_row_shared_inputs, shared_cache_frame,  # noqa: E402
                                      shared_inputs)

DEV = "cuda:0"
BF16, I32 = torch.bfloat16, torch.int32


def _bits(t):
    return t.contiguous().view(torch.int16)


def _launch(D, inputs):
    W, scale = H * D, D ** -0.5
    qkv, prefix, seg, M, pos = inputs
    qkv0 = qkv.clone()
    cos, sin = fb.rope_tables(D, device=DEV)
    o = fb.poisoned((M, W), BF16, DEV)
    cache = shared_cache_frame(D, prefix, seg, DEV)
    cache0 = cache.clone()
    seg_host = torch.tensor(seg, dtype=I32)
    pos_dev = pos.clamp_min(0).to(DEV)
    out = ops.attn_prefill_ragged_shared(qkv, pos_dev, seg_host.to(DEV), seg_host, cache, cos, sin, H, D, scale, out=o)
    torch.cuda.synchronize()
    assert out is o
    return dict(D=D, W=W, scale=scale, qkv=qkv, qkv0=qkv0, prefix=prefix, seg=seg, M=M, pos=pos_dev, cos=cos, sin=sin, o=o,
                cache=cache, cache0=cache0)


@pytest.fixture(scope="module", params=[16, 128])
def shared_case(request):
    """One launch of the kernel per head dim on the poisoned frames, shared by the bit-equality and the fp64 test."""
    return _launch(request.param, shared_inputs(request.param, DEV))


@pytest.fixture(scope="module", params=[16, 128])
def one_row_case(request):
    return _launch(request.param, one_row_shared_inputs(request.param, DEV))


def _check_bits(c):
    D, W, o, cache = c["D"], c["W"], c["o"], c["cache"]
    assert torch.equal(_bits(c["qkv"]), _bits(c["qkv0"]))            # qkv is only read
    assert torch.equal(_bits(cache), _bits(c["cache0"]))             # no cache byte is written
    assert len({s for _, _, s, _ in c["seg"]}) < len(c["seg"])       # slots do repeat
    owned = torch.zeros(c["M"], dtype=torch.bool)
    for r0, n, slot, past in c["seg"]:
        owned[r0:r0 + n] = True
        # the parent's entry for this segment ALONE, on a private copy of its slot that holds the first `past` prefix rows and
        # poison elsewhere; the frame (qkv, pos, row0) is the shared launch's
        own = fb.poisoned((N_SLOTS, T_CAP, 2 * W), BF16, DEV)
        own[slot, :past] = c["prefix"][slot][:past]
        o_ref = fb.poisoned((c["M"], W), BF16, DEV)
        seg_host = torch.tensor([(r0, n, slot, past)], dtype=I32)
        ops.attn_prefill_ragged_past(c["qkv0"], c["pos"], seg_host.to(DEV), seg_host, own, c["cos"], c["sin"], H, D, c["scale"],
                                     out=o_ref)
        assert torch.equal(_bits(o[r0:r0 + n]), _bits(o_ref[r0:r0 + n])), ((D, past, n), "o")
    named = {}
    for _, _, slot, past in c["seg"]:
        named[slot] = max(named.get(slot, 0), past)
    for s in range(N_SLOTS):                                         # poisoned before the launch, still untouched after it
        fb.assert_untouched(cache[s, named.get(s, 0):], f"D={D} cache rows >= past of slot {s}")
    fb.assert_untouched(o[~owned.to(DEV)], f"D={D} gap and padding rows of o")
    assert int((~owned).sum()) == GAP + TAIL


def test_kernel_equals_the_past_entry_per_segment_alone_bit_for_bit(shared_case):
    _check_bits(shared_case)


def test_one_row_segments_on_one_slot_equal_the_past_entry_bit_for_bit(one_row_case):
    _check_bits(one_row_case)


def _heads(t, n, D):
    return t.reshape(1, n, H, D).transpose(1, 2)


def _tok(t):
    return t.transpose(1, 2).reshape(t.shape[2], -1)


def _check_fp64(c):
    """tests/test_ragged_past_gpu.py's _check_fp64 with the segment's keys the first `past` rows of its slot's one prefix; the
    exempt share is a condition: tests/test_answer_scores_cpu.py."""
    D, W = c["D"], c["W"]
    for r0, n, slot, past in c["seg"]:
        pre = c["prefix"][slot][:past]
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
        print(f"D={D} slot={slot} past={past} len={n}: o max err / bound {worst:.3f}")


def test_kernel_is_within_the_fp64_bound_per_segment(shared_case):
    _check_fp64(shared_case)


def test_one_row_segments_on_one_slot_are_within_the_fp64_bound(one_row_case):
    _check_fp64(one_row_case)


@pytest.mark.parametrize("D", [16, 128])
def test_distinct_slots_equal_the_past_entry_bit_for_bit(D):
    W, scale = H * D, D ** -0.5
    qkv, prefixes, seg, M, pos = past_inputs(D, DEV)
    cos, sin = fb.rope_tables(D, device=DEV)
    pos_dev, seg_host = pos.clamp_min(0).to(DEV), torch.tensor(seg, dtype=I32)
    got = []
    for fn in (ops.attn_prefill_ragged_past, ops.attn_prefill_ragged_shared):
        o = fb.poisoned((M, W), BF16, DEV)
        fn(qkv, pos_dev, seg_host.to(DEV), seg_host, cache_frame(D, prefixes, seg, DEV), cos, sin, H, D, scale, out=o)
        got.append(o)
    torch.cuda.synchronize()
    assert not bool(fb.untouched(got[0]).all())                      # the existing entry did run
    assert torch.equal(_bits(got[0]), _bits(got[1]))


def _refusal_frame(D):
    W = H * D
    qkv = (fb.rnd(64, 3 * W + 64, seed=D) * 0.5).to(BF16).to(DEV)
    cos, sin = fb.rope_tables(D, device=DEV)
    pos = torch.arange(64, dtype=I32, device=DEV) % 16
    return qkv, cos, sin, pos, fb.poisoned((64, W), BF16, DEV), fb.poisoned((3, 64, 2 * W), BF16, DEV)


@pytest.mark.parametrize("D,seg,code", [
    (16, [(0, 10, 0, -1)], "MH_ERR_ARG"),                            # past < 0
    (16, [(0, 10, 0, 55)], "MH_ERR_ARG"),                            # past + len = T_cap + 1
    (16, [(0, 10, 0, 3), (9, 10, 1, 3)], "MH_ERR_ARG"),              # overlapping rows
    (16, [(0, 10, 0)], "must be a contiguous"),                      # a [R, 3] table
    (88, [(0, 10, 0, 3)], "MH_ERR_UNSUPPORTED"),
])
def test_bad_arguments_are_refused_before_any_launch(D, seg, code):
    qkv, cos, sin, pos, o, cache = _refusal_frame(D)
    seg_host = torch.tensor(seg, dtype=I32)
    with pytest.raises(_lib.MyriadHipError, match=code):
        ops.attn_prefill_ragged_shared(qkv, pos, seg_host.to(DEV), seg_host, cache, cos, sin, H, D, D ** -0.5, out=o)
    torch.cuda.synchronize()
    fb.assert_untouched(o, "o"), fb.assert_untouched(cache, "cache")


def test_a_duplicate_slot_is_accepted():
    """The table tests/test_ragged_past_gpu.py has the _past entry refuse."""
    qkv, cos, sin, pos, o, cache = _refusal_frame(16)
    seg_host = torch.tensor([(0, 10, 1, 3), (10, 10, 1, 0)], dtype=I32)
    ops.attn_prefill_ragged_shared(qkv, pos, seg_host.to(DEV), seg_host, cache, cos, sin, H, 16, 0.25, out=o)
    torch.cuda.synchronize()
    assert not bool(fb.untouched(o[:20]).any()) and bool(fb.untouched(o[20:]).all())
    fb.assert_untouched(cache, "cache")
