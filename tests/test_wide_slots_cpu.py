"""The wide packed products' C ABI and the slot scheduler at the wide slot counts, without a device: the three entries are declared
and exported with their 16-row counterparts' signatures, the row limits are what the header states, and SlotScheduler +
RefillPlanner replayed at 64 slots over a few hundred synthetic requests admit every request once and finish it."""
import re

import pytest
import torch

from myriad_amd import _lib, ops
from myriad_amd.llama import replay_slot_run

PAIRS = (("mh_gemv_packed_wide", "mh_gemv_packed"), ("mh_gemv_packed_fp8_wide", "mh_gemv_packed_fp8"),
         ("mh_gemv_packed_fp4_wide", "mh_gemv_packed_fp4"))


def test_wide_entries_are_exported_and_declared_with_their_16_row_signatures():
    sigs = _lib.signatures()
    L = _lib.load()
    for wide, narrow in PAIRS:
        assert wide in sigs, wide
        assert getattr(L, wide) is not None
        assert sigs[wide] == sigs[narrow], wide
    txt = re.sub(r"\s*\n \*\s*", " ", open(_lib.HEADER_PATH).read())
    rule = txt[txt.index("The packed products at up to 64 rows"):txt.index("int mh_gemv_packed_wide")]
    for must in ("M > 64 is MH_ERR_ARG", "Bit contract", "fp8 row scale, alpha, bias, residual"):
        assert must in rule, must


def test_row_limits():
    assert ops.GEMV_WIDE_MAX_ROWS == 64 and ops.GEMV_MAX_ROWS == 16


def test_wide_wrapper_refuses_too_many_rows_before_any_launch():
    pw = ops.PackedWeight(torch.empty(0), 32, 64)
    with pytest.raises(_lib.MyriadHipError):
        ops.gemv_packed_wide(torch.zeros(65, 64, dtype=torch.bfloat16), pw)


def _synthetic_run(n, max_new, eos, seed):
    """n requests: prompt lengths 3 .. 23 and generated ids that end where the stop rule ends them (EOS, or max_new ids)."""
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(3, 24, (n,), generator=g).tolist()
    ids = []
    for L in torch.randint(1, max_new + 1, (n,), generator=g).tolist():
        body = torch.randint(10, 1000, (L,), generator=g).tolist()
        if L < max_new:
            body[-1] = eos
        ids.append(body)
    return lengths, ids


@pytest.mark.parametrize("plan", [dict(), dict(prefill_batch=8, refill_min=2), dict(prefill_batch=16, refill_min=2)],
                         ids=["one_request_refill", "pb8_rm2", "pb16_rm2"])
@pytest.mark.parametrize("slots", [17, 32, 64])
def test_scheduler_replay_at_wide_slot_counts(slots, plan):
    n, max_new, eos = 300, 24, 2
    lengths, ids = _synthetic_run(n, max_new, eos, seed=slots)
    st = replay_slot_run(lengths, ids, slots, max_new, (), eos, **plan)
    assert st["prefills"] == n                                          # every request admitted once
    assert st["live_row_steps"] == sum(len(q) - 1 for q in ids)         # and decoded to its end: one live row-step per later id
    assert st["packed_rows"] == sum(lengths)
    assert 0 < st["live_row_steps"] <= st["steps"] * slots
    assert st["occupancy"] == pytest.approx(st["live_row_steps"] / (st["steps"] * slots))
    assert st["prefill_passes"] <= n and (plan == {} or st["prefill_passes"] < n)
    if not plan:
        assert st["prefill_passes"] == n
