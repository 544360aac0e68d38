"""The device-free side of the decode slots' split-KV choice: the rule at its boundaries, the argument's values and default, and
the view keys -- a non-split view keeps the key it had before the engine had the choice, so its captured graphs are shared."""
import inspect

import pytest

from myriad_amd import llama as M
from myriad_amd.chat import ChatPool
from myriad_amd.llama import LlamaHIP, SlotDecoder, split_kv_rows_rule


def test_the_rule_at_its_boundaries():
    """live_rows * H at most the largest product, and the longest context at least the shortest, at which split was measured
    faster (the constants' comment in llama.py)."""
    rh, keys = M.SPLIT_KV_ROWS_MAX_ROWHEADS, M.SPLIT_KV_ROWS_MIN_KEYS
    assert rh >= 32 and keys >= 128                                  # one conversation of 32 heads can qualify; at least a chunk
    H = 32
    most = rh // H                                                   # the most live rows that still split
    assert split_kv_rows_rule(most, H, keys) is True
    assert split_kv_rows_rule(most, H, keys - 1) is False
    assert split_kv_rows_rule(most + 1, H, keys) is False
    assert split_kv_rows_rule(most + 1, H, 1 << 20) is False
    assert split_kv_rows_rule(1, rh, keys) is True and split_kv_rows_rule(1, rh + 1, 1 << 20) is False     # row-heads, inclusive
    assert split_kv_rows_rule(8, H, 1 << 20) is False                # 256 workgroups fill the CUs: never measured faster
    for slots in (1, 8, 64):                                         # run(): lengths unknown up front, so None never splits
        assert split_kv_rows_rule(slots, H, 0) is False


def test_split_kv_takes_false_true_or_none_and_defaults_to_false():
    assert SlotDecoder(None, 4, 64).split_kv is False
    assert SlotDecoder(None, 4, 64, split_kv=True).split_kv is True
    assert SlotDecoder(None, 4, 64, split_kv=None).split_kv is None
    for bad in ("yes", 1, 0, "False"):
        with pytest.raises(ValueError, match="split_kv"):
            SlotDecoder(None, 4, 64, split_kv=bad)
    for fn in (SlotDecoder.__init__, LlamaHIP.slot_decoder, ChatPool.__init__):
        assert inspect.signature(fn).parameters["split_kv"].default is False


def test_a_non_split_view_keeps_its_key_and_a_split_view_has_its_own():
    key = SlotDecoder._view_key
    assert key(1.0) == 1.0 and isinstance(key(1.0), float)           # the plain step: inv_temp
    assert key(0.5, None, False) == 0.5
    assert key(0.5, (False, True)) == (0.5, False, True)             # the per-row tail: (inv_temp, device-sampled, penalty)
    assert key(0.5, (True, False)) == (None, True, False)            # a device-sampled view reads inv_temp from memory
    for args in ((1.0, None), (0.5, (False, True)), (0.5, (True, True))):
        assert key(*args, True) == ("split", key(*args, False))
        assert key(*args, True) != key(*args, False)
