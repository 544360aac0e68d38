"""The packed batches of tests/test_shared_prefix_gpu.py's kernel tests (mh_attn_prefill_ragged_shared: several segments that
continue the SAME cached prefix), built without a device so that the CPU suite can check the condition the fp64 test puts on them
(tests/test_answer_scores_cpu.py).  qkv, the rows and `pos` are tests/ragged_past_case.py's, unchanged -- its SEGS, seeds, gap and
tail rows; only the slot column differs, so that slots repeat, and each named slot holds ONE prefix of which a segment sees its
first `past` rows."""
import torch

from tests import fp64_bounds as fb
from tests import ragged_past_case as pc

BF16 = torch.bfloat16

H, N_SLOTS, T_CAP = pc.H, pc.N_SLOTS, pc.T_CAP
# (0,17) (1,64) (63,2) (64,65) on one slot, (65,1) (130,100) (192,64) on another: equal slots with different past, a segment
# without a prefix beside ones with, a one-row segment beside multi-tile ones
SHARED_SLOTS = [5, 5, 5, 5, 1, 1, 1]
# the four one-row segments (112,1) (128,1) (200,1) (255,1) all on one slot
ONE_ROW_SHARED_SLOTS = [3, 3, 3, 3]


def _share(D, device, inputs, slots, seed):
    """(qkv, prefix of each named slot {slot: [max past, 2W] bf16}, seg with the slot column replaced, M, pos)."""
    qkv, _, seg, M, pos = inputs(D, device)
    seg = [(r0, n, s, past) for (r0, n, _, past), s in zip(seg, slots)]
    W = H * D
    prefix = {}
    for s in sorted(set(slots)):
        rows = max(past for _, _, slot, past in seg if slot == s)
        prefix[s] = fb.rnd(rows, 2 * W, seed=seed + 10 * D + s).to(BF16).to(device)
    return qkv, prefix, seg, M, pos


def shared_inputs(D, device):
    return _share(D, device, pc.past_inputs, SHARED_SLOTS, 1300)


def one_row_shared_inputs(D, device):
    return _share(D, device, pc.one_row_inputs, ONE_ROW_SHARED_SLOTS, 1700)


def shared_cache_frame(D, prefix, seg, device):
    """The slot caches [N_SLOTS, T_CAP, 2W]: each named slot's prefix in place and EVERYTHING else poison -- rows at or above the
    largest `past` of a named slot and all unnamed slots; the kernel must neither read nor write those."""
    cache = fb.poisoned((N_SLOTS, T_CAP, 2 * H * D), BF16, device)
    for s, pre in prefix.items():
        cache[s, :pre.shape[0]] = pre
    return cache
