"""The packed batch of tests/test_ragged_past_gpu.py's kernel tests (mh_attn_prefill_ragged_past: new rows on top of a cached
prefix), built without a device so that the CPU suite can check the condition the fp64 test puts on it
(tests/test_ragged_past_cpu.py).  The layout follows tests/ragged_case.py."""
import torch

from tests import fp64_bounds as fb

BF16, I32 = torch.bfloat16, torch.int32

H = 2
# (past, len): no prefix; a one-row prefix; a boundary tile that mixes cache and new rows; a tile-aligned prefix; a single new row
# (the minimal turn); a multi-tile prefix with a multi-tile chunk; past + len == T_CAP
SEGS = [(0, 17), (1, 64), (63, 2), (64, 65), (65, 1), (130, 100), (192, 64)]
SLOTS = [5, 0, 3, 6, 1, 4, 7]            # of 8: slot 2 is named by no segment
N_SLOTS, T_CAP = 8, 256
FREE_SLOT = 2
POS_OFF = [0, 0, 0, 5, 0, 0, 0]          # positions are the caller's: the fourth segment's are past + i + 5
GAP_AFTER, GAP, TAIL = 2, 3, 5           # 3 poisoned rows after the third segment, 5 poisoned padding rows at the end
# One-row segments on long prefixes, on top of the list above: a one-row segment takes the decode kernel's arithmetic
# (csrc/attn_ragged.hip one_row_attention), whose loops only turn at these sizes -- past + 1 = 113 keys is the first at which the
# eight-keys-at-a-time P.V loop runs (for one wave), 129 the first with a second pass of the score loop, 201 and 256 (= T_CAP)
# have every wave in both loops and the new row's key (read from LDS, not from the cache) inside the unrolled loop.
ONE_ROW_SEGS = [(112, 1), (128, 1), (200, 1), (255, 1)]
ONE_ROW_SLOTS = [3, 0, 4, 1]             # of 8: the rest named by no segment


def past_layout(segs=SEGS, slots=SLOTS, pos_off=POS_OFF):
    """(segment table [(row0, len, slot, past)], M, pos [M] int32 with -1 outside the segments)."""
    seg, row = [], 0
    for i, ((past, n), s) in enumerate(zip(segs, slots)):
        seg.append((row, n, s, past))
        row += n + (GAP if i == GAP_AFTER else 0)
    M = row + TAIL
    pos = torch.full((M,), -1, dtype=I32)
    for (r0, n, _, past), off in zip(seg, pos_off):
        pos[r0:r0 + n] = torch.arange(n, dtype=I32) + past + off
    return seg, M, pos


def past_inputs(D, device, segs=SEGS, slots=SLOTS, pos_off=POS_OFF, seed=500):
    """(qkv frame [M, 3W + 64] bf16, prefixes, seg, M, pos).  qkv: poison everywhere, the recipe of ragged_case.ragged_inputs in
    the segments' [q | k | v] windows (unit normal rows, the keys of each segment's last-but-one row times 4).  prefixes[i]
    [past_i, 2W] bf16 N(0, 1): the rows cache[slot_i] holds already, k | v, the k taken as already rotated."""
    seg, M, pos = past_layout(segs, slots, pos_off)
    W = H * D
    qkv = fb.poisoned((M, 3 * W + 64), BF16, device)
    prefixes = []
    for i, (r0, n, _, past) in enumerate(seg):
        x = fb.rnd(n, 3 * W, seed=seed + 10 * D + i).to(BF16)
        if n > 2:
            x[n - 2, W:2 * W] = (x[n - 2, W:2 * W].float() * 4).to(BF16)
        qkv[r0:r0 + n, :3 * W] = x.to(device)
        prefixes.append(fb.rnd(past, 2 * W, seed=seed + 200 + 10 * D + i).to(BF16).to(device))
    return qkv, prefixes, seg, M, pos


def cache_frame(D, prefixes, seg, device):
    """The slot caches [N_SLOTS, T_CAP, 2W]: the prefix rows in place and EVERYTHING else poison, rows >= past of the named slots
    included -- the kernel must never read those."""
    cache = fb.poisoned((N_SLOTS, T_CAP, 2 * H * D), BF16, device)
    for (_, _, slot, past), pre in zip(seg, prefixes):
        cache[slot, :past] = pre
    return cache


def one_row_inputs(D, device):
    """past_inputs for ONE_ROW_SEGS (seeds 900 + 10 * D + i), positions past + i."""
    return past_inputs(D, device, ONE_ROW_SEGS, ONE_ROW_SLOTS, [0] * len(ONE_ROW_SEGS), seed=900)
