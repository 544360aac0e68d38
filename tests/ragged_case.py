"""The packed batch of tests/test_ragged_prefill_gpu.py's kernel tests, built without a device so that the CPU suite can check the
condition the fp64 test puts on it (tests/test_ragged_prefill_cpu.py)."""
import torch

from tests import fp64_bounds as fb

BF16, I32 = torch.bfloat16, torch.int32

H = 2
LENS = [1, 63, 64, 65, 129, 17]          # one row, a tile minus one, a tile, a tile plus one, two tiles plus one, a partial tile
SLOTS = [5, 0, 3, 6, 1, 4]               # of 7: slot 2 is named by no segment
N_SLOTS, T_CAP = 7, 192
POS_OFF = [0, 37, 0, 0, 37, 0]           # positions are the caller's: two segments do not start at 0
GAP_AFTER, GAP, TAIL = 2, 3, 5           # 3 poisoned rows after the third segment, 5 poisoned padding rows at the end


def ragged_layout():
    """(segment table [(row0, len, slot)], M, pos [M] int32 with -1 outside the segments)."""
    seg, row = [], 0
    for i, (n, s) in enumerate(zip(LENS, SLOTS)):
        seg.append((row, n, s))
        row += n + (GAP if i == GAP_AFTER else 0)
    M = row + TAIL
    pos = torch.full((M,), -1, dtype=I32)
    for (r0, n, _), off in zip(seg, POS_OFF):
        pos[r0:r0 + n] = torch.arange(n, dtype=I32) + off
    return seg, M, pos


def ragged_inputs(D, device):
    """The qkv frame [M, 3W + 64] bf16: poison everywhere, N(0, 1) in the segments' [q | k | v] windows (the recipe of
    tests/test_attention_edges_gpu.py::_rope_case: unit normal rows, the keys of each segment's last-but-one row times 4, a late
    score spike that makes the running max jump)."""
    seg, M, pos = ragged_layout()
    W = H * D
    qkv = fb.poisoned((M, 3 * W + 64), BF16, device)
    for i, (r0, n, _) in enumerate(seg):
        x = fb.rnd(n, 3 * W, seed=300 + 10 * D + i).to(BF16)
        if n > 2:
            x[n - 2, W:2 * W] = (x[n - 2, W:2 * W].float() * 4).to(BF16)
        qkv[r0:r0 + n, :3 * W] = x.to(device)
    return qkv, seg, M, pos
