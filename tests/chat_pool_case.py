"""The three conversations of tests/test_chat_pool_gpu.py on the peaked token-transition LLaMA (tests/golden_utils.py
decode_chain_weights), built without a device: which chain each turn starts, how a turn's context grows out of the last one, and
the keys that name its positions.  SEED was picked on the CPU with the oracle (oracle.myriad_ref.greedy_generate's margins and
tests/fp8_ref.two_ulp_horizon) so that at least MIN_WHOLE of the nine turns have no near tie; the GPU test asserts that count."""
import torch

from tests import golden_utils as gu

SESSIONS = ["a", "b", "c"]
STARTS = {"a": ["row1", "row3", "row0"], "b": ["stop835", "row0", "row2"], "c": ["row2", "row1", "row3"]}   # per turn
FIRST_ROWS = {"a": 5, "b": 23, "c": 9}
MAX_NEW, STOPS, EOS = 8, ((835,),), 2
SLOTS, CAPACITY = 3, 128
SEED, MIN_WHOLE = 1201, 7


def _tail(n, name, emb_w, g):
    """n rows of N(0, 0.3^2) noise that end on the chain's start-token embedding."""
    x = torch.randn(n, gu.DECODE_CHAIN["D"], generator=g) * 0.3
    x[-1] = emb_w[gu.DECODE_CHAINS[name][0]]
    return x


def first_turn(s, emb_w, seed=SEED):
    """(context [S, D] f32, keys [S]) of session s's first turn."""
    g = torch.Generator().manual_seed(seed + 100 * SESSIONS.index(s))
    n = FIRST_ROWS[s]
    return _tail(n, STARTS[s][0], emb_w, g), [("r", s, 0, j) for j in range(n)]


def next_turn(s, k, ctx, keys, ids, id_rows, emb_w, seed=SEED):
    """Turn k (1 or 2) of session s: the last context, the embeddings `id_rows` [len(ids), D] of ALL ids the last turn generated
    (the cache holds all but the last), and 3 to 20 new rows that end on the turn's chain start."""
    g = torch.Generator().manual_seed(seed + 100 * SESSIONS.index(s) + k)
    n = int(torch.randint(3, 21, (1,), generator=g))
    new = _tail(n, STARTS[s][k], emb_w, g)
    return (torch.cat([ctx, id_rows.to(ctx.dtype).cpu(), new], 0), list(keys) + [("t", int(t)) for t in ids]
            + [("r", s, k, j) for j in range(n)])
