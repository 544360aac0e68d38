"""The "beam-trap" LLaMA: a tiny LLaMA made a token-transition machine (the construction of tests/golden_utils.py's decode
chain, with exactly orthonormal state directions) whose beam search is decisive and differs from greedy decoding.

After state token t the residual stream is dominated by embed[t] = 16 * dir_t, and lm_head[u] carries logit(t, u) / 8 * dir_t,
so logit(u | t) ~ logit(t, u).  Per batch row r (its own token ids; the stop sequence and EOS are shared):
  S  -> A 20, B 19, fan            greedy takes A ...
  A  -> EOS 20, A1 19.1, fan       ... and then EOS: greedy = [A, EOS]
  B  -> B1 22, fan;  B1 -> B2 -> ... -> B7 -> X1 -> X2, each 22 over a fan
with (X1, X2) = (2277, 29937), the evaluation script's two-token stop.  [A, EOS] has the larger log-prob sum (about -1 against
-1.7 for the ten tokens of the B path) but the smaller mean, so it wins at length_penalty = 0 and loses at 1, where the B path,
finished by the two-token stop, is the best hypothesis.  Every state also has a fan of eight "dead" tokens of its own (logits
2.5 to 7 below its successor, 0.43 apart, the fan bases shifted per state kind and per row so that sums over different beams do
not collide), and those lm_head rows carry no random part: the fans keep the top 2 * num_beams candidates of every step apart
from the flat background.  A dead token's only continuation is EOS (logit 12 over the flat background, about -0.2 nats), so a beam
parked on one finishes at once and fills the pool.  tools/make_golden_beam.py checks all of this on the reference's forward,
and that every top-K boundary and every returned pool rank is decisive (>= 0.05 nats in fp32)."""
from __future__ import annotations

import math
from typing import Dict, List

import torch

from tests import golden_utils as gu

BEAM_TRAP = dict(D=64, layers=2, heads=4, inter=172, vocab=32000, seed=907, s0=6, fan_S=17.0, fan_A=17.05, fan_A1=17.2,
                 row_shift=0.2, dead_eos=12.0)
EOS, X1, X2 = 2, 2277, 29937
STOPS = ((X1, X2),)
N_ROWS = 3
FAN = 8


def row_tokens(r: int) -> Dict[str, object]:
    o = 1000 + 100 * r
    return dict(S=o, A=o + 1, A1=o + 2, B=o + 3, Bs=[o + 4 + i for i in range(7)])


def fan_tokens(r: int, k: int) -> List[int]:
    """the dead tokens of row r's k-th state"""
    return [5000 + 1000 * r + 10 * (k % 16) + i for i in range(FAN)]


def transitions() -> Dict[int, Dict[int, float]]:
    """state token -> {next token: target logit}; `None` marks the dead direction (every fan token)."""
    tr: Dict[object, Dict[int, float]] = {}
    k = 0

    def with_fan(r, base, extra):                      # every state its own fan tokens: one lm_head direction each
        nonlocal k
        d = {fan_tokens(r, k)[i]: base - 0.43 * i for i in range(FAN)}
        k += 1
        d.update(extra)
        return d

    for r in range(N_ROWS):
        t = row_tokens(r)
        tr[t["S"]] = with_fan(r, BEAM_TRAP["fan_S"], {t["A"]: 20.0, t["B"]: 19.0})
        tr[t["A"]] = with_fan(r, BEAM_TRAP["fan_A"], {EOS: 20.0, t["A1"]: 19.1})
        tr[t["A1"]] = with_fan(r, BEAM_TRAP["fan_A1"], {EOS: 20.5})
        chain = [t["B"]] + t["Bs"] + [X1]
        for a, b in zip(chain[:-1], chain[1:]):
            tr[a] = with_fan(r, 18.0 - BEAM_TRAP["row_shift"] * r, {b: 22.0})
    tr[X1] = {9000 + i: 17.3 - 0.43 * i for i in range(FAN)}
    tr[X1].update({X2: 22.0})
    tr[None] = {EOS: BEAM_TRAP["dead_eos"]}
    return tr


def weights() -> Dict[str, torch.Tensor]:
    c = BEAM_TRAP
    D, V = c["D"], c["vocab"]
    sd = gu.llama_weights(D, c["layers"], c["inter"], V, c["seed"], std=0.02)
    g = torch.Generator().manual_seed(c["seed"] + 1)
    q, _ = torch.linalg.qr(torch.randn(D, D, generator=g, dtype=torch.float64))
    q = q.t().float()                                  # rows: orthonormal directions
    emb = sd["llama_model.model.embed_tokens.weight"]
    lm = sd["llama_model.lm_head.weight"]
    tr = transitions()
    states = [s for s in tr if s is not None]
    dirs = {s: q[i] for i, s in enumerate(states)}
    dirs[None] = q[len(states)]
    for s in states:
        emb[s] = dirs[s] * math.sqrt(D) * 2.0
    for s, nxt in tr.items():
        for u in nxt:
            if u not in tr and u != EOS and u != X2:
                emb[u] = dirs[None] * math.sqrt(D) * 2.0
    engineered = {u for nxt in tr.values() for u in nxt}
    for u in engineered:                               # their logits are the engineered ones only: no random part
        lm[u] = 0.0
    for s, nxt in tr.items():
        for u, logit in nxt.items():
            lm[u] += logit / math.sqrt(D) * dirs[s]
    return sd


def inputs(rows: List[int]) -> torch.Tensor:
    """[B, s0, D] prompt embeddings: small noise, last position = the embedding of the row's start token."""
    c = BEAM_TRAP
    sd = weights()
    g = torch.Generator().manual_seed(c["seed"] + 2)
    x = torch.randn(len(rows), c["s0"], c["D"], generator=g) * 0.3
    for i, r in enumerate(rows):
        x[i, -1] = sd["llama_model.model.embed_tokens.weight"][row_tokens(r)["S"]]
    return x


# the committed cases (tests/golden/beam_chain.npz): name -> rows and beam arguments (max_new_tokens MAX_NEW unless given)
CASES = {
    "b1_nb2": dict(rows=[0], nb=2, lp=1.0, es=False, nrs=2),
    "b1_nb4": dict(rows=[0], nb=4, lp=1.0, es=False, nrs=2),
    "b1_nb2_lp0": dict(rows=[0], nb=2, lp=0.0, es=False, nrs=1),
    "b3_nb2": dict(rows=[0, 1, 2], nb=2, lp=1.0, es=True, nrs=1),
    "b3_nb2_nrs2": dict(rows=[0, 1, 2], nb=2, lp=1.0, es=False, nrs=2),
    # ten tokens: with four beams every running beam is parked on a dead token after the B path finishes, and their
    # flat-background continuations would decide nothing but would not be decisive either
    "b3_nb4": dict(rows=[0, 1, 2], nb=4, lp=1.0, es=False, nrs=2, max_new=10),
}
MAX_NEW, MIN_LENGTH = 16, 1
