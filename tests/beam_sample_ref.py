"""Beam-search multinomial sampling as the installed transformers runs it (GenerationMixin._beam_search with do_sample=True:
_get_logits_processor's chain on the log-probs, then _get_top_k_continuations' torch.multinomial(softmax(acc), 2 * num_beams)),
restated for mh_beam_sample_topk (include/myriad_hip.h) in torch fp32, with the kernel's Philox4x32-10 from tests/sampling_ref.py.

Per step, t = the index of the token being generated (t = 0: the pick from the prefill's logits).  Row r = b * nb + j of item b:
  1. lp = log_softmax(x) (a NaN log-prob is -inf: a row holding a NaN or +inf logit is all -inf, as in mh_beam_topk)
  2. repetition penalty p ON THE LOG-PROBS (HF processes log_softmax under beams), every generated id once: lp < 0 ? lp*p : lp/p
  3. the EOS ban: lp[ban] = -inf
  4. w = lp * inv_temp
  5. top-k with k = max(top_k, 2) (min_tokens_to_keep = 2 under beams with one EOS id), ties at the k-th value kept
  6. top-p over softmax of the kept w: candidate i in (w desc, id asc) order stays iff its exclusive prefix mass < top_p * total;
     the best two always stay; top_p >= 1 keeps all (HF adds no warper then)
  7. acc = w + score[r] for what stays
  8. key = acc + g, g = -log(-log(u)), u = ((x0 >> 9) + 0.5) * 2^-23, x0 = the first word of Philox4x32-10 with key = seed and
     counter (t, flat, b, 1), flat = j * V + token
  9. per item the K = 2 * nb candidates by (key desc, flat asc); the record holds (acc, flat) in that order.
Gumbel top-K is sampling without replacement in draw order (Plackett-Luce), the distribution of torch.multinomial(softmax(acc), K).
draw = False leaves 4-6 and the noise out: key = acc.

`near` marks a row where some candidate's exclusive prefix mass lies within 1e-5 (relative to the total) of the top-p cut, so that
fp32 summation order may legitimately move the cut (tests/sampling_ref.py sample_row's flag)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from tests import sampling_ref as S

NINF = float("-inf")
NEAR_TOL = 1e-5
TOL = 1e-5                  # |got - ref| <= TOL * max(1, |ref|): the relative tolerance of tests/sampling_ref.py's kernel family


def gumbel(seed: int, t: int, flats: Sequence[int], item: int) -> torch.Tensor:
    """g for each flat index: fp32, u = ((x0 >> 9) + 0.5) * 2^-23 (exact in fp32, never 0 or 1)."""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    x = torch.tensor([S.philox4x32_10((t, int(f), item, 1), key)[0] >> 9 for f in flats], dtype=torch.float32)
    u = (x + torch.tensor(0.5)) * torch.tensor(2.0 ** -23, dtype=torch.float32)
    return -torch.log(-torch.log(u))


def processed(x: torch.Tensor, seen_ids: Sequence[int], penalty: float, ban: int, inv_temp: float, top_k: int, top_p: float,
              draw: bool = True):
    """Steps 1-6 on one fp32 row: (w with -inf where the candidate is out, near)."""
    lp = torch.log_softmax(x.detach().float(), -1)
    lp = torch.where(torch.isnan(lp), torch.full_like(lp, NINF), lp)
    lp = S.penalize(lp, [i for i in seen_ids if 0 <= i < lp.numel()], penalty)
    if ban >= 0:
        lp[ban] = NINF
    if not draw:
        return lp, False
    V = lp.numel()
    w = lp * torch.tensor(np.float32(inv_temp))
    k = min(max(int(top_k), 2), V)
    thr = torch.topk(w, k).values[-1]
    keep = (w >= thr) & torch.isfinite(w)
    near = False
    ids = torch.nonzero(keep).flatten().numpy()
    if top_p < 1.0 and len(ids) > 2:
        wv = w.numpy()[ids].astype(np.float64)
        o = np.lexsort((ids, -wv))
        ids, wv = ids[o], wv[o]
        p = np.exp(wv - wv[0])
        cum = np.cumsum(p)
        excl, total = cum - p, cum[-1]
        mk = max(int(np.sum(excl < top_p * total)), 2)
        near = bool(np.any(np.abs(excl - top_p * total) <= NEAR_TOL * total))
        keep = torch.zeros_like(keep)
        keep[torch.from_numpy(ids[:mk])] = True
    return torch.where(keep, w, torch.full_like(w, NINF)), near


@dataclass
class Item:
    """One item's step: every kept candidate (flat -> acc / key) and the K selected, in the record's order."""
    acc: Dict[int, np.float32]
    key: Dict[int, np.float32]
    sel_flat: List[int]
    sel_acc: List[np.float32]
    sel_key: List[np.float32]
    near: bool


def step(logits: torch.Tensor, scores: torch.Tensor, seen: Sequence[Sequence[int]], B: int, nb: int, ban: int, inv_temp: float,
         top_k: int, top_p: float, penalty: float, seed: int, t: int, draw: bool = True, item0: int = 0) -> List[Item]:
    """The rule on logits [B * nb, V] fp32 (CPU), scores [B * nb], seen[r] = the ids row r's hypothesis generated."""
    R, V = logits.shape
    assert R == B * nb
    out = []
    for b in range(B):
        acc, key, near = {}, {}, False
        for j in range(nb):
            r = b * nb + j
            w, nr = processed(logits[r], seen[r], penalty, ban, inv_temp, top_k, top_p, draw)
            near |= nr
            a = w + scores[r].float()
            a = torch.where(torch.isnan(a), torch.full_like(a, NINF), a)
            if draw:
                toks = torch.nonzero(torch.isfinite(w)).flatten()
            else:                                          # no cuts: every token is a candidate; only a row's best K can be selected
                toks = torch.sort(a, descending=True, stable=True)[1][:4 * nb].sort()[0]
            flats = (j * V + toks).tolist()
            ks = a[toks] + gumbel(seed, t, flats, item0 + b) if draw else a[toks]
            acc.update(zip(flats, a[toks].numpy()))
            key.update(zip(flats, ks.numpy()))
        flats = np.array(sorted(acc), dtype=np.int64)
        keys = np.array([key[f] for f in flats], dtype=np.float32)
        order = flats[np.lexsort((flats, -keys))][:2 * nb]
        out.append(Item(acc, key, [int(f) for f in order], [acc[int(f)] for f in order], [key[int(f)] for f in order], near))
    return out


# ------------------------------------------------------------------------------------------------ the shared case grid
@dataclass
class Case:
    name: str
    V: int
    nb: int
    B: int
    top_k: int = 50
    top_p: float = 1.0
    temperature: float = 1.0
    penalty: float = 1.0
    ban: int = -1
    t: int = 7
    ldl_extra: int = 0             # ldl = V + ldl_extra
    first: bool = False            # the t = 0 layout: one logits row per item repeated nb times, scores (0, -1e9, ...)
    seed: int = 0
    _cache: Optional[dict] = field(default=None, repr=False)

    @property
    def inv_temp(self) -> float:
        return float(np.float32(1.0 / self.temperature))   # what the decode loop uploads: 1 / temperature rounded to fp32

    def inputs(self) -> dict:
        """logits [R, V], scores [R], seen (lists of ids per row), the Philox seed: the same tensors on every call."""
        if self._cache is None:
            g = torch.Generator().manual_seed(7919 * self.seed + self.V + 131 * self.nb + self.B)
            R = self.B * self.nb
            if self.first:
                logits = (torch.randn(self.B, self.V, generator=g) * 3.0).repeat_interleave(self.nb, 0)
                scores = torch.full((R,), -1.0e9)
                scores[::self.nb] = 0.0
                seen = [[] for _ in range(R)]
            else:
                logits = torch.randn(R, self.V, generator=g) * 3.0
                scores = -torch.rand(R, generator=g) * 5.0
                n_seen = min(self.V // 2, 40)
                seen = [torch.randperm(self.V, generator=g)[:int(torch.randint(0, n_seen + 1, (1,), generator=g))].tolist()
                        for _ in range(R)] if self.penalty != 1.0 else [[] for _ in range(R)]
                if self.penalty != 1.0:                    # every other row has also generated its three likeliest tokens
                    for r in range(1, R, 2):
                        seen[r] = sorted(set(seen[r]) | set(torch.topk(logits[r], 3).indices.tolist()))
            philox_seed = int(torch.randint(0, 2**63 - 1, (1,), generator=g))
            self._cache = dict(logits=logits, scores=scores, seen=seen, seed=philox_seed, ref=None)
        return self._cache

    def ref(self) -> List[Item]:
        c = self.inputs()
        if c["ref"] is None:                               # computed once, shared by the tests that need it
            c["ref"] = step(c["logits"], c["scores"], c["seen"], self.B, self.nb, self.ban, self.inv_temp, self.top_k, self.top_p,
                            self.penalty, c["seed"], 0 if self.first else self.t)
        return c["ref"]


def seen_bitmap(seen: Sequence[Sequence[int]], V: int) -> torch.Tensor:
    """int32 [R, ceil(V / 32)] bitmaps of the ids in seen[r]."""
    W = (V + 31) // 32
    bm = np.zeros((len(seen), W), dtype=np.uint32)
    for r, ids in enumerate(seen):
        for i in ids:
            bm[r, i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return torch.from_numpy(bm.view(np.int32))


def _grid() -> List[Case]:
    """Every value of the issue's grid at least once, each knob crossed with the vocabulary sizes at which the row kernel takes
    another shape (V = 16 / 36: less than one value per thread; 4100: the second register, partly; 32000 / 32768: every register,
    with and without padding), kept small: the reference walks every kept candidate's Philox stream in Python."""
    cs, n = [], 0
    for V in (16, 36, 4100, 32000, 32768):
        for nb, B, top_k, top_p, temp, pen, ban in ((2, 1, 5, 1.0, 1.0, 1.0, False), (3, 3, 50, 0.9, 0.7, 1.3, True),
                                                    (8, 1, 1, 0.01, 3.0, 1.0, True), (2, 3, 1024, 0.9, 1.0, 1.3, False),
                                                    (3, 1, 50, 1.0, 3.0, 1.3, False), (8, 3, 5, 0.9, 0.7, 1.0, True)):
            if V < 2 * nb:
                continue
            n += 1
            cs.append(Case(f"V{V}_nb{nb}_B{B}_k{top_k}_p{top_p}_T{temp}_pen{pen}_ban{int(ban)}", V, nb, B, top_k, top_p, temp, pen,
                           2 if ban else -1, seed=n))
    cs.append(Case("first_V32000_nb3", 32000, 3, 3, 50, 0.9, 0.7, 1.0, 2, first=True, seed=101))
    cs.append(Case("first_V36_nb8_k1", 36, 8, 1, 1, 1.0, 1.0, 1.0, -1, first=True, seed=102))
    cs.append(Case("first_V16_nb2", 16, 2, 3, 5, 0.9, 1.0, 1.0, 2, first=True, seed=103))
    cs.append(Case("ldl_V4100_nb2", 4100, 2, 3, 50, 0.9, 0.7, 1.3, 2, ldl_extra=12, seed=104))
    cs.append(Case("ldl_V36_nb3", 36, 3, 1, 5, 1.0, 1.0, 1.0, -1, ldl_extra=4, seed=105))
    cs.append(Case("V32768_nb2_k1024_p001", 32768, 2, 1, 1024, 0.01, 1.0, 1.0, -1, seed=106))
    return cs


CASES: List[Case] = _grid()


# ------------------------------------------------------------------------------------------------ the distribution case
DIST = dict(nb=2, V=8, scores=(0.0, -0.7), seed=1234, steps=8, items=512)


def dist_logits() -> torch.Tensor:
    """[2, 8] fp32 logits of the distribution case, the same for every item."""
    return torch.randn(2, 8, generator=torch.Generator().manual_seed(4321)) * 1.5


def plackett_luce() -> dict:
    """Exact first-draw and ordered first-pair probabilities of the distribution case (fp64): {flat: p}, {(flat1, flat2): p}."""
    x = dist_logits().double()
    acc = (torch.log_softmax(x, -1) + torch.tensor(DIST["scores"], dtype=torch.float64)[:, None]).reshape(-1)
    p = torch.softmax(acc, 0).numpy()
    first = {i: float(p[i]) for i in range(p.size)}
    pair = {(i, j): float(p[i] * p[j] / (1.0 - p[i])) for i in range(p.size) for j in range(p.size) if i != j}
    return dict(first=first, pair=pair)


def check_counts(firsts: Sequence[int], pairs: Sequence[tuple]) -> dict:
    """The issue's bounds on N draws: every outcome with expectation >= 20 lies within 5 sqrt(N p (1 - p)) of N p.  Returns the
    worst z of the first draws and of the pairs and how many of each were checked; raises AssertionError on a miss."""
    pl, N = plackett_luce(), len(firsts)
    assert N == len(pairs) == DIST["steps"] * DIST["items"]
    worst = {}
    for what, got, want in (("first", firsts, pl["first"]), ("pair", pairs, pl["pair"])):
        counts: Dict[object, int] = {}
        for o in got:
            counts[o] = counts.get(o, 0) + 1
        zs = []
        for o, p in want.items():
            if N * p < 20:
                continue
            sd = float(np.sqrt(N * p * (1 - p)))
            z = abs(counts.get(o, 0) - N * p) / sd
            assert z <= 5.0, (what, o, counts.get(o, 0), N * p, z)
            zs.append(z)
        worst[what] = (max(zs), len(zs))
    return worst


# ------------------------------------------------------------------------------------------------ the whole search
def beam_search(logits_fn, B: int, nb: int, max_new_tokens: int, eos_id: int, min_length: int, length_penalty: float, stop_seqs,
                penalty: float = 1.0, draw: bool = False, inv_temp: float = 1.0, top_k: int = 50, top_p: float = 1.0, seed: int = 0,
                num_return_sequences: int = 1):
    """tests/beam_ref.beam_search (early_stopping=False) with the step's top-K replaced by `step` above: the penalty follows each
    hypothesis's own generated ids, and with `draw` the candidates are the kernel's Gumbel top-K.  Returns (ids, scores)."""
    from tests import beam_ref
    NEG, K, nrs = beam_ref.NEG, 2 * nb, num_return_sequences
    run_scores = torch.zeros((B, nb), dtype=torch.float32)
    run_scores[:, 1:] = NEG
    run_seqs = [[() for _ in range(nb)] for _ in range(B)]
    fin_scores = torch.full((B, nb), NEG, dtype=torch.float32)
    fin_seqs = [[() for _ in range(nb)] for _ in range(B)]
    is_fin = torch.zeros((B, nb), dtype=torch.bool)
    unsat = torch.ones((B, 1), dtype=torch.bool)
    top_mask = torch.arange(K) < nb
    for cur in range(max_new_tokens):
        logits = logits_fn([(b, run_seqs[b][j]) for b in range(B) for j in range(nb)]).to(torch.float32)
        V = logits.shape[-1]
        items = step(logits, run_scores.reshape(-1), [run_seqs[b][j] for b in range(B) for j in range(nb)], B, nb,
                     eos_id if cur < min_length else -1, inv_temp, top_k, top_p, penalty, seed, cur, draw)
        sel = torch.tensor([it.sel_flat for it in items])
        top_scores = torch.tensor(np.array([it.sel_acc for it in items], dtype=np.float32))
        parent, tok = (sel // V).tolist(), (sel % V).tolist()
        cand = [[run_seqs[b][parent[b][k]] + (tok[b][k],) for k in range(K)] for b in range(B)]
        hits = torch.tensor([[beam_ref.hits_stop(c, eos_id, stop_seqs) or cur + 1 >= max_new_tokens for c in cb] for cb in cand])
        run_lp = top_scores + hits.to(torch.float32) * NEG
        nxt = beam_ref._topk_stable(run_lp, nb)
        run_scores = torch.gather(run_lp, 1, nxt)
        run_seqs = [[cand[b][k] for k in nxt[b].tolist()] for b in range(B)]
        did = hits & top_mask[None, :]
        lp_scores = top_scores / ((cur + 1) ** length_penalty)
        lp_scores += (~unsat).to(torch.float32) * NEG
        lp_scores += (~did) * NEG
        merged = torch.cat((fin_scores, lp_scores), dim=1)
        keep = beam_ref._topk_stable(merged, nb)
        merged_seqs = [fin_seqs[b] + cand[b] for b in range(B)]
        fin_scores = torch.gather(merged, 1, keep)
        fin_seqs = [[merged_seqs[b][i] for i in keep[b].tolist()] for b in range(B)]
        is_fin = torch.gather(torch.cat((is_fin, did), dim=1), 1, keep)
        best_run = run_scores[:, :1] / ((cur + 1) ** length_penalty)
        worst = torch.where(is_fin, torch.min(fin_scores, dim=1, keepdim=True)[0], NEG)
        unsat = unsat & torch.any(best_run > worst, dim=-1, keepdim=True)
        if not bool(torch.any(unsat)) or bool(torch.all(hits)):
            break
    seqs = [fin_seqs[b][i] for b in range(B) for i in range(nrs)]
    return seqs, torch.stack([fin_scores[b, i] for b in range(B) for i in range(nrs)])
