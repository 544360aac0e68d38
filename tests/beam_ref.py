"""Beam search as the installed transformers runs it (GenerationMixin._beam_search and its helpers
_get_top_k_continuations, _get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic,
_beam_search_has_unfinished_sequences), restated over a logits callable so that any forward can drive it: the CPU oracle,
the reference's modeling_llama, a transformers model.  The arithmetic is HF's, step for step in fp32, so scores agree to
rounding; only the tie rule is pinned down where torch.topk leaves it open: equal scores go to the lower index.

The rules, in the order a step applies them (gen_len = tokens generated including the new one):
  * log_softmax of the fp32 logits of every running beam; while fewer than `min_length` tokens were generated the EOS
    log-prob is -inf (the prompt is embeddings only, so only generated tokens count); add the beam's running score.  Before
    the first step the running scores are 0 for beam 0 and -1e9 for the others.
  * per item the top K = 2 * num_beams candidates over num_beams * V, best first, ties to the lower flat index beam * V + token.
  * a candidate finishes when its token is EOS, when its sequence ends with a stop sequence, or at max_new_tokens.
  * next running beams: the best num_beams candidates after adding -1e9 to the finished ones (so a finished candidate runs on
    only when fewer than num_beams unfinished ones exist).
  * the finished pool: only candidates ranked below num_beams that finished may enter, scored sum_logprobs / gen_len ** lp;
    nothing enters once the early-stop heuristic said no improvement is possible, nor (early_stopping=True) once the pool is
    full; the pool keeps its best num_beams.
  * the early-stop heuristic (per item, sticky): the best running score / L ** lp must still beat the pool's worst, L = the
    current generated length, or max_new_tokens when early_stopping == "never" and lp > 0.
  * the loop ends when no item can improve, or (early_stopping=True) when every pool is full, or when every candidate finished.
Output: the best num_return_sequences finished hypotheses per item, best first, batch-major, right-padded with `pad_id`.
"""
from __future__ import annotations

from typing import Callable, List, Sequence, Tuple

import torch

NEG = -1.0e9


def _topk_stable(x: torch.Tensor, k: int) -> torch.Tensor:
    """Indices of the k largest along dim 1, best first, equal values to the lower index."""
    return torch.sort(x, dim=1, descending=True, stable=True)[1][:, :k]


def hits_stop(seq: Sequence[int], eos_id: int, stop_seqs) -> bool:
    if len(seq) and seq[-1] == eos_id:
        return True
    return any(len(seq) >= len(st) and tuple(seq[-len(st):]) == tuple(st) for st in stop_seqs)


def beam_search(logits_fn: Callable[[List[Tuple[int, Tuple[int, ...]]]], torch.Tensor], B: int, num_beams: int,
                max_new_tokens: int, eos_id: int, min_length: int = 0, length_penalty: float = 1.0, early_stopping=False,
                num_return_sequences: int = 1, stop_seqs=(), pad_id=None, return_trace: bool = False):
    """logits_fn(prefixes) -> [len(prefixes), V] fp32 logits of the next token, prefixes = [(item, generated ids)] in row order
    (item-major, num_beams rows per item).  Returns (ids [B * nrs, L] int64, scores [B * nrs] f32) and, with return_trace,
    the per-step records [(scores [B, K + 1], flat [B, K + 1])] (the top K and the first candidate that misses them), the
    finished pools' scores [B, num_beams], how many hypotheses finished and each returned hypothesis's length."""
    nb, K, nrs = num_beams, 2 * num_beams, num_return_sequences
    if not 1 <= nrs <= nb:
        raise ValueError(f"num_return_sequences={nrs} must be in [1, num_beams={nb}]")
    pad = eos_id if pad_id is None else pad_id
    run_scores = torch.zeros((B, nb), dtype=torch.float32)
    run_scores[:, 1:] = NEG
    run_seqs = [[() for _ in range(nb)] for _ in range(B)]
    fin_scores = torch.full((B, nb), NEG, dtype=torch.float32)
    fin_seqs = [[() for _ in range(nb)] for _ in range(B)]
    is_fin = torch.zeros((B, nb), dtype=torch.bool)
    unsat = torch.ones((B, 1), dtype=torch.bool)           # the early-stop heuristic still allows an improvement
    top_mask = torch.arange(K) < nb
    trace = []
    for cur in range(max_new_tokens):
        logits = logits_fn([(b, run_seqs[b][j]) for b in range(B) for j in range(nb)]).to(torch.float32)
        V = logits.shape[-1]
        logp = torch.nn.functional.log_softmax(logits, dim=-1)
        if cur < min_length:
            logp[:, eos_id] = float("-inf")
        acc = (logp.view(B, nb, V) + run_scores[:, :, None]).reshape(B, nb * V)
        sel1 = _topk_stable(acc, K + 1)                    # the top K and the first candidate that misses them
        sel = sel1[:, :K]
        top_scores = torch.gather(acc, 1, sel)
        trace.append((torch.gather(acc, 1, sel1), sel1))
        parent, tok = (sel // V).tolist(), (sel % V).tolist()
        cand = [[run_seqs[b][parent[b][k]] + (tok[b][k],) for k in range(K)] for b in range(B)]
        hits = torch.tensor([[hits_stop(c, eos_id, stop_seqs) or cur + 1 >= max_new_tokens for c in cb] for cb in cand])
        # running beams for the next step
        run_lp = top_scores + hits.to(torch.float32) * NEG
        nxt = _topk_stable(run_lp, nb)
        run_scores = torch.gather(run_lp, 1, nxt)
        run_seqs = [[cand[b][k] for k in nxt[b].tolist()] for b in range(B)]
        # the finished pool
        did = hits & top_mask[None, :]
        lp_scores = top_scores / ((cur + 1) ** length_penalty)
        full = torch.all(is_fin, dim=-1, keepdim=True) & (early_stopping is True)
        lp_scores += full.to(torch.float32) * NEG
        lp_scores += (~unsat).to(torch.float32) * NEG
        lp_scores += (~did) * NEG
        merged = torch.cat((fin_scores, lp_scores), dim=1)
        keep = _topk_stable(merged, nb)
        merged_seqs = [fin_seqs[b] + cand[b] for b in range(B)]
        fin_scores = torch.gather(merged, 1, keep)
        fin_seqs = [[merged_seqs[b][i] for i in keep[b].tolist()] for b in range(B)]
        is_fin = torch.gather(torch.cat((is_fin, did), dim=1), 1, keep)
        # stop?
        gen_len = cur + 1
        best_len = max_new_tokens if (early_stopping == "never" and length_penalty > 0.0) else gen_len
        best_run = run_scores[:, :1] / (best_len ** length_penalty)
        worst = torch.where(is_fin, torch.min(fin_scores, dim=1, keepdim=True)[0], NEG)
        unsat = unsat & torch.any(best_run > worst, dim=-1, keepdim=True)
        going = bool(torch.any(unsat)) and not (bool(torch.all(is_fin)) and early_stopping is True) and not bool(torch.all(hits))
        if not going:
            break
    seqs = [fin_seqs[b][i] for b in range(B) for i in range(nrs)]
    scores = torch.stack([fin_scores[b, i] for b in range(B) for i in range(nrs)])
    L = max(1, max(len(s) for s in seqs))
    ids = torch.full((len(seqs), L), pad, dtype=torch.long)
    for r, s in enumerate(seqs):
        ids[r, :len(s)] = torch.tensor(s, dtype=torch.long)
    if return_trace:
        return ids, scores, dict(trace=trace, pool=fin_scores, finished=int(is_fin.sum()), lengths=[len(s) for s in seqs])
    return ids, scores


def rescore(logits_fn, items: Sequence[int], seqs: Sequence[Sequence[int]], eos_id: int, min_length: int, length_penalty: float):
    """What beam search reports for a finished hypothesis: the sum of its tokens' log-probs (EOS banned while fewer than
    min_length were generated) / len ** lp.  seqs[r] = hypothesis r's own tokens (no padding), items[r] = its batch item."""
    out = []
    for b, seq in zip(items, seqs):
        seq = list(seq)
        total = torch.zeros((), dtype=torch.float32)
        for t in range(len(seq)):
            lp = torch.nn.functional.log_softmax(logits_fn([(b, tuple(seq[:t]))]).to(torch.float32)[0], dim=-1)
            if t < min_length:
                lp[eos_id] = float("-inf")
            total = total + lp[seq[t]]
        out.append(total / (len(seq) ** length_penalty))
    return torch.stack(out)
