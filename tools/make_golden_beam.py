#!/usr/bin/env python3
"""Generate tests/golden/beam_chain.npz: beam search (tests/beam_ref.py, the installed transformers' rules) over the REFERENCE's
own modeling_llama forward on the beam-trap LLaMA of tests/beam_fixture.py, plus greedy decoding of the same prompts.

The reference is loaded by tools/make_golden.py's loaders; the fixture holds only ids and scores (weights come from seeds).
Checked here before anything is written: greedy and beam search differ, the early-EOS hypothesis wins at length_penalty = 0
and loses at 1, a hypothesis is finished by the two-token stop, and every top-2*nb boundary of every step (the candidates
that enter and the first one that misses) and every returned pool rank is at least 0.05 nats from its neighbour in fp32.

Usage:  python tools/make_golden_beam.py [--ref PATH_TO_REFERENCE_CHECKOUT]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden import load_reference, load_sd, ref_llama, save  # noqa: E402
from tests import beam_fixture as bf  # noqa: E402
from tests import beam_ref  # noqa: E402

GAP = 0.05


def logits_fn_for(lm, x):
    emb = lm.model.embed_tokens.weight

    def fn(prefixes):
        out = []
        for b, seq in prefixes:            # full forward per prefix: no cache to reorder
            e = torch.cat([x[b], emb[list(seq)]], 0) if seq else x[b]
            out.append(lm(inputs_embeds=e[None], attention_mask=torch.ones(1, e.shape[0], dtype=torch.long),
                          return_dict=True).logits[0, -1].float())
        return torch.stack(out)
    return fn


def memo(fn):
    cache = {}

    def f(prefixes):
        miss = [p for p in prefixes if p not in cache]
        if miss:
            for p, row in zip(miss, fn(miss)):
                cache[p] = row
        return torch.stack([cache[p] for p in prefixes])
    return f


def check_decisive(name, info, nrs):
    for t, (sc, _) in enumerate(info["trace"]):
        gaps = sc[:, :-1] - sc[:, 1:]
        live = sc[:, :-1] > -1e8
        assert bool((gaps[live] >= GAP).all()), (name, t, sc)
    pool = info["pool"]
    for b in range(pool.shape[0]):
        p = pool[b][pool[b] > -1e8][:nrs + 1]
        assert bool(((p[:-1] - p[1:]) >= GAP).all()), (name, b, pool[b])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("MYRIAD_REFERENCE", ""))
    a = ap.parse_args()
    torch.set_num_threads(8)
    M = load_reference(a.ref)
    c = bf.BEAM_TRAP
    lm = ref_llama(M, c["D"], c["layers"], c["heads"], c["inter"], c["vocab"])
    load_sd(lm, bf.weights(), "llama_model.")
    out = {}
    with torch.no_grad():
        x3 = bf.inputs(list(range(bf.N_ROWS)))
        fn = memo(logits_fn_for(lm, x3))
        # greedy (arg-max, EOS banned at step 0, per-row EOS) of every row
        greedy = []
        for r in range(bf.N_ROWS):
            seq = ()
            for t in range(bf.MAX_NEW):
                lg = fn([(r, seq)])[0].clone()
                if t < bf.MIN_LENGTH:
                    lg[bf.EOS] = float("-inf")
                seq = seq + (int(lg.argmax()),)
                if seq[-1] == bf.EOS:
                    break
            greedy.append(seq)
        L = max(len(s) for s in greedy)
        out["greedy_ids"] = torch.tensor([list(s) + [bf.EOS] * (L - len(s)) for s in greedy])
        for name, cs in bf.CASES.items():
            rows = cs["rows"]
            sub = memo(lambda prefixes, rows=rows: fn([(rows[b], s) for b, s in prefixes]))
            ids, scores, info = beam_ref.beam_search(sub, len(rows), cs["nb"], cs.get("max_new", bf.MAX_NEW), bf.EOS,
                                                     min_length=bf.MIN_LENGTH,
                                                     length_penalty=cs["lp"], early_stopping=cs["es"],
                                                     num_return_sequences=cs["nrs"], stop_seqs=bf.STOPS, return_trace=True)
            check_decisive(name, info, cs["nrs"])
            print(name, ids.tolist(), scores.tolist())
            out[name + "_ids"], out[name + "_scores"] = ids, scores
            out[name + "_lengths"] = torch.tensor(info["lengths"])
    t0 = bf.row_tokens(0)
    b_path = [t0["B"]] + t0["Bs"] + [bf.X1, bf.X2]
    assert list(greedy[0]) == [t0["A"], bf.EOS], greedy[0]
    assert out["b1_nb2_ids"][0].tolist() == b_path, out["b1_nb2_ids"]          # the two-token stop finished the winner
    assert out["b1_nb2_lp0_ids"][0].tolist()[:2] == [t0["A"], bf.EOS]           # length_penalty 0: the early EOS wins
    assert out["b1_nb2_ids"][1].tolist()[:2] == [t0["A"], bf.EOS]               # ... and loses at 1
    save("beam_chain", **out)


if __name__ == "__main__":
    main()
