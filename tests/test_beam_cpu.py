"""Beam search without a device: tests/beam_ref.py against the installed transformers' own beam search on a tiny LLaMA, the
committed beam-trap fixture against the oracle's forward, and the argument checks of LlamaHIP.beam_generate."""
import numpy as np
import pytest
import torch

from oracle import myriad_ref as R
from tests import beam_fixture as bf
from tests import beam_ref


class _Suffix:
    """A per-row stopping criterion (one bool per hypothesis, as transformers applies it): the row ends with a stop sequence."""

    def __init__(self, stops):
        self.stops = stops

    def __call__(self, input_ids, scores, **kw):
        hit = torch.zeros(input_ids.shape[0], dtype=torch.bool)
        for st in self.stops:
            if input_ids.shape[1] >= len(st):
                hit |= (input_ids[:, -len(st):] == torch.tensor(st)).all(1)
        return hit


class _CachedLogits:
    """Drives beam_ref with the model's own KV-cached forward, in transformers' order: a prefill of num_beams copies of each
    prompt, then one token per row on the cache reordered by each row's parent."""

    def __init__(self, m, x, nb):
        self.m, self.x, self.nb, self.prev, self.cache = m, x, nb, None, None

    def __call__(self, prefixes):
        if self.prev is None:
            out = self.m(inputs_embeds=self.x.repeat_interleave(self.nb, 0), use_cache=True)
        else:
            self.cache.reorder_cache(torch.tensor([self.prev.index((b, s[:-1])) for b, s in prefixes]))
            out = self.m(input_ids=torch.tensor([[s[-1]] for _, s in prefixes]), past_key_values=self.cache, use_cache=True)
        self.cache, self.prev = out.past_key_values, list(prefixes)
        return out.logits[:, -1].float()


@pytest.fixture(scope="module")
def tiny():
    tr = pytest.importorskip("transformers")
    torch.manual_seed(0)
    cfg = tr.LlamaConfig(vocab_size=96, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                         num_key_value_heads=4, max_position_embeddings=128, pad_token_id=None, bos_token_id=1, eos_token_id=2)
    m = tr.LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        m.lm_head.weight.mul_(8.0)                     # peaked enough that EOS and the stop sequence get chosen
    return tr, m


# (num_beams, length_penalty, early_stopping, min_new_tokens, num_return_sequences, stop sequences)
CONFIGS = [
    (2, 1.0, False, 0, 1, ()),
    (4, 0.0, True, 2, 2, ()),
    (8, 2.0, "never", 1, 3, ()),
    (4, -0.5, False, 0, 4, ((5, 7),)),
    (2, 1.0, "never", 3, 2, ((5, 7), (11,))),
    (8, 0.0, False, 0, 8, ((5, 7),)),
    (4, 1.0, True, 1, 1, ((5, 7),)),
    (2, -0.5, "never", 0, 1, ()),
]


@pytest.mark.parametrize("cfg", CONFIGS, ids=[f"nb{c[0]}-lp{c[1]}-es{c[2]}-min{c[3]}-nrs{c[4]}-stops{len(c[5])}" for c in CONFIGS])
def test_beam_ref_is_transformers_beam_search(tiny, cfg):
    tr, m = tiny
    nb, lp, es, mn, nrs, stops = cfg
    B, max_new = 2, 12
    x = torch.randn(B, 5, 32, generator=torch.Generator().manual_seed(nb * 31 + mn))
    kw = dict(num_beams=nb, length_penalty=lp, early_stopping=es, num_return_sequences=nrs, max_new_tokens=max_new,
              do_sample=False, min_new_tokens=mn, eos_token_id=2, pad_token_id=2, return_dict_in_generate=True, output_scores=True)
    if stops:
        kw["stopping_criteria"] = tr.StoppingCriteriaList([_Suffix(stops)])
    with torch.no_grad():
        hf = m.generate(inputs_embeds=x, **kw)
        ids, scores = beam_ref.beam_search(_CachedLogits(m, x, nb), B, nb, max_new, 2, min_length=mn, length_penalty=lp,
                                           early_stopping=es, num_return_sequences=nrs, stop_seqs=stops)
    assert torch.equal(ids, hf.sequences), (ids, hf.sequences)
    assert float((scores - hf.sequences_scores).abs().max()) <= 1e-6


def test_beam_ref_argument_checks():
    with pytest.raises(ValueError):
        beam_ref.beam_search(lambda p: torch.zeros(len(p), 8), 1, 2, 4, 2, num_return_sequences=3)


def _oracle_logits(rows):
    c = bf.BEAM_TRAP
    sd = bf.weights()
    x = bf.inputs(rows)
    emb = sd["llama_model.model.embed_tokens.weight"]

    def fn(prefixes):
        out = []
        for b, seq in prefixes:
            e = torch.cat([x[b], emb[list(seq)]], 0) if seq else x[b]
            _, lg = R.llama_causal_lm(sd, e[None], torch.ones(1, e.shape[0]), None, c["heads"])
            out.append(lg[0, -1].float())
        return torch.stack(out)
    return fn


@pytest.mark.parametrize("name", ["b1_nb2", "b1_nb2_lp0"])
def test_committed_beam_fixture_is_what_the_oracle_searches(name):
    """tests/golden/beam_chain.npz came from the reference's modeling_llama; the oracle's forward gives the same search."""
    g = np.load("tests/golden/beam_chain.npz")
    cs = bf.CASES[name]
    with torch.no_grad():
        ids, scores = beam_ref.beam_search(_oracle_logits(cs["rows"]), len(cs["rows"]), cs["nb"], bf.MAX_NEW, bf.EOS,
                                           min_length=bf.MIN_LENGTH, length_penalty=cs["lp"], early_stopping=cs["es"],
                                           num_return_sequences=cs["nrs"], stop_seqs=bf.STOPS)
    assert ids.tolist() == g[name + "_ids"].tolist()
    assert np.abs(scores.numpy() - g[name + "_scores"]).max() < 1e-3
    t0 = bf.row_tokens(0)
    assert g["greedy_ids"][0].tolist()[:2] == [t0["A"], bf.EOS]            # greedy takes the early EOS ...
    assert g["b1_nb2_ids"][0].tolist()[-2:] == list(bf.STOPS[0])           # ... beams the path the two-token stop finishes


def test_beam_generate_argument_checks_without_a_device():
    from myriad_amd.llama import LlamaHIP
    lm = LlamaHIP.__new__(LlamaHIP)                        # the checks run before anything touches the device
    lm.V = 32000
    x = torch.zeros(1, 3, 8)
    with pytest.raises(NotImplementedError):
        lm.beam_generate(x, 9)
    with pytest.raises(ValueError):
        lm.beam_generate(x, 4, num_return_sequences=5)
    with pytest.raises(ValueError):
        lm.beam_generate(x, 4, early_stopping="sometimes")
    with pytest.raises(ValueError):
        lm.beam_generate(x, 0)
