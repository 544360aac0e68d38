"""Beam search on the device: mh_beam_topk / mh_beam_reorder_kv against torch, LlamaHIP.beam_generate against the committed
beam-trap fixture (tests/golden/beam_chain.npz, from the reference's forward) and the oracle, and MyriadHIP.generate's beam
arguments on the model built from the reference's on-disk files."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import ops  # noqa: E402
from myriad_amd.llama import LlamaHIP  # noqa: E402
from oracle import myriad_ref as R  # noqa: E402
from tests import beam_fixture as bf  # noqa: E402
from tests import beam_ref  # noqa: E402
from tests.test_entrypoints_gpu import _batch, fx, model  # noqa: E402,F401

DEV = "cuda"
GOLD = "tests/golden/beam_chain.npz"


def _topk_want(logits, scores, B, nb, ban):
    """per item the top 2*nb (score desc, flat index asc) of scores[row] + log_softmax(logits[row]) (fp64 ordering keys)"""
    R_, V = logits.shape
    rpi = R_ // B
    lp = torch.log_softmax(logits.double(), -1)
    if ban >= 0:
        lp[:, ban] = float("-inf")
    acc = (lp + scores.double()[:, None]).view(B, rpi * V).float()
    s_out, i_out = [], []
    for b in range(B):
        a = acc[b].numpy()
        order = np.lexsort((np.arange(a.size), -a))[:2 * nb]
        s_out.append(a[order])
        i_out.append(order)
    return np.stack(s_out), np.stack(i_out)


@pytest.mark.parametrize("V", [32000, 1237])
@pytest.mark.parametrize("nb,B", [(2, 1), (2, 12), (4, 3), (4, 6), (8, 1), (8, 3)])
def test_beam_topk_matches_torch(V, nb, B):
    g = torch.Generator().manual_seed(V + 10 * nb + B)
    R_ = B * nb
    ldl = V + 3
    buf = torch.randn(R_, ldl, generator=g) * 3.0
    logits = buf[:, :V]
    scores = -torch.rand(R_, generator=g) * 5.0
    scores[1::nb] = -1e9                                    # beams parked at HF's initial -1e9
    ban = 2
    dev_buf = buf.to(DEV)
    out = torch.zeros(2, B * 2 * nb, dtype=torch.int32, device=DEV)
    part_s = torch.empty(R_ * 2 * nb, dtype=torch.float32, device=DEV)
    part_i = torch.empty(R_ * 2 * nb, dtype=torch.int32, device=DEV)
    ops.beam_topk(dev_buf[:, :V], scores.to(DEV), part_s, part_i, out[0].view(torch.float32), out[1], B, nb, ban_id=ban)
    torch.cuda.synchronize()
    got_s = out[0].view(torch.float32).cpu().numpy().reshape(B, 2 * nb)
    got_i = out[1].cpu().numpy().reshape(B, 2 * nb)
    want_s, want_i = _topk_want(logits, scores, B, nb, ban)
    assert np.array_equal(got_i, want_i), (got_i, want_i)
    assert np.abs(got_s - want_s).max() <= 1e-5
    assert not np.any(got_i % V == ban)
    # one row per item (the step after a B-row prefill): flat index = token
    out.zero_()
    ops.beam_topk(dev_buf[:B, :V], scores[:B].to(DEV) * 0, part_s, part_i, out[0].view(torch.float32), out[1], B, nb, ban_id=-1)
    torch.cuda.synchronize()
    want_s, want_i = _topk_want(logits[:B], scores[:B] * 0, B, nb, -1)
    assert np.array_equal(out[1].cpu().numpy().reshape(B, 2 * nb), want_i)


def test_beam_topk_advances_pos_and_kvlen():
    B, nb, V = 2, 4, 512
    logits = torch.randn(B * nb, V, device=DEV)
    pos = torch.full((B * nb,), 7, dtype=torch.int32, device=DEV)
    kvlen = torch.full((B * nb,), 8, dtype=torch.int32, device=DEV)
    out = torch.zeros(2, B * 2 * nb, dtype=torch.int32, device=DEV)
    ps, pi = torch.empty(B * nb * 2 * nb, device=DEV), torch.empty(B * nb * 2 * nb, dtype=torch.int32, device=DEV)
    ops.beam_topk(logits, torch.zeros(B * nb, device=DEV), ps, pi, out[0].view(torch.float32), out[1], B, nb, pos=pos, kvlen=kvlen)
    torch.cuda.synchronize()
    assert pos.tolist() == [8] * (B * nb) and kvlen.tolist() == [9] * (B * nb)


@pytest.mark.parametrize("nb,B,C", [(4, 2, 128), (8, 2, 8192), (2, 3, 64)])
def test_beam_reorder_kv_matches_index_select(nb, B, C):
    L, T = 3, 70
    g = torch.Generator().manual_seed(nb * 100 + C)
    caches = [(torch.randn(B * nb, T, C, generator=g)).to(torch.bfloat16).to(DEV) for _ in range(L)]
    table = torch.tensor([c.data_ptr() for c in caches], dtype=torch.long).to(DEV)
    # duplicate parents, identity rows, a permutation
    src = []
    for b in range(B):
        par = [0] * nb
        for j in range(nb):
            par[j] = [0, j, nb - 1 - j][(b + j) % 3]
        src += [b * nb + p for p in par]
    src_t = torch.tensor(src, dtype=torch.int32)
    for lo, hi in ((9, 41), (0, 5), (13, 13)):
        before = [c.clone() for c in caches]
        ops.beam_reorder_kv(table, L, B, nb, T, C, src_t.to(DEV), torch.tensor([lo], dtype=torch.int32).to(DEV),
                            torch.tensor([hi], dtype=torch.int32).to(DEV))
        torch.cuda.synchronize()
        for c, c0 in zip(caches, before):
            want = c0.clone()
            want[:, lo:hi] = c0.index_select(0, src_t.long().to(DEV))[:, lo:hi]
            assert torch.equal(c.view(torch.int16), want.view(torch.int16))     # bits, canaries outside [lo, hi) included
    # the after-prefill broadcast: every sibling from row b * nb over [0, S0)
    before = [c.clone() for c in caches]
    bsrc = torch.arange(B, dtype=torch.int32).repeat_interleave(nb) * nb
    ops.beam_reorder_kv(table, L, B, nb, T, C, bsrc.to(DEV), torch.tensor([0], dtype=torch.int32).to(DEV),
                        torch.tensor([6], dtype=torch.int32).to(DEV))
    torch.cuda.synchronize()
    for c, c0 in zip(caches, before):
        want = c0.clone()
        want[:, :6] = c0.index_select(0, bsrc.long().to(DEV))[:, :6]
        assert torch.equal(c.view(torch.int16), want.view(torch.int16))


# ------------------------------------------------------------------------------------------------ beam_generate
@pytest.fixture(scope="module")
def trap():
    c = bf.BEAM_TRAP
    return LlamaHIP(bf.weights(), c["heads"], DEV, need_backward=False)


def _oracle_fn(rows, sd=None, lora=None):
    c = bf.BEAM_TRAP
    sd = bf.weights() if sd is None else sd
    x = bf.inputs(rows)
    emb = sd["llama_model.model.embed_tokens.weight"]

    def fn(prefixes):
        out = []
        for b, seq in prefixes:
            e = torch.cat([x[b], emb[list(seq)]], 0) if seq else x[b]
            _, lg = R.llama_causal_lm(sd, e[None], torch.ones(1, e.shape[0]), None, c["heads"], lora=lora)
            out.append(lg[0, -1].float())
        return torch.stack(out)
    return fn


def _run(lm, cs, use_graph=True, nb=None, rows=None):
    rows = cs["rows"] if rows is None else rows
    x = bf.inputs(rows).to(DEV)
    return lm.beam_generate(x, cs["nb"] if nb is None else nb, max_new_tokens=cs.get("max_new", bf.MAX_NEW), stop_ids=bf.STOPS, eos_id=bf.EOS,
                            min_length=bf.MIN_LENGTH, length_penalty=cs["lp"], early_stopping=cs["es"],
                            num_return_sequences=cs["nrs"], use_graph=use_graph, return_scores=True)


@pytest.mark.parametrize("name", list(bf.CASES))
def test_beam_generate_matches_the_reference_fixture(trap, name):
    g = np.load(GOLD)
    cs = bf.CASES[name]
    ids, scores = _run(trap, cs)
    assert ids.tolist() == g[name + "_ids"].tolist(), (name, ids, g[name + "_ids"])
    assert np.abs(scores.numpy() - g[name + "_scores"]).max() < 2e-2
    st = trap.last_generate_stats
    assert st["num_beams"] == cs["nb"] and torch.equal(st["sequences_scores"], scores)
    assert st["lengths"] == g[name + "_lengths"].tolist() and st["finished_hypotheses"] >= cs["nrs"]
    again, sc2 = _run(trap, cs, use_graph=False)          # eager steps: the same ids and scores as the graph replays
    assert torch.equal(again, ids) and torch.equal(sc2, scores)


def test_beam_differs_from_greedy_and_replays_its_graph(trap):
    g = np.load(GOLD)
    x = bf.inputs([0]).to(DEV)
    greedy = trap.greedy_generate(x, max_new_tokens=bf.MAX_NEW, stop_ids=bf.STOPS, eos_id=bf.EOS, min_length=bf.MIN_LENGTH)
    n = greedy.shape[1]
    assert greedy[0].tolist() == g["greedy_ids"][0].tolist()[:n]
    ids, _ = _run(trap, bf.CASES["b1_nb2"])
    assert ids[0].tolist()[:n] != greedy[0].tolist()
    assert trap.last_generate_stats["graph_replays"] > 0


def _check_rescored(lm, ids, rows, nb, fn, lp=1.0):
    st = lm.last_generate_stats
    per = ids.shape[0] // len(rows)
    seqs = [ids[r, :st["lengths"][r]].tolist() for r in range(ids.shape[0])]
    want = beam_ref.rescore(fn, [r // per for r in range(len(seqs))], seqs, bf.EOS, bf.MIN_LENGTH, lp)
    got = st["sequences_scores"]
    assert float((got - want).abs().max()) < 2e-2, (got, want)
    _, ref_scores = beam_ref.beam_search(fn, len(rows), nb, bf.MAX_NEW, bf.EOS, min_length=bf.MIN_LENGTH, length_penalty=lp,
                                         num_return_sequences=per, stop_seqs=bf.STOPS)
    for b in range(len(rows)):
        assert float(got[b * per]) >= float(ref_scores[b * per]) - 2e-2


def test_beam_generate_above_16_rows_runs_the_gemm_path(trap, monkeypatch):
    calls = {"gemv": 0, "gemm_rows": set()}
    gemm, gemv_packed = ops.gemm, ops.gemv_packed

    def count_gemm(a, *args, **kw):
        calls["gemm_rows"].add(a.shape[0])
        return gemm(a, *args, **kw)

    def count_gemv(*args, **kw):
        calls["gemv"] += 1
        return gemv_packed(*args, **kw)
    monkeypatch.setattr(ops, "gemm", count_gemm)
    monkeypatch.setattr(ops, "gemv_packed", count_gemv)
    monkeypatch.setattr(ops, "gemv_packed_rmsnorm", lambda *a, **k: pytest.fail("packed GEMV at 24 rows"))
    monkeypatch.setattr(ops, "gemv_packed_silu", lambda *a, **k: pytest.fail("packed GEMV at 24 rows"))
    trap._decode_ws.clear()                                 # eager steps and a fresh capture: every launch goes through Python
    cs = dict(rows=[0, 1, 2], nb=8, lp=1.0, es=False, nrs=2)
    ids, scores = _run(trap, cs)
    monkeypatch.undo()
    assert ids.shape[0] == 6
    assert calls["gemv"] == 0 and 24 in calls["gemm_rows"]   # the token steps' products ran as 24-row GEMMs
    _check_rescored(trap, ids, cs["rows"], 8, _oracle_fn(cs["rows"]))


def test_beam_generate_reusing_a_workspace_with_another_prompt(trap):
    """The workspace (its KV caches included) is kept across calls: a second call with another prompt must not see the first
    one's keys / values in any beam -- its result is the golden one and bit-equal to a run on a fresh workspace."""
    g = np.load(GOLD)
    cs = bf.CASES["b1_nb2"]
    x0 = bf.inputs([0])
    other = bf.inputs([1]) + torch.randn(x0.shape, generator=torch.Generator().manual_seed(5)) * 0.5
    trap._decode_ws.clear()
    trap.beam_generate(other.to(DEV), cs["nb"], max_new_tokens=bf.MAX_NEW, stop_ids=bf.STOPS, eos_id=bf.EOS,
                       min_length=bf.MIN_LENGTH)
    assert len(trap._decode_ws) == 1
    ids, scores = _run(trap, cs)
    assert len(trap._decode_ws) == 1                        # the same workspace served the second call
    assert ids.tolist() == g["b1_nb2_ids"].tolist()
    trap._decode_ws.clear()
    fresh_ids, fresh_scores = _run(trap, cs)
    assert torch.equal(ids, fresh_ids) and torch.equal(scores, fresh_scores)


def test_beam_generate_with_lora_attached():
    from myriad_amd.lora import PEFT_PREFIX, LoraQV, lora_param_specs
    from myriad_amd.myriad import ParamStore
    c = bf.BEAM_TRAP
    sd = bf.weights()
    r = 8
    gen = torch.Generator().manual_seed(913)
    st = ParamStore(lora_param_specs(c["layers"], c["D"], r), DEV)
    osd = dict(sd)
    for name, ishape, _ in st.specs:
        t = torch.randn(ishape, generator=gen) * (0.02 if "lora_A" in name else 0.05)
        st.p[name].copy_(t)
        osd[name.replace(PEFT_PREFIX, "llama_model.model.layers.")] = t
    lm = LlamaHIP(sd, c["heads"], DEV, need_backward=False)
    lm.attach_lora(LoraQV(c["layers"], c["D"], r, 16.0, 0.0, st.p, st.g, DEV))
    cs = dict(rows=[0], nb=4, lp=1.0, es=False, nrs=2)
    ids, _ = _run(lm, cs)
    _check_rescored(lm, ids, cs["rows"], 4, _oracle_fn(cs["rows"], osd, lora=dict(r=r, alpha=16.0, dropout_mask=None)))


# ------------------------------------------------------------------------------------------------ MyriadHIP.generate
def test_generate_takes_num_beams(model):
    tok = model.llama_tokenizer
    samples = _batch(2, train=False, seed=5)
    hashes = tok("###", add_special_tokens=False).input_ids
    from myriad_amd.myriad import StoppingCriteriaSub
    kw = {"max_new_tokens": 10, "stopping_criteria": [StoppingCriteriaSub(stops=[torch.tensor(hashes).to(DEV)])], "min_length": 1,
          "num_beams": 4, "num_return_sequences": 2, "length_penalty": 1.0, "early_stopping": False}
    model.eval()
    try:
        out = model.generate(samples, **kw)
        ids = out["token_ids"]
        assert ids.shape[0] == 4 and ids.shape[1] >= 1
        assert out["ve_anomaly_maps"].shape == samples["anomaly_maps"].shape
        st = dict(model.last_generate_stats)
        assert st["num_beams"] == 4 and st["sequences_scores"].shape == (4,) and "graph_replays" in st
        assert st["finished_hypotheses"] >= 2
        s = st["sequences_scores"].view(2, 2)
        assert bool((s[:, 0] >= s[:, 1]).all())           # best first within each item
        again = model.generate(samples, **kw)
        assert torch.equal(again["token_ids"], ids)
        assert torch.equal(again["ve_anomaly_maps"], out["ve_anomaly_maps"])
        for bad, exc in (({"do_sample": True}, NotImplementedError), ({"repetition_penalty": 1.3}, NotImplementedError),
                         ({"num_beams": 9}, NotImplementedError), ({"num_return_sequences": 5}, ValueError),
                         ({"num_beams": 0}, ValueError), ({"num_beams": -2}, ValueError), ({"num_beams": 1.5}, ValueError),
                         ({"early_stopping": "sometimes"}, ValueError)):
            with pytest.raises(exc):
                model.generate(samples, **dict(kw, **bad))
        plain = {k: v for k, v in kw.items() if k not in ("num_beams", "num_return_sequences", "length_penalty", "early_stopping")}
        for bad, exc in (({"length_penalty": 2.0}, NotImplementedError), ({"num_return_sequences": 2}, NotImplementedError),
                         ({"early_stopping": True}, TypeError), ({"num_beams": 1, "early_stopping": True}, TypeError)):
            with pytest.raises(exc):
                model.generate(samples, **dict(plain, **bad))
    finally:
        model.train()
