"""Beam search in the decode slots on the device: mh_beam_topk_items / mh_beam_reorder_kv_items against their one-item forms and
torch, SlotDecoder.run(num_beams > 1) against LlamaHIP.beam_generate on each request alone (the beam-trap fixture and its
committed golden), and generate_stream / eval_aqa with beams on the model built from the reference's on-disk files."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from myriad_amd.decode_host import replay_slot_run  # noqa: E402
from myriad_amd.llama import LlamaHIP  # noqa: E402
from tests import beam_fixture as bf  # noqa: E402
from tests.test_decode_slots_gpu import _ragged_batches  # noqa: E402
from tests.test_entrypoints_gpu import DEV, _batch, fx, model  # noqa: E402,F401

GOLD = "tests/golden/beam_chain.npz"
F32, I32 = torch.float32, torch.int32
POISON_I = 0x7F7F7F7F


def _i32(v):
    return torch.tensor(v, dtype=I32).to(DEV)


# ------------------------------------------------------------------------------------------------ mh_beam_topk_items
def _topk_case(nb, G, V, seed, edge):
    """logits [G*nb, V] cut from a wider buffer, running scores, and an edge in the LAST item.  "tie": its rows 0 and 1 are one
    row (with -inf logits in it) under one score, and its other rows are far below, so every candidate ties across the two rows.
    "nan": its last row holds -inf and NaN logits; such a row never ranks (mh_beam_topk maps its NaN scores to -inf)."""
    g = torch.Generator().manual_seed(seed)
    R_ = G * nb
    buf = torch.randn(R_, V + 3, generator=g) * 3.0
    scores = -torch.rand(R_, generator=g) * 5.0
    r0 = (G - 1) * nb
    if edge == "tie":
        buf[r0, 5:9] = float("-inf")
        buf[r0 + 1] = buf[r0]
        scores[r0 + 2:r0 + nb] -= 20.0                               # the item's other rows never reach its top K ...
        scores[r0:r0 + 2] = -0.25                                    # ... which is K / 2 tied pairs of rows 0 and 1
    else:
        buf[r0 + nb - 1, 5:9] = float("-inf")
        buf[r0 + nb - 1, 17:19] = float("nan")
        scores[r0 + nb - 1] = 0.0                                    # the best running score of the item, and still it never ranks
    return buf.to(DEV)[:, :V], scores.to(DEV)


def _topk_items(logits, scores, nb, G, live, gen, prm):
    K, R_ = 2 * nb, G * nb
    out = torch.full((2, G * K), POISON_I, dtype=I32, device=DEV)
    part_s = torch.full((R_ * K,), -7.0, dtype=F32, device=DEV)
    part_i = torch.full((R_ * K,), POISON_I, dtype=I32, device=DEV)
    pos, kvlen = torch.arange(10, 10 + R_, dtype=I32).to(DEV), torch.arange(11, 11 + R_, dtype=I32).to(DEV)
    live_d, gen_d = _i32(live), _i32(gen)
    ops.beam_topk_items(logits, scores, part_s, part_i, out[0].view(F32), out[1], G, nb, live_d, gen_d, _i32(prm), pos, kvlen)
    torch.cuda.synchronize()
    return out, part_s, part_i, pos.cpu(), kvlen.cpu(), gen_d.cpu()


@pytest.mark.parametrize("edge", ["tie", "nan"])
@pytest.mark.parametrize("V", [1237, 32000])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("nb", [2, 4, 8])
def test_beam_topk_items_is_beam_topk_per_item(nb, G, V, edge):
    K, eos, min_length = 2 * nb, 3, 2
    logits, scores = _topk_case(nb, G, V, V + 10 * nb + G, edge)
    # G = 3: item 0 banned (gen < min_length), item 1 idle, item 2 not banned; G = 1: the item banned, then not, then idle
    runs = [([1, 0, 1], [0, 1, 5])] if G == 3 else [([1], [1]), ([1], [2]), ([0], [0])]
    for live, gen in runs:
        out, part_s, part_i, pos, kvlen, gen_after = _topk_items(logits, scores, nb, G, live, gen, [min_length, eos])
        for g in range(G):
            rows, rec = slice(g * nb, (g + 1) * nb), slice(g * K, (g + 1) * K)
            if not live[g]:                                          # its record is (0.0, -1) and nothing else of it moved
                assert out[0, rec].view(F32).tolist() == [0.0] * K and out[1, rec].tolist() == [-1] * K
                assert pos[rows].tolist() == list(range(10 + g * nb, 10 + (g + 1) * nb))
                assert kvlen[rows].tolist() == list(range(11 + g * nb, 11 + (g + 1) * nb)) and int(gen_after[g]) == gen[g]
                assert bool((part_s[g * nb * K:(g + 1) * nb * K] == -7.0).all())
                assert bool((part_i[g * nb * K:(g + 1) * nb * K] == POISON_I).all())
                continue
            ban = eos if gen[g] < min_length else -1
            want = torch.full((2, K), POISON_I, dtype=I32, device=DEV)
            ops.beam_topk(logits[rows], scores[rows].clone(), torch.empty(nb * K, dtype=F32, device=DEV),
                          torch.empty(nb * K, dtype=I32, device=DEV), want[0].view(F32), want[1], 1, nb, ban_id=ban)
            assert torch.equal(out[:, rec], want), (g, out[:, rec], want)              # bits, scores and flat indices
            if ban >= 0:
                assert not bool((out[1, rec] % V == eos).any())
            assert pos[rows].tolist() == list(range(11 + g * nb, 11 + (g + 1) * nb))
            assert kvlen[rows].tolist() == list(range(12 + g * nb, 12 + (g + 1) * nb)) and int(gen_after[g]) == gen[g] + 1
        if live[G - 1]:
            rec = slice((G - 1) * K, G * K)
            s, i = out[0, rec].view(F32).cpu(), out[1, rec].cpu()
            assert not bool(torch.isnan(s).any()) and bool(torch.isfinite(s).all())
            if edge == "tie":                                        # every pair comes out row 0 first: the lower flat index
                assert torch.equal(s[0::2], s[1::2]) and bool((i[0::2] < V).all()) and torch.equal(i[1::2], i[0::2] + V), (s, i)
                assert not any(5 <= int(t) % V < 9 for t in i)       # no -inf id is picked
            else:                                                    # no flat index of the NaN row in the record
                assert not bool((i // V == nb - 1).any()), i


def test_beam_topk_items_refusals():
    nb, G, V = 2, 2, 64
    K, R_ = 2 * nb, G * nb

    def args(**kw):
        a = dict(logits=torch.randn(R_, V, device=DEV), scores=torch.zeros(R_, device=DEV),
                 part_s=torch.empty(R_ * K, device=DEV), part_i=torch.empty(R_ * K, dtype=I32, device=DEV),
                 out_s=torch.empty(G * K, device=DEV), out_i=torch.empty(G * K, dtype=I32, device=DEV), G=G, nb=nb,
                 live=_i32([1] * G), gen=_i32([0] * G), prm=_i32([1, 2]), pos=_i32([3] * R_), kvlen=_i32([4] * R_))
        a.update(kw)
        return a

    ops.beam_topk_items(**args())                                    # the baseline call is fine
    bad = [dict(G=3), dict(nb=4), dict(live=_i32([1])), dict(gen=_i32([0])), dict(prm=_i32([1])), dict(pos=None), dict(kvlen=None),
           dict(pos=_i32([3] * (R_ - 1))), dict(live=torch.ones(G, device=DEV)), dict(gen=torch.zeros(G, dtype=torch.long, device=DEV)),
           dict(scores=torch.zeros(R_ - 1, device=DEV)), dict(part_s=torch.empty(R_ * K - 1, device=DEV)),
           dict(out_i=torch.empty(G * K - 1, dtype=I32, device=DEV)), dict(live=torch.ones(G, dtype=I32)),
           dict(logits=torch.randn(R_, V, device=DEV).double())]
    for kw in bad:
        with pytest.raises((_lib.MyriadHipError, ValueError, TypeError)):
            ops.beam_topk_items(**args(**kw))
    # the library's own limits, made before any launch: more than 8 beams, a vocabulary under 2 * nb or over 32768
    for nb_, V_ in ((9, 64), (4, 7), (2, 32769)):
        R2, K2 = 2 * nb_, 2 * nb_
        with pytest.raises(_lib.MyriadHipError, match="UNSUPPORTED"):
            ops.beam_topk_items(torch.randn(R2, V_, device=DEV), torch.zeros(R2, device=DEV), torch.empty(R2 * K2, device=DEV),
                                torch.empty(R2 * K2, dtype=I32, device=DEV), torch.empty(2 * K2, device=DEV),
                                torch.empty(2 * K2, dtype=I32, device=DEV), 2, nb_, _i32([1, 1]), _i32([0, 0]), _i32([1, 2]),
                                _i32([3] * R2), _i32([4] * R2))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ mh_beam_reorder_kv_items
@pytest.mark.parametrize("nb,G,C", [(4, 2, 128), (2, 3, 64), (8, 2, 8192)])
def test_beam_reorder_kv_items_matches_index_select_per_item(nb, G, C):
    L, T = 2, 64
    g = torch.Generator().manual_seed(nb * 100 + C)
    caches = [torch.randn(G * nb, T, C, generator=g).to(torch.bfloat16).to(DEV) for _ in range(L)]      # every cell a canary
    table = torch.tensor([c.data_ptr() for c in caches], dtype=torch.long).to(DEV)
    # item 0: duplicate parents (all from its row 0, one row naming a row OUTSIDE the item: ignored); others: reversed
    src = []
    for b in range(G):
        par = [0] * nb if b == 0 else [nb - 1 - j for j in range(nb)]
        src += [b * nb + p for p in par]
    src[nb - 1] = (nb + 1) % (G * nb) if G * nb > nb + 1 else -1     # out of item 0
    assert not 0 <= src[nb - 1] < nb
    eff = [s if r // nb * nb <= s < r // nb * nb + nb else r for r, s in enumerate(src)]
    src_t, eff_t = _i32(src), torch.tensor(eff, dtype=torch.long).to(DEV)
    launches = [  # (lo, hi, live) per item; a third item takes the last column
        ([5, 13, 60], [41, 13, 64], [1, 1, 1]),                      # lo % 4 != 0; empty; hi == T_cap
        ([0, 0, 3], [200, 64, 7], [1, 0, 1]),                        # hi > T_cap is clamped; an idle item; a short window
        ([61, -3, 62], [64, 9, 999], [1, 1, 1]),                     # hi == T_cap; lo < 0 is clamped; both ends
    ]
    for lo, hi, live in launches:
        lo, hi, live = lo[:G], hi[:G], live[:G]
        before = [c.clone() for c in caches]
        ops.beam_reorder_kv_items(table, L, G, nb, T, C, src_t, _i32(lo), _i32(hi), _i32(live))
        torch.cuda.synchronize()
        for c, c0 in zip(caches, before):
            want = c0.clone()
            moved = c0.index_select(0, eff_t)
            for b in range(G):
                if live[b]:
                    a, e = max(lo[b], 0), min(hi[b], T)
                    want[b * nb:(b + 1) * nb, a:e] = moved[b * nb:(b + 1) * nb, a:e]
            assert torch.equal(c.view(torch.int16), want.view(torch.int16))          # bits, everything outside the windows included
    for kw in (dict(lo=_i32([0])), dict(live=_i32([1])), dict(hi=torch.zeros(G, device=DEV)), dict(src=_i32([0] * (G * nb - 1)))):
        a = dict(src=src_t, lo=_i32([0] * G), hi=_i32([1] * G), live=_i32([1] * G))
        a.update(kw)
        with pytest.raises(_lib.MyriadHipError):
            ops.beam_reorder_kv_items(table, L, G, nb, T, C, a["src"], a["lo"], a["hi"], a["live"])
    with pytest.raises(_lib.MyriadHipError, match="UNSUPPORTED"):
        ops.beam_reorder_kv_items(table, L, G, nb, T, C + 4, src_t, _i32([0] * G), _i32([1] * G), _i32([1] * G))


# ------------------------------------------------------------------------------------------------ SlotDecoder.run(num_beams)
KW = dict(max_new_tokens=bf.MAX_NEW, stop_ids=bf.STOPS, eos_id=bf.EOS, min_length=bf.MIN_LENGTH)
NOISE = [0, 10, 3, 7, 1, 5, 2]


@pytest.fixture(scope="module")
def trap():
    lm = LlamaHIP(bf.weights(), bf.BEAM_TRAP["heads"], DEV, need_backward=False)
    lm.slot_beams = True
    return lm


def _ragged(n=7):
    """request i: fixture row i % 3 behind NOISE[i] rows of noise, so the prompts differ in length"""
    g = torch.Generator().manual_seed(41)
    rows = bf.inputs([0, 1, 2])
    return [torch.cat([torch.randn(NOISE[i], rows.shape[2], generator=g) * 0.3, rows[i % 3]], 0).to(DEV) for i in range(n)]


@pytest.fixture(scope="module")
def alone(trap):
    """beam_generate on each ragged request alone, computed once: (ids, scores, lengths, steps) per (request, knobs)"""
    memo = {}

    def get(reqs, i, nb=2, nrs=2, lp=1.0, es=False, min_length=bf.MIN_LENGTH):
        key = (i, nb, nrs, lp, es, min_length)
        if key not in memo:
            ids, sc = trap.beam_generate(reqs[i][None], nb, length_penalty=lp, early_stopping=es, num_return_sequences=nrs,
                                         return_scores=True, **dict(KW, min_length=min_length))
            st = trap.last_generate_stats
            memo[key] = (ids, sc, list(st["lengths"]), st["steps"])
        return memo[key]
    return get


def _same(got, want, bits=True):
    _, ids, sc, lengths = got
    assert ids.dtype == torch.long and torch.equal(ids, want[0]), (ids, want[0])
    assert lengths == want[2]
    if bits:
        assert torch.equal(sc, want[1]), (sc, want[1])
    else:
        assert float((sc - want[1]).abs().max()) < 2e-2


@pytest.mark.parametrize("nb,rows", [(2, [0, 1]), (4, [0])])
def test_slot_beams_return_the_golden_ids_and_beam_generates_bits(trap, nb, rows):
    gold = np.load(GOLD)
    reqs = [bf.inputs([r])[0].to(DEV) for r in rows]
    dec = trap.slot_decoder(4, 64)
    outs = sorted(dec.run(reqs, num_beams=nb, num_return_sequences=2, **KW), key=lambda o: o[0])
    assert [o[0] for o in outs] == list(range(len(rows)))
    assert outs[0][1].tolist() == gold[f"b1_nb{nb}_ids"].tolist()
    assert np.abs(outs[0][2].numpy() - gold[f"b1_nb{nb}_scores"]).max() < 2e-2
    st = dict(dec.last_stats)
    assert st["num_beams"] == nb and st["groups"] == 4 // nb and st["finished_hypotheses"] >= 2 * len(rows)
    for o, x in zip(outs, reqs):                                     # ids, lengths and scores: bit for bit
        ids, sc = trap.beam_generate(x[None], nb, num_return_sequences=2, return_scores=True, **KW)
        _same(o, (ids, sc, list(trap.last_generate_stats["lengths"])))


def test_refills_ragged_prompts_and_host_only_knobs(trap, alone):
    reqs = _ragged()
    dec = trap.slot_decoder(4, 64)
    outs = list(dec.run(reqs, num_beams=2, num_return_sequences=2, **KW))
    st = dict(dec.last_stats)
    assert sorted(o[0] for o in outs) == list(range(7))              # no request is left out
    for o in outs:
        _same(o, alone(reqs, o[0]), bits=False)
    assert st["graph_captures"] == 1 and st["prefills"] == 7 and st["graph_replays"] > 0
    steps = [alone(reqs, i)[3] for i in range(7)]
    pred = replay_slot_run([int(x.shape[0]) for x in reqs], [[0] * (n - 1) + [bf.EOS] for n in steps], 2, 10 ** 6, (), bf.EOS)
    assert (st["steps"], st["live_row_steps"], st["occupancy"]) == (pred["steps"], pred["live_row_steps"], pred["occupancy"])
    assert st["prefill_passes"] == 7 and st["packed_rows"] == sum(int(x.shape[0]) for x in reqs)
    # isolation: a request alone in the decoder, on stale cache rows, is what it was among six others
    (solo,) = list(dec.run([reqs[3]], num_beams=2, num_return_sequences=2, **KW))
    among = next(o for o in outs if o[0] == 3)
    assert torch.equal(solo[1], among[1]) and torch.equal(solo[2], among[2]) and solo[3] == among[3]
    # the knobs live on the host or in device memory: other values replay the graph captured above
    kw2 = dict(KW, min_length=3)
    outs2 = list(dec.run(reqs, num_beams=2, num_return_sequences=1, length_penalty=0.0, early_stopping=True, ordered=True, **kw2))
    assert [o[0] for o in outs2] == list(range(7))
    for o in outs2:
        _same(o, alone(reqs, o[0], nrs=1, lp=0.0, es=True, min_length=3), bits=False)
    assert dec.last_stats["graph_captures"] == 1 and dec.last_stats["graph_replays"] == dec.last_stats["steps"]
    assert any(not torch.equal(a[1][:1], b[1]) for a, b in zip(sorted(outs, key=lambda o: o[0]), outs2))     # the knobs mattered
    # packed prefill: the same ids (its GEMM plans differ, so not required bitwise)
    outs3 = list(dec.run(reqs, num_beams=2, num_return_sequences=2, prefill_batch=2, ordered=True, **KW))
    assert dec.last_stats["prefill_passes"] < 7 and dec.last_stats["prefills"] == 7
    for o in outs3:
        assert torch.equal(o[1], alone(reqs, o[0])[0]) and o[3] == alone(reqs, o[0])[2]


def test_an_idle_group_and_pad_id(trap, alone):
    reqs = _ragged(2)
    dec = trap.slot_decoder(6, 64)                                   # three groups, two requests: group 2 is idle throughout
    outs = list(dec.run(reqs, num_beams=2, num_return_sequences=2, ordered=True, pad_id=0, **KW))
    assert [o[0] for o in outs] == [0, 1] and dec.last_stats["groups"] == 3 and dec.last_stats["occupancy"] <= 2 / 3
    for o in outs:
        want = alone(reqs, o[0])
        ids = want[0].clone()
        for r, n in enumerate(want[2]):
            ids[r, n:] = 0
        _same(o, (ids, want[1], want[2]), bits=False)


def test_slot_beam_refusals(trap):
    reqs = _ragged(2)
    dec = trap.slot_decoder(4, 64)
    trap.slot_beams = False
    try:
        with pytest.raises(NotImplementedError, match="MYRIAD_SLOT_BEAMS"):
            list(dec.run(reqs, num_beams=2, **KW))
    finally:
        trap.slot_beams = True
    for bad, exc in ((dict(num_beams=3), ValueError), (dict(num_beams=0), ValueError), (dict(num_beams=9), NotImplementedError),
                     (dict(num_beams=2, do_sample=True), NotImplementedError),
                     (dict(num_beams=2, repetition_penalty=1.2), NotImplementedError),
                     (dict(num_beams=2, return_scores=True), NotImplementedError),
                     (dict(num_beams=2, seeds=[1, 2]), NotImplementedError),
                     (dict(num_beams=2, num_return_sequences=3), ValueError),
                     (dict(num_beams=2, early_stopping="sometimes"), ValueError)):
        with pytest.raises(exc):
            list(dec.run(reqs, **dict(KW, **bad)))
    with pytest.raises(NotImplementedError):
        dec.run_turns([("a", reqs[0], list(range(reqs[0].shape[0])))], num_beams=2)
    with pytest.raises(ValueError):                                  # a request that does not fit a slot
        list(dec.run([torch.zeros(60, reqs[0].shape[1], device=DEV)], num_beams=2, **KW))
    assert [o[0] for o in dec.run(reqs, num_beams=2, ordered=True, **KW)] == [0, 1]      # and the decoder still serves


# ------------------------------------------------------------------------------------------------ the model and the eval entry
NEAR_TIE = 2e-2                                                      # what tests/test_beam_gpu.py holds the device's beam scores to


def _oracle_min_gap(sd, x, kw):
    """The CPU oracle's beam search on one sample's prompt embeddings x [S0, D]: the smallest gap between neighbours among every
    step's top K + 1 candidates and among the finished pool's scores.  Two correct device runs whose scores differ by rounding
    can order candidates differently only where such a gap is small."""
    from oracle import myriad_ref as R
    from tests import beam_ref
    emb = sd["llama_model.model.embed_tokens.weight"]

    def fn(prefixes):
        rows = []
        for _, seq in prefixes:
            e = torch.cat([x, emb[list(seq)]], 0) if seq else x
            rows.append(R.llama_causal_lm(sd, e[None], torch.ones(1, e.shape[0]), None, 32)[1][0, -1].float())
        return torch.stack(rows)

    _, _, tr = beam_ref.beam_search(fn, 1, kw["num_beams"], kw["max_new_tokens"], 2, min_length=kw["min_length"],
                                    num_return_sequences=kw["num_return_sequences"], stop_seqs=kw["stop_ids"], return_trace=True)
    gap = float("inf")
    for v in [s[0] for s, _ in tr["trace"]] + [tr["pool"][0]]:
        v = v[v > -1e8]
        if v.numel() > 1:
            gap = min(gap, float((v[:-1] - v[1:]).min()))
    return gap


def test_generate_stream_with_beams_matches_generate_per_sample(model, fx):
    """generate_stream(slots=4, num_beams=2, num_return_sequences=2) against generate() per sample, hypothesis by hypothesis.
    The two sides run the token step at 4 and at 2 rows, and on this fixture (random weights, nearly flat logits) their
    sequence scores differ by rounding (measured over twelve seeds of the batches: 2e-4 to 5e-3), so a sample may differ only
    where the CPU oracle shows a near tie (a gap under NEAR_TIE between neighbouring candidates or pool scores), and at most
    one of the five may.  Seed 3 was chosen from that measurement: all five samples came out equal (as for seeds 1, 4, 6, 9
    to 12; seeds 2, 5, 7 and 8 each had one sample whose two hypotheses swapped at oracle gaps of 1.3e-3 to 1.5e-2)."""
    model.eval()
    prev = getattr(model.llama, "slot_beams", False)
    try:
        batches = _ragged_batches(model, (2, 3), seed=3)
        assert len({len(b) for bt in batches for b in bt["before_ids"]}) > 1
        kw = dict(max_new_tokens=8, stop_ids=((835,), (2277, 29937)), min_length=1, num_beams=2, num_return_sequences=2)
        model.llama.slot_beams = False
        with pytest.raises(NotImplementedError, match="MYRIAD_SLOT_BEAMS"):
            model.generate_stream(iter(batches), slots=4, **kw)
        model.llama.slot_beams = True
        outs = list(model.generate_stream(iter(batches), slots=4, **kw))
        assert [o["index"] for o in outs] == [0, 1, 2, 3, 4]
        st = model.last_generate_stats
        assert st["prefills"] == 5 and st["num_beams"] == 2 and 0 < st["occupancy"] <= 1
        k, excluded = 0, []
        for bt in batches:
            for i in range(bt["image"].shape[0]):
                one = dict(image=bt["image"][i:i + 1], anomaly_maps=bt["anomaly_maps"][i:i + 1],
                           before_ids=bt["before_ids"][i][None], after_ids=bt["after_ids"][i][None])
                ref = model.generate(one, **kw)
                ids, want = outs[k]["token_ids"], ref["token_ids"].cpu()
                assert ids.dtype == torch.long and ids.dim() == 2 and ids.shape[0] == 2
                assert torch.equal(outs[k]["ve_anomaly_map"], ref["ve_anomaly_maps"][0])
                if torch.equal(ids, want):
                    assert float((outs[k]["sequences_scores"] - model.last_generate_stats["sequences_scores"]).abs().max()) < 2e-2
                else:                                                # only a near tie of the oracle excuses a difference
                    with torch.no_grad():
                        parts = model.encode_img(one["image"].to(DEV, torch.float32), one["anomaly_maps"].to(DEV, torch.float32), 1, False)
                        x = model._assemble(parts, one["before_ids"], one["after_ids"], None, None)[0][0, 1:].contiguous().cpu()
                    gap = _oracle_min_gap(fx["sd"], x, kw)
                    print(f"sample {k}: hypotheses differ, oracle's smallest gap {gap:.3e}")
                    assert gap < NEAR_TIE, (k, ids, want, gap)
                    excluded.append(k)
                k += 1
        assert len(excluded) <= 1, excluded
        one_seq = list(model.generate_stream(iter(batches[:1]), slots=4, **dict(kw, num_return_sequences=1)))
        assert all(o["token_ids"].dim() == 1 and o["sequences_scores"].shape == (1,) for o in one_seq)
        if 0 not in excluded:
            assert torch.equal(one_seq[0]["token_ids"], outs[0]["token_ids"][0][:one_seq[0]["token_ids"].shape[0]])
        for bad, exc in ((dict(repetition_penalty=1.2), NotImplementedError), (dict(do_sample=True), NotImplementedError),
                         (dict(num_beams=3), ValueError)):
            with pytest.raises(exc):
                model.generate_stream(iter(batches), slots=4, **dict(kw, **bad))
        with pytest.raises(NotImplementedError):
            model.generate_stream(iter(batches), slots=4, seeds=[1, 2, 3, 4, 5], **kw)
    finally:
        model.llama.slot_beams = prev
        model.train()


def test_eval_entry_point_takes_num_beams_in_the_slots(fx, tmp_path, monkeypatch):
    import eval_aqa
    monkeypatch.setenv("MYRIAD_SLOT_BEAMS", "1")
    rows = {}
    for slots in (0, 4):
        res = str(tmp_path / f"res{slots}.jsonl")
        path, records = eval_aqa.main(["--cfg-path", fx["eval_yaml"], "--dataset", "synthetic", "--bs", "2", "--limit", "2",
                                       "--slots", str(slots), "--num-beams", "2", "--out", res])
        rows[slots] = [json.loads(l) for l in open(path)]
        assert len(rows[slots]) == len(records) == 4                 # one record per sample
    assert [r["image_id"] for r in rows[4]] == [r["image_id"] for r in rows[0]]          # the dataset's order
    assert [r["image_path"] for r in rows[4]] == [r["image_path"] for r in rows[0]]
    assert all(set(a) == set(b) for a, b in zip(rows[4], rows[0]))
