"""Beam sampling and the repetition penalty in the decode slots' beam groups on the device: mh_beam_sample_topk_items /
mh_beam_seen_update_items against their batch forms at B = 1 bit for bit (every output a window inside a poisoned buffer),
SlotDecoder.run(num_beams > 1, do_sample / repetition_penalty / seeds) against LlamaHIP.beam_generate on each request alone (the
beam-trap fixture, and the flat llama_tiny model where the noise and the seen bitmaps decide every request's answer), and
generate_stream / eval_aqa with sampled beams on the tiny model of tests/test_entrypoints_gpu.py."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, decode, ops  # noqa: E402
from myriad_amd.decode_host import beam_sample_select  # noqa: E402
from myriad_amd.llama import LlamaHIP  # noqa: E402
from tests import beam_fixture as bf  # noqa: E402
from tests import beam_sample_ref as BR  # noqa: E402
from tests.fp64_bounds import assert_frame_untouched, assert_untouched, poisoned, untouched  # noqa: E402
from tests.test_decode_slots_gpu import _ragged_batches, _requests  # noqa: E402
from tests.test_sampling_gpu import _tiny  # noqa: E402
from tests.test_slot_beams_gpu import NEAR_TIE  # noqa: E402
from tests.test_entrypoints_gpu import DEV, fx, model  # noqa: E402,F401

F32, I32 = torch.float32, torch.int32
PAD = 8
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
EOS_K, MIN_LEN_K = 3, 2                                              # the kernel tests' (eos_id, min_length)


def _win(n, dtype):
    """(buffer, window): n contiguous elements inside a poisoned [1, n + 2 PAD] buffer."""
    buf = poisoned((1, n + 2 * PAD), dtype, DEV)
    return buf, buf[0, PAD:PAD + n]


def _buffers(G, nb):
    R, K = G * nb, 2 * nb
    return dict(part_k=_win(R * K, F32), part_a=_win(R * K, F32), part_i=_win(R * K, I32), part_f=_win(R, I32),
                out_s=_win(G * K, F32), out_i=_win(G * K, I32), out_f=_win(G, I32), out_k=_win(G * K, F32))


def _i32(v):
    return torch.tensor(v, dtype=I32).to(DEV)


def _i64(v):
    return torch.tensor(v, dtype=torch.long).to(DEV)


def _prm(inv_temp, top_p, top_k, penalty):
    return torch.tensor([inv_temp, top_p, float(top_k), penalty], dtype=F32).to(DEV)


def _bits(t):
    return t.view(I32) if t.dtype == F32 else t


def _items(logits, scores, G, nb, live, gen, seeds, prm, seen=None, draw=True, t_add=0, advance=True):
    """One ops.beam_sample_topk_items into bordered windows: the windows (device), and pos / kvlen / gen after it."""
    R = G * nb
    wins = _buffers(G, nb)
    w = {k: v[1] for k, v in wins.items()}
    pos, kvlen = torch.arange(10, 10 + R, dtype=I32).to(DEV), torch.arange(11, 11 + R, dtype=I32).to(DEV)
    gen_d = _i32(gen)
    adv = dict(pos=pos, kvlen=kvlen) if advance else {}
    ops.beam_sample_topk_items(logits, scores, w["part_k"], w["part_a"], w["part_i"], w["part_f"], w["out_s"], w["out_i"], w["out_f"],
                               G, nb, _i32(live), gen_d, _i32([MIN_LEN_K, EOS_K]), draw=draw, params=prm, seed=_i64(seeds), seen=seen,
                               t_add=t_add, out_k=w["out_k"], **adv)
    torch.cuda.synchronize()
    for name, (buf, win) in wins.items():
        assert_frame_untouched(buf, slice(0, 1), slice(PAD, PAD + win.numel()), name)
    return w, pos.cpu(), kvlen.cpu(), gen_d.cpu()


def _batch_form(logits, scores, nb, seed, prm, ban, t, seen=None, draw=True):
    """ops.beam_sample_topk at B = 1 on one group's rows with step = None and t_add = t: (acc, flat, flag, key) on the device."""
    K = 2 * nb
    w = {k: v[1] for k, v in _buffers(1, nb).items()}
    ops.beam_sample_topk(logits, scores, w["part_k"], w["part_a"], w["part_i"], w["part_f"], w["out_s"], w["out_i"], w["out_f"], 1, nb,
                         ban_id=ban, draw=draw, params=prm, seed=_i64([seed]), seen=seen, t_add=t, out_k=w["out_k"])
    torch.cuda.synchronize()
    assert w["out_s"].numel() == K
    return w["out_s"], w["out_i"], w["out_f"], w["out_k"]


def _case(V, nb, G, seed):
    """logits [G * nb, V] cut from a wider NaN-padded buffer, running scores and seen-id bitmaps (EOS_K among the seen ids)."""
    g = torch.Generator().manual_seed(seed)
    R = G * nb
    host = torch.full((R, V + 4), float("nan"), dtype=F32)
    host[:, :V] = torch.randn(R, V, generator=g) * 2.0
    scores = -torch.rand(R, generator=g) * 3.0
    seen_ids = [[int(i) for i in torch.randint(0, V, (5,), generator=g)] + [EOS_K] for _ in range(R)]
    return host.to(DEV)[:, :V], scores.to(DEV), BR.seen_bitmap(seen_ids, V).to(DEV)


def _check_idle(w, g, nb, what):
    K = 2 * nb
    rec, rows = slice(g * K, (g + 1) * K), slice(g * nb * K, (g + 1) * nb * K)
    assert w["out_s"][rec].tolist() == [0.0] * K and w["out_i"][rec].tolist() == [-1] * K and int(w["out_f"][g]) == 0, what
    for name in ("part_k", "part_a", "part_i"):                     # its scratch rows and its keys: nothing wrote them
        assert bool(untouched(w[name][rows]).all()), (what, name)
    assert bool(untouched(w["part_f"][g * nb:(g + 1) * nb]).all()) and bool(untouched(w["out_k"][rec]).all()), what


# ------------------------------------------------------------------------------------------------ mh_beam_sample_topk_items
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("nb", [2, 4, 8])
@pytest.mark.parametrize("V", [36, 4100, 32000])
def test_items_form_is_the_batch_form_per_group_bit_for_bit(V, nb, G):
    """Group g with seed s_g and gen[g] = t records what mh_beam_sample_topk records at B = 1 on its rows with that seed, step =
    null and t_add = t, with the ban decided by gen[g] < min_length: draw on and off, with and without bitmaps and a penalty.  An
    idle group is inert, a live one advances exactly its own rows and its own gen."""
    K = 2 * nb
    logits, scores, bitmap = _case(V, nb, G, 7 * V + 10 * nb + G)
    # G = 3: group 0 banned (gen < min_length), group 1 idle, group 2 not banned; G = 1: banned, then not, then idle
    runs = [([1, 0, 1], [0, 7, 5])] if G == 3 else [([1], [1]), ([1], [4]), ([0], [3])]
    seeds = [991 + (1 << 40), 17, (1 << 62) + 5][:G]
    for live, gen in runs:
        for draw in (True, False):
            for seen, prm in ((None, _prm(1.0 / 0.7, 0.9, 50, 1.0)), (bitmap, _prm(1.0 / 0.7, 0.9, 50, 1.3))):
                what = f"V={V} nb={nb} live={live} gen={gen} draw={draw} seen={seen is not None}"
                w, pos, kvlen, gen_after = _items(logits, scores, G, nb, live, gen, seeds, prm, seen=seen, draw=draw)
                for g in range(G):
                    rows, rec = slice(g * nb, (g + 1) * nb), slice(g * K, (g + 1) * K)
                    before = (list(range(10 + g * nb, 10 + (g + 1) * nb)), list(range(11 + g * nb, 11 + (g + 1) * nb)))
                    if not live[g]:
                        _check_idle(w, g, nb, what)
                        assert (pos[rows].tolist(), kvlen[rows].tolist()) == before and int(gen_after[g]) == gen[g], what
                        continue
                    ban = EOS_K if gen[g] < MIN_LEN_K else -1
                    acc, flat, flag, key = _batch_form(logits[rows], scores[rows].clone(), nb, seeds[g], prm, ban, gen[g],
                                                       seen=None if seen is None else seen[rows].clone(), draw=draw)
                    assert torch.equal(_bits(w["out_s"][rec]), _bits(acc)), (what, g, w["out_s"][rec], acc)
                    assert torch.equal(w["out_i"][rec], flat), (what, g, w["out_i"][rec], flat)
                    assert torch.equal(_bits(w["out_k"][rec]), _bits(key)), (what, g)
                    assert int(w["out_f"][g]) == int(flag[0]) == 0, what
                    if ban >= 0:
                        assert not bool((w["out_i"][rec] % V == EOS_K).any()), what
                    for name in ("part_k", "part_a", "part_i"):
                        assert not bool(untouched(w[name][g * nb * K:(g + 1) * nb * K]).any()), (what, name)
                    assert pos[rows].tolist() == [p + 1 for p in before[0]] and kvlen[rows].tolist() == [p + 1 for p in before[1]], what
                    assert int(gen_after[g]) == gen[g] + 1, what
    # without pos / kvlen (a refill's first pick) the record is the same and nothing advances, gen included
    live, gen = runs[0]
    prm = _prm(1.0, 0.95, 40, 1.0)
    w, _, _, _ = _items(logits, scores, G, nb, live, gen, seeds, prm)
    w2, pos, kvlen, gen_after = _items(logits, scores, G, nb, live, gen, seeds, prm, advance=False)
    assert all(torch.equal(_bits(w[k]), _bits(w2[k])) for k in ("out_s", "out_i", "out_f"))
    assert pos.tolist() == list(range(10, 10 + G * nb)) and kvlen.tolist() == list(range(11, 11 + G * nb)) and gen_after.tolist() == gen


def test_a_groups_place_does_not_change_its_draws():
    """The same rows, seed and gen in group 0 and in group 2: identical records (the counter's item field is fixed), and another
    seed or another gen draws something else."""
    V, nb, G = 4100, 4, 3
    K = 2 * nb
    logits, scores, _ = _case(V, nb, G, 5)
    logits, scores = logits.clone(), scores.clone()
    logits[2 * nb:] = logits[:nb]
    scores[2 * nb:] = scores[:nb]
    prm = _prm(1.0, 1.0, 50, 1.0)
    w, _, _, _ = _items(logits, scores, G, nb, [1, 1, 1], [4, 4, 4], [77, 78, 77], prm)
    first, last = slice(0, K), slice(2 * K, 3 * K)
    for name in ("out_s", "out_i", "out_k"):
        assert torch.equal(_bits(w[name][first]), _bits(w[name][last])), name
    w2, _, _, _ = _items(logits, scores, G, nb, [1, 1, 1], [4, 4, 5], [77, 78, 78], prm)
    assert torch.equal(w2["out_i"][first], w["out_i"][first])
    assert not torch.equal(w2["out_i"][last], w["out_i"][last])              # flat logits scale: another stream, another draw
    w3, _, _, _ = _items(logits, scores, G, nb, [1, 1, 1], [4, 4, 4], [77, 78, 77], prm, t_add=1)
    w4, _, _, _ = _items(logits, scores, G, nb, [1, 1, 1], [5, 5, 5], [77, 78, 77], prm)
    assert torch.equal(w3["out_i"], w4["out_i"])                              # the Philox step is gen[g] + t_add


def test_a_tie_past_the_cap_flags_its_group_only_and_the_host_redoes_it():
    V, nb, G = 4100, 2, 3
    logits, scores, _ = _case(V, nb, G, 77)
    x = logits.cpu().clone()
    x[3, :] = -4.0
    x[3, 100:1600] = 1.0                                             # 1500 tokens tied at what becomes the k-th value ...
    x[3, 2000:2010] = torch.arange(10).float() * 0.25 + 2.0          # ... below ten distinct ones
    seeds, gen, top_k, top_p, inv_temp = [5, 991, 6], [2, 5, 3], 50, 0.9, float(np.float32(1.0 / 0.7))
    w, _, _, _ = _items(x.to(DEV), scores, G, nb, [1, 1, 1], gen, seeds, _prm(inv_temp, top_p, top_k, 1.0))
    assert w["out_f"].tolist() == [0, 1, 0]
    flat = w["out_i"][2 * nb:4 * nb].tolist()
    assert all(0 <= f < nb * V for f in flat) and len(set(flat)) == 2 * nb           # valid indices all the same
    # the host's rule with the group's own seed, its t = gen[g] and item 0 is the rule of the group alone (B = 1, item 0)
    sc = scores[2:4].cpu()
    ref = BR.step(x[2:4], sc, [[]] * nb, 1, nb, -1, inv_temp, top_k, top_p, 1.0, seeds[1], gen[1])[0]
    h_acc, h_flat, h_key = beam_sample_select(x[2:4].numpy(), sc.numpy(), [[], []], -1, inv_temp, top_k, top_p, 1.0, seeds[1], gen[1], 0)
    assert h_flat.tolist() == ref.sel_flat
    tol = lambda r: BR.TOL * np.maximum(1.0, np.abs(np.asarray(r, dtype=np.float64)))         # noqa: E731
    assert np.all(np.abs(h_acc - np.array(ref.sel_acc)) <= tol(ref.sel_acc))
    assert np.all(np.abs(h_key - np.array(ref.sel_key)) <= tol(ref.sel_key))


# ------------------------------------------------------------------------------------------------ mh_beam_seen_update_items
@pytest.mark.parametrize("V", [36, 32000])
@pytest.mark.parametrize("nb", [2, 8])
def test_seen_update_items_follows_the_parents_of_live_groups_only(nb, V):
    G, W = 3, (V + 31) // 32
    R = G * nb
    g = torch.Generator().manual_seed(nb * V + 1)
    old = torch.randint(-2**31, 2**31 - 1, (R, W), generator=g, dtype=torch.long).to(I32)
    # group 0: a reversal with one parent OUTSIDE the group (ignored); group 1: idle, with parents that would move its rows;
    # group 2: everything from one row
    src = list(range(nb))[::-1] + [nb + (nb - 1 - j) for j in range(nb)] + [2 * nb + (nb - 1)] * nb
    src[0] = nb + 1
    ids = torch.randint(0, V, (R,), generator=g)
    ids[1], ids[R - 1] = -1, V + 5                                   # no bit for an id outside the vocabulary
    live = [1, 0, 1]
    buf, win = _win(R * W, I32)
    win.copy_(old.reshape(-1).to(DEV))
    ops.beam_seen_update_items(win, _i32(src), ids.to(DEV), G, nb, V, _i32(live))
    ref_buf, ref = _win(R * W, I32)
    ref.copy_(old.reshape(-1).to(DEV))
    ops.beam_seen_update(ref, _i32(src), ids.to(DEV), G, nb, V)
    torch.cuda.synchronize()
    assert_frame_untouched(buf, slice(0, 1), slice(PAD, PAD + R * W), "seen")
    got, want = win.cpu().view(R, W), ref.cpu().view(R, W)
    for b in range(G):
        rows = slice(b * nb, (b + 1) * nb)
        assert torch.equal(got[rows], want[rows] if live[b] else old[rows]), b
    o = old.numpy().view(np.uint32)
    row0 = o[0].copy()                                               # row 0's parent is outside its group: it keeps its own word
    row0[int(ids[0]) >> 5] |= np.uint32(1) << np.uint32(int(ids[0]) & 31)
    assert np.array_equal(got[0].numpy().view(np.uint32), row0)


# ------------------------------------------------------------------------------------------------ refusals
def test_items_launchers_refuse_bad_arguments_before_any_launch():
    G, nb, V = 2, 2, 64
    R, K = G * nb, 2 * nb
    L = _lib.load()
    logits = torch.randn(R, V, device=DEV)
    scores = torch.zeros(R, device=DEV)
    seen_buf, seen = _win(R * 2, I32)
    wins = _buffers(G, nb)
    w = {k: v[1].data_ptr() for k, v in wins.items()}
    prm, seed = _prm(1.0, 0.9, 50, 1.2), _i64([3, 4])
    live, gen, bprm = _i32([1, 1]), _i32([4, 4]), _i32([1, 2])
    pbuf, pos = _win(R, I32)
    pos.fill_(4)
    good = [logits.data_ptr(), V, scores.data_ptr(), seen.data_ptr(), w["part_k"], w["part_a"], w["part_i"], w["part_f"], w["out_s"],
            w["out_i"], w["out_f"], w["out_k"], G, nb, V, 1, prm.data_ptr(), seed.data_ptr(), live.data_ptr(), gen.data_ptr(),
            bprm.data_ptr(), 0, pos.data_ptr(), pos.data_ptr(), None]
    LDL, NB, V_AT, PRM, SEED, LIVE, GEN, BPRM, POS, KVL = 1, 13, 14, 16, 17, 18, 19, 20, 22, 23
    refused = [({V_AT: 32772, LDL: 40000}, ERR_UNSUPPORTED), ({V_AT: 62, LDL: 64}, ERR_UNSUPPORTED), ({NB: 0}, ERR_UNSUPPORTED),
               ({NB: 9}, ERR_UNSUPPORTED), ({V_AT: 12, NB: 8}, ERR_UNSUPPORTED), ({LDL: V - 4}, ERR_ARG), ({V_AT: 0}, ERR_ARG),
               ({PRM: None}, ERR_ARG), ({SEED: None}, ERR_ARG), ({LIVE: None}, ERR_ARG), ({GEN: None}, ERR_ARG), ({BPRM: None}, ERR_ARG),
               ({POS: None}, ERR_ARG), ({KVL: None}, ERR_ARG)]
    refused += [({at: None}, ERR_ARG) for at in (0, 2, 4, 5, 6, 7, 8, 9, 10)]
    for change, rc in refused:
        args = list(good)
        for at, v in change.items():
            args[at] = v
        assert L.mh_beam_sample_topk_items(*args) == rc, (change, rc)
    ids = torch.zeros(R, dtype=torch.long, device=DEV)
    seen_good = [seen.data_ptr(), pos.data_ptr(), ids.data_ptr(), G, nb, V, live.data_ptr(), None]
    for change, rc in (({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: None}, ERR_ARG), ({6: None}, ERR_ARG), ({5: 0}, ERR_ARG),
                       ({4: 0}, ERR_UNSUPPORTED), ({4: 9}, ERR_UNSUPPORTED), ({3: 65536}, ERR_UNSUPPORTED)):
        args = list(seen_good)
        for at, v in change.items():
            args[at] = v
        assert L.mh_beam_seen_update_items(*args) == rc, (change, rc)
    torch.cuda.synchronize()
    # the wrappers: a short or mistyped buffer never reaches the library
    t = {k: v[1] for k, v in wins.items()}
    pos_args = [logits, scores, t["part_k"], t["part_a"], t["part_i"], t["part_f"], t["out_s"], t["out_i"], t["out_f"], G, nb, live, gen,
                bprm]
    base = dict(params=prm, seed=seed)
    for at, bad in ((2, t["part_k"][:R * K - 1]), (4, t["part_a"]), (5, t["part_f"][:R - 1]), (8, t["out_f"][:G - 1]), (9, 3), (10, 9),
                    (11, live[:1]), (11, torch.ones(G, device=DEV)), (12, gen[:1]), (12, torch.zeros(G, dtype=torch.long, device=DEV)),
                    (13, bprm[:1]), (11, None), (12, None), (13, None)):
        args = list(pos_args)
        args[at] = bad
        with pytest.raises((_lib.MyriadHipError, ValueError, TypeError)):
            ops.beam_sample_topk_items(*args, **base)
    for kw in (dict(params=prm[:3], seed=seed), dict(params=prm, seed=None), dict(params=prm, seed=seed[:1]),
               dict(params=prm, seed=_i32([3, 4])), dict(base, seen=seen[:R * 2 - 1]), dict(base, pos=pos), dict(base, pos=pos[:R - 1], kvlen=pos),
               dict(base, out_k=t["out_k"][:G * K - 1])):
        with pytest.raises(_lib.MyriadHipError):
            ops.beam_sample_topk_items(*pos_args, **kw)
    with pytest.raises(_lib.MyriadHipError, match="UNSUPPORTED"):            # V % 4 through the wrapper: the library's own limit
        ops.beam_sample_topk_items(torch.randn(R, 62, device=DEV), *pos_args[1:], **base)
    for bad in (dict(seen=seen[:R * 2 - 1]), dict(ids=torch.zeros(R, dtype=I32, device=DEV)), dict(live=live[:1]), dict(live=None),
                dict(live=torch.ones(G, device=DEV)), dict(src=pos[:R - 1])):
        a = dict(dict(seen=seen, src=pos, ids=ids, live=live), **bad)
        with pytest.raises(_lib.MyriadHipError):
            ops.beam_seen_update_items(a["seen"], a["src"], a["ids"], G, nb, V, a["live"])
    torch.cuda.synchronize()
    for name, (buf, _) in dict(wins, seen=(seen_buf, seen)).items():
        assert_untouched(buf, f"refusal {name}")
    assert pos.tolist() == [4] * R and gen.tolist() == [4, 4]
    assert_frame_untouched(pbuf, slice(0, 1), slice(PAD, PAD + R), "pos")
    assert L.mh_beam_sample_topk_items(*good) == OK and L.mh_beam_sample_topk_items(*[0 if i == 12 else a for i, a in enumerate(good)]) == OK
    torch.cuda.synchronize()
    assert gen.tolist() == [5, 5]                                     # the good call ran once; G = 0 is a no-op


# ------------------------------------------------------------------------------------------------ SlotDecoder.run(num_beams, sampled)
KW = dict(max_new_tokens=bf.MAX_NEW, stop_ids=bf.STOPS, eos_id=bf.EOS, min_length=bf.MIN_LENGTH)
# SAMPLE is the evaluation script's kind of knobs.  Under its top-p cut a row of this decisive fixture keeps no more than the two
# candidates a row must keep, so a group offers exactly the 2 * nb a step takes: every seed selects the same set and the noise
# decides nothing.  DRAW (no top-p cut, a higher temperature) keeps top_k candidates a row in play: there the noise decides which
# 2 * nb are taken.  On the beam trap the two returned hypotheses still follow the seed for some requests only (the engineered
# paths outscore what the noise brings in), so every comparison the noise has to decide is also made on the flat model below,
# where moving the seeds changes every request's answer, and that is asserted.
SAMPLE = dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.95, repetition_penalty=1.3)
DRAW = dict(do_sample=True, temperature=1.5, top_k=20, top_p=1.0, repetition_penalty=1.1)
NOISE = [0, 10, 3, 7, 1, 5, 2]
SEEDS = [11, 2**40 + 5, 977, 31337, 2**62 + 1, 8, 4242]
RESCORE_TOL = NEAR_TIE                                               # the bound the beam tests hold a device beam score to (2e-2)


@pytest.fixture(scope="module")
def trap():
    lm = LlamaHIP(bf.weights(), bf.BEAM_TRAP["heads"], DEV, need_backward=False)
    lm.slot_beams = lm.beam_sampling = True
    return lm


def _ragged(n=7):
    """request i: fixture row i % 3 behind NOISE[i] rows of noise, so the prompts differ in length"""
    g = torch.Generator().manual_seed(41)
    rows = bf.inputs([0, 1, 2])
    return [torch.cat([torch.randn(NOISE[i], rows.shape[2], generator=g) * 0.3, rows[i % 3]], 0).to(DEV) for i in range(n)]


def _first_draw(gen_seed):
    """The seed beam_generate draws from a generator seeded with gen_seed (its first draw)."""
    return int(torch.randint(0, 2**63 - 1, (1,), generator=torch.Generator().manual_seed(gen_seed)))


def _equal_runs(a, b):
    a, b = sorted(a, key=lambda o: o[0]), sorted(b, key=lambda o: o[0])
    assert [o[0] for o in a] == [o[0] for o in b]
    for x, y in zip(a, b):
        assert torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]) and x[3] == y[3], (x, y)


def _changed(a, b):
    """The requests whose ids differ between two runs of the same requests."""
    a, b = {o[0]: o[1] for o in a}, {o[0]: o[1] for o in b}
    assert sorted(a) == sorted(b)
    return [i for i in sorted(a) if a[i].shape != b[i].shape or not torch.equal(a[i], b[i])]


@pytest.mark.parametrize("mode", ["sampled", "draw", "penalty"])
@pytest.mark.parametrize("nb,rows", [(2, [0, 1, 2]), (4, [0, 1])])
def test_sampled_slot_beams_are_beam_generate_alone_bit_for_bit(trap, nb, rows, mode):
    """Request i with seeds=[s_i] returns the ids, lengths and sequence scores of beam_generate on it alone with a generator
    whose first draw is s_i; the same for the penalty without a draw.  More requests than groups, so groups are refilled.
    "draw" is DRAW, where the noise decides which candidates a step takes; the two hypotheses this fixture returns follow the
    seed for some requests only (all three at nb = 2, none at nb = 4, measured), so the comparison that every seed moves is
    test_flat_sampled_slot_beams_are_beam_generate_alone_whatever_the_neighbours."""
    reqs = [bf.inputs([r])[0].to(DEV) for r in rows]
    skw = dict(sampled=SAMPLE, draw=DRAW, penalty=dict(repetition_penalty=1.3))[mode]
    drawn = [_first_draw(100 + i) for i in range(len(rows))]
    seeds = dict(seeds=drawn) if mode != "penalty" else {}
    dec = trap.slot_decoder(4, 64)
    outs = sorted(dec.run(reqs, num_beams=nb, num_return_sequences=2, **KW, **skw, **seeds), key=lambda o: o[0])
    st = dict(dec.last_stats)
    assert [o[0] for o in outs] == list(range(len(rows)))
    assert st["num_beams"] == nb and st["beam_sampled_steps"] == st["steps"] > 0 and st["beam_host_steps"] == 0
    for i, (o, x) in enumerate(zip(outs, reqs)):
        ids, sc = trap.beam_generate(x[None], nb, num_return_sequences=2, return_scores=True,
                                     generator=torch.Generator().manual_seed(100 + i), **KW, **skw)
        assert o[1].dtype == torch.long and torch.equal(o[1], ids), (i, o[1], ids)
        assert o[3] == list(trap.last_generate_stats["lengths"])
        assert torch.equal(o[2], sc), (i, o[2], sc)                  # bit for bit


def test_sampled_requests_do_not_depend_on_neighbours_slots_or_order(trap):
    """Under DRAW, where the noise decides which candidates a step takes: moving every seed by one changes the answers of
    requests 0, 2, 5 and 6 (measured; asserted: at least one).  The flat model's test below repeats the comparisons where
    every request's answer follows its seed."""
    reqs = _ragged()
    run = dict(num_beams=2, num_return_sequences=2, seeds=SEEDS, **KW, **DRAW)
    dec = trap.slot_decoder(4, 64)
    outs = list(dec.run(reqs, **run))
    st = dict(dec.last_stats)
    assert sorted(o[0] for o in outs) == list(range(7)) and st["prefills"] == st["prefill_passes"] == 7
    assert st["graph_captures"] == 1 and st["graph_replays"] > 0 and st["beam_host_steps"] == 0
    moved = _changed(outs, list(dec.run(reqs, **dict(run, seeds=[s + 1 for s in SEEDS]))))
    print(f"requests whose answer changes with the seed: {moved}")
    assert moved                                                     # another seed, another answer
    # request 3 alone in the decoder, on stale cache rows and bitmaps, is what it was among six others
    (solo,) = list(dec.run([reqs[3]], **dict(run, seeds=[SEEDS[3]])))
    among = next(o for o in outs if o[0] == 3)
    assert torch.equal(solo[1], among[1]) and torch.equal(solo[2], among[2]) and solo[3] == among[3]
    _equal_runs(outs, list(dec.run(reqs, ordered=True, **run)))
    dec8 = trap.slot_decoder(8, 64)
    _equal_runs(outs, list(dec8.run(reqs, **run)))
    # a generator hands out the same seeds as the list of its draws
    g = torch.Generator().manual_seed(3)
    drawn = [int(torch.randint(0, 2**63 - 1, (1,), generator=g)) for _ in range(7)]
    by_gen = list(dec.run(reqs, **dict(run, seeds=None, generator=torch.Generator().manual_seed(3))))
    _equal_runs(by_gen, list(dec.run(reqs, **dict(run, seeds=drawn))))
    # the knobs sit in device memory: other values replay the graph captured above
    kw2 = dict(run, temperature=1.2, top_p=0.98, top_k=12, repetition_penalty=1.3, min_length=3)
    outs2 = list(dec.run(reqs, **kw2))
    st2 = dec.last_stats
    assert sorted(o[0] for o in outs2) == list(range(7))
    assert st2["graph_captures"] == 1 and st2["graph_replays"] == st2["steps"] == st2["beam_sampled_steps"] > 0
    for o in outs2:                                                  # EOS is banned while a request has fewer than 3 tokens
        assert all(bf.EOS not in o[1][r, :min(n, 3)].tolist() for r, n in enumerate(o[3])), o
    assert _changed(outs, outs2)                                     # the knobs mattered
    list(dec.run(reqs, **dict(run, **SAMPLE)))
    assert dec.last_stats["graph_captures"] == 1 and dec.last_stats["graph_replays"] == dec.last_stats["steps"]


def test_packed_prefill_returns_every_request_and_rescores_through_the_oracle(trap):
    """prefill_batch=2: every hypothesis teacher-forced through the CPU oracle on the request's own prompt -- each id lies in its
    step's kept set and the processed values sum to the reported score, within beam_generate's own rescoring bound."""
    from oracle import myriad_ref as R
    reqs = _ragged()
    sd, heads = bf.weights(), bf.BEAM_TRAP["heads"]
    emb = sd["llama_model.model.embed_tokens.weight"]
    dec = trap.slot_decoder(4, 64)
    outs = list(dec.run(reqs, num_beams=2, num_return_sequences=2, seeds=SEEDS, prefill_batch=2, ordered=True, **KW, **SAMPLE))
    st = dec.last_stats
    assert [o[0] for o in outs] == list(range(7)) and st["prefills"] == 7 and st["prefill_passes"] < 7
    inv_temp = float(np.float32(1.0 / SAMPLE["temperature"]))
    for i, ids, sc, lengths in outs:
        x = reqs[i].cpu()
        for r in range(ids.shape[0]):
            seq = ids[r, :lengths[r]].tolist()
            total = torch.zeros((), dtype=F32)
            for t in range(len(seq)):
                e = torch.cat([x, emb[seq[:t]]], 0) if t else x
                row = R.llama_causal_lm(sd, e[None], torch.ones(1, e.shape[0]), None, heads)[1][0, -1].float()
                w, _ = BR.processed(row, seq[:t], SAMPLE["repetition_penalty"], bf.EOS if t < bf.MIN_LENGTH else -1, inv_temp,
                                    SAMPLE["top_k"], SAMPLE["top_p"])
                assert bool(torch.isfinite(w[seq[t]])), (i, r, t, seq)
                total = total + w[seq[t]]
            assert abs(float(total / len(seq)) - float(sc[r])) < RESCORE_TOL, (i, r, seq, float(total / len(seq)), float(sc[r]))


def test_a_flagged_group_is_redone_by_the_host_rule(trap, monkeypatch):
    """The overflow flag of group 0 forced in every record read (refills' first selections included): those selections run on
    decode_host's rule with the group's seed, its own t and item 0, and the run returns what the device's selection returned.
    Under DRAW: request 0, the first through group 0, is one whose answer follows its seed (asserted), so a redo with another
    seed, t or item shows; the flat model's test repeats the redo where every request's does."""
    reqs = _ragged(5)
    run = dict(num_beams=2, num_return_sequences=2, seeds=SEEDS[:5], ordered=True, **KW, **DRAW)
    dec = trap.slot_decoder(4, 64)
    outs = list(dec.run(reqs, **run))
    steps = dec.last_stats["steps"]
    assert dec.last_stats["beam_host_steps"] == 0
    assert 0 in _changed(outs, list(dec.run(reqs, **dict(run, seeds=[s + 1 for s in SEEDS[:5]]))))
    read = decode._beam_sample_record

    def flagged(rec, G, K):
        top_s, top_i, flags = read(rec, G, K)
        flags = flags.copy()
        flags[0] = 1
        return top_s, top_i, flags
    monkeypatch.setattr(decode, "_beam_sample_record", flagged)
    again = list(dec.run(reqs, **run))
    st = dec.last_stats
    assert st["beam_host_steps"] > 0 and st["steps"] == steps
    for a, b in zip(outs, again):
        assert a[0] == b[0] and torch.equal(a[1], b[1]) and a[3] == b[3] and float((a[2] - b[2]).abs().max()) < 1e-4


@pytest.fixture(scope="module")
def flat():
    """The flat llama_tiny model of tests/test_sampling_gpu.py: its hypotheses do come back to tokens they have generated, so the
    seen bitmaps decide selections, which the beam-trap chains never let them do."""
    _, sd, heads = _tiny()
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    lm.slot_beams = lm.beam_sampling = True
    return lm


FLAT_KW = dict(max_new_tokens=8, stop_ids=(), eos_id=2, min_length=1)


@pytest.mark.parametrize("mode", ["penalty", "sampled"])
def test_the_bitmaps_decide_on_the_flat_model_and_the_slots_stay_beam_generate_alone(flat, mode, monkeypatch):
    """Five random prompts through two groups (so groups are refilled over stale bitmaps) with repetition_penalty = 2, without
    a draw and under DRAW: each request returns the ids and lengths of beam_generate on it alone with its seed, and its scores
    within the bound the deterministic slot beams are held to on prompts that are no fixture rows (their prefill is another
    kernel's than beam_generate's).  The penalty is shown to decide -- the run without it returns other ids -- and so is the
    seed; then the same run with group 0 flagged in every record, redone by the host rule on BeamItem.run_seqs."""
    reqs = [x.to(DEV) for x in _requests([4, 9, 6, 5, 7], flat.D, 31)]
    skw = dict(repetition_penalty=2.0) if mode == "penalty" else dict(DRAW, repetition_penalty=2.0)
    drawn = [_first_draw(200 + i) for i in range(len(reqs))]
    seeds = dict(seeds=drawn) if mode == "sampled" else {}
    run = dict(num_beams=2, num_return_sequences=2, ordered=True, **FLAT_KW)
    dec = flat.slot_decoder(4, 64)
    outs = list(dec.run(reqs, **run, **skw, **seeds))
    st = dict(dec.last_stats)
    assert [o[0] for o in outs] == list(range(len(reqs)))
    assert st["beam_sampled_steps"] == st["steps"] > 0 and st["beam_host_steps"] == 0 and st["prefills"] == len(reqs)
    for i, (o, x) in enumerate(zip(outs, reqs)):
        ids, sc = flat.beam_generate(x[None], 2, num_return_sequences=2, return_scores=True,
                                     generator=torch.Generator().manual_seed(200 + i), **FLAT_KW, **skw)
        print(f"{mode} request {i}: ids {o[1].tolist()} score bits equal: {torch.equal(o[2], sc)}")
        assert torch.equal(o[1], ids) and o[3] == list(flat.last_generate_stats["lengths"]), (i, o[1], ids)
        assert float((o[2] - sc).abs().max()) < NEAR_TIE, (i, o[2], sc)
    repeats = sum(len(set(o[1][r, :n].tolist())) < n for o in outs for r, n in enumerate(o[3]))
    plain = list(dec.run(reqs, **run, **dict(skw, repetition_penalty=1.0), **seeds))
    moved = _changed(outs, plain)
    print(f"{mode}: hypotheses with a repeated token under the penalty: {repeats}; requests the penalty changes: {moved}")
    assert moved                                                     # the bitmaps decide
    if mode == "sampled":
        assert _changed(outs, list(dec.run(reqs, **run, **skw, seeds=[s + 1 for s in drawn]))) == list(range(len(reqs)))
    read = decode._beam_sample_record

    def flagged(rec, G, K):
        top_s, top_i, flags = read(rec, G, K)
        flags = flags.copy()
        flags[0] = 1
        return top_s, top_i, flags
    monkeypatch.setattr(decode, "_beam_sample_record", flagged)
    again = list(dec.run(reqs, **run, **skw, **seeds))
    assert dec.last_stats["beam_host_steps"] > 0 and dec.last_stats["steps"] == st["steps"]
    for a, b in zip(outs, again):
        assert a[0] == b[0] and torch.equal(a[1], b[1]) and a[3] == b[3] and float((a[2] - b[2]).abs().max()) < 1e-4


def test_flat_sampled_slot_beams_are_beam_generate_alone_whatever_the_neighbours(flat):
    """Seven ragged random prompts under DRAW on the flat model, where every request's answer follows its seed (asserted: moving
    the seeds by one changes all seven).  Each request returns the ids and lengths of beam_generate on it alone with its seed
    (scores within the bound held on prompts that are no fixture rows), so its seed, its t = gen[g] and its bitmap are its own;
    request 3 alone is request 3 among the others, 8 slots are 4 slots and ordered is unordered, bit for bit; the packed
    prefill hands every request its own seed too."""
    reqs = [x.to(DEV) for x in _requests([5, 11, 3, 8, 4, 9, 6], flat.D, 32)]
    drawn = [_first_draw(300 + i) for i in range(len(reqs))]
    knobs = dict(FLAT_KW, **dict(DRAW, repetition_penalty=1.3))
    run = dict(num_beams=2, num_return_sequences=2, seeds=drawn, **knobs)
    dec = flat.slot_decoder(4, 64)
    outs = list(dec.run(reqs, **run))
    st = dict(dec.last_stats)
    assert sorted(o[0] for o in outs) == list(range(7)) and st["prefills"] == st["prefill_passes"] == 7
    assert st["beam_sampled_steps"] == st["steps"] > 0 and st["beam_host_steps"] == 0
    assert _changed(outs, list(dec.run(reqs, **dict(run, seeds=[s + 1 for s in drawn])))) == list(range(7))
    alone = {}
    for i, x in enumerate(reqs):
        ids, sc = flat.beam_generate(x[None], 2, num_return_sequences=2, return_scores=True,
                                     generator=torch.Generator().manual_seed(300 + i), **knobs)
        alone[i] = (ids, sc, list(flat.last_generate_stats["lengths"]))
    for o in outs:
        ids, sc, lengths = alone[o[0]]
        print(f"request {o[0]}: score bits equal: {torch.equal(o[2], sc)}")
        assert torch.equal(o[1], ids) and o[3] == lengths, (o[0], o[1], ids)
        assert float((o[2] - sc).abs().max()) < NEAR_TIE, (o[0], o[2], sc)
    (solo,) = list(dec.run([reqs[3]], **dict(run, seeds=[drawn[3]])))
    among = next(o for o in outs if o[0] == 3)
    assert torch.equal(solo[1], among[1]) and torch.equal(solo[2], among[2]) and solo[3] == among[3]
    _equal_runs(outs, list(dec.run(reqs, ordered=True, **run)))
    _equal_runs(outs, list(flat.slot_decoder(8, 64).run(reqs, **run)))
    packed = list(dec.run(reqs, prefill_batch=2, ordered=True, **run))
    assert [o[0] for o in packed] == list(range(7)) and dec.last_stats["prefill_passes"] < 7
    for o in packed:                                                 # another prefill kernel: the same draws, near scores
        ids, sc, lengths = alone[o[0]]
        assert torch.equal(o[1], ids) and o[3] == lengths and float((o[2] - sc).abs().max()) < NEAR_TIE, (o[0], o[1], ids)


def test_sampled_slot_beams_sit_behind_both_switches(trap):
    reqs = _ragged(2)
    dec = trap.slot_decoder(4, 64)
    trap.beam_sampling = False
    try:
        for bad in (dict(do_sample=True), dict(repetition_penalty=1.2), dict(seeds=[1, 2])):
            with pytest.raises(NotImplementedError):
                list(dec.run(reqs, num_beams=2, **KW, **bad))
    finally:
        trap.beam_sampling = True
    for bad, exc in ((dict(return_scores=True), NotImplementedError), (dict(return_scores=True, **SAMPLE), NotImplementedError),
                     (dict(do_sample=True, top_k=2000), NotImplementedError), (dict(do_sample=True, top_k=0), NotImplementedError),
                     (dict(seeds=[1, 2]), ValueError), (dict(seeds=[1, 2], repetition_penalty=1.3), ValueError),
                     (dict(do_sample=True, temperature=0.0), ValueError), (dict(repetition_penalty=0.0), ValueError),
                     (dict(do_sample=True, seeds=[1]), ValueError), (dict(do_sample=True, seeds=[1, -2]), ValueError)):
        with pytest.raises(exc):
            list(dec.run(reqs, num_beams=2, **dict(KW, **bad)))
    with pytest.raises(NotImplementedError):
        dec.run_turns([("a", reqs[0], list(range(reqs[0].shape[0])))], num_beams=2, **SAMPLE)
    trap.slot_beams = False
    try:
        with pytest.raises(NotImplementedError, match="MYRIAD_SLOT_BEAMS"):
            list(dec.run(reqs, num_beams=2, **KW, **SAMPLE))
    finally:
        trap.slot_beams = True
    assert [o[0] for o in dec.run(reqs, num_beams=2, ordered=True, seeds=[5, 6], **KW, **SAMPLE)] == [0, 1]    # and it still serves


def test_deterministic_slot_beams_issue_the_launches_they_did(trap, monkeypatch):
    """run(num_beams=2) without a sampling argument, both switches on: the library calls of the run with the beam sampling switch
    off, none of the items-form sampling entries among them, and the deterministic step's own sequence of beam entries."""
    from tests.test_decode_launches_gpu import _Noting
    reqs = [bf.inputs([0])[0].to(DEV)]
    lib, calls = _lib.load(), []
    ops.ensure_workspace(DEV)
    monkeypatch.setattr(_lib, "load", lambda: _Noting(lib, calls))
    traces = {}
    for on in (False, True):
        trap.beam_sampling = on
        try:
            dec = trap.slot_decoder(2, 64)
            del calls[:]
            out = list(dec.run(reqs, num_beams=2, num_return_sequences=2, top_k=7, top_p=0.5, temperature=2.0, **KW))
            torch.cuda.synchronize()
            traces[on] = (list(calls), out[0][1].tolist(), dec.last_stats["steps"], sorted(dec.beam_views))
        finally:
            trap.beam_sampling = True
    assert traces[True] == traces[False]
    names, _, steps, views = traces[True]
    assert views == [(2, False)] and steps >= 2
    beam = [c for c in names if c.startswith("mh_beam")]
    # the refill's first selection and broadcast, then the eager step, the eager step that is captured and the capture itself
    assert beam == ["mh_beam_topk", "mh_beam_reorder_kv_items"] + ["mh_beam_reorder_kv_items", "mh_beam_topk_items"] * 3, beam
    del calls[:]
    list(trap.slot_decoder(2, 64).run(reqs, num_beams=2, seeds=[3], **KW, **SAMPLE))
    beam = [c for c in calls if c.startswith("mh_beam")]
    assert beam[:2] == ["mh_beam_sample_topk_items", "mh_beam_reorder_kv_items"]
    assert beam[2:5] == ["mh_beam_reorder_kv_items", "mh_beam_seen_update_items", "mh_beam_sample_topk_items"]
    assert "mh_beam_topk" not in beam and "mh_beam_topk_items" not in beam


# ------------------------------------------------------------------------------------------------ the model and the eval entry
def test_generate_stream_takes_sampled_beams_behind_both_switches(model):
    model.eval()
    prev = (getattr(model.llama, "slot_beams", False), model.llama.beam_sampling)
    try:
        batches = _ragged_batches(model, (2, 3), seed=3)
        kw = dict(max_new_tokens=8, stop_ids=((835,), (2277, 29937)), min_length=1, num_beams=2, num_return_sequences=2, do_sample=True,
                  top_p=0.9, temperature=1.0, repetition_penalty=1.2)
        seeds = [5, 6, 7, 8, 9]
        model.llama.slot_beams, model.llama.beam_sampling = True, False
        with pytest.raises(NotImplementedError):
            model.generate_stream(iter(batches), slots=4, seeds=seeds, **kw)
        with pytest.raises(NotImplementedError):
            model.generate_stream(iter(batches), slots=4, seeds=seeds, **dict(kw, do_sample=False, repetition_penalty=1.0))
        model.llama.slot_beams, model.llama.beam_sampling = False, True
        with pytest.raises(NotImplementedError, match="MYRIAD_SLOT_BEAMS"):
            model.generate_stream(iter(batches), slots=4, seeds=seeds, **kw)
        model.llama.slot_beams = True
        runs = [list(model.generate_stream(iter(batches), slots=s, seeds=seeds, **kw)) for s in (4, 4, 8)]
        st = model.last_generate_stats
        assert st["prefills"] == 5 and st["num_beams"] == 2 and st["beam_sampled_steps"] == st["steps"] > 0
        for outs in runs:
            assert [o["index"] for o in outs] == [0, 1, 2, 3, 4]
            for o, ref in zip(outs, runs[0]):
                assert o["token_ids"].dtype == torch.long and o["token_ids"].dim() == 2 and o["token_ids"].shape[0] == 2
                assert o["sequences_scores"].shape == (2,) and bool(torch.isfinite(o["sequences_scores"]).all())
                assert torch.equal(o["token_ids"], ref["token_ids"]) and torch.equal(o["sequences_scores"], ref["sequences_scores"])
        other = list(model.generate_stream(iter(batches), slots=4, seeds=[15, 16, 17, 18, 19], **kw))
        assert any(a["token_ids"].shape != b["token_ids"].shape or not torch.equal(a["token_ids"], b["token_ids"])
                   for a, b in zip(other, runs[0]))                                             # flat logits: another seed differs
        with pytest.raises(NotImplementedError):
            model.generate_stream(iter(batches), slots=4, **dict(kw, top_k=0))
    finally:
        model.llama.slot_beams, model.llama.beam_sampling = prev
        model.train()


def test_eval_entry_point_takes_beam_sample_in_the_slots(fx, tmp_path, monkeypatch):
    import eval_aqa
    monkeypatch.setenv("MYRIAD_SLOT_BEAMS", "1")
    monkeypatch.setenv("MYRIAD_BEAM_SAMPLING", "1")
    rows = {}
    for slots in (0, 4):
        res = str(tmp_path / f"res{slots}.jsonl")
        path, records = eval_aqa.main(["--cfg-path", fx["eval_yaml"], "--dataset", "synthetic", "--bs", "2", "--limit", "2",
                                       "--slots", str(slots), "--num-beams", "2", "--beam-sample", "--repetition-penalty", "1.05",
                                       "--out", res])
        rows[slots] = [json.loads(l) for l in open(path)]
        assert len(rows[slots]) == len(records) == 4                 # one record per sample
    assert [r["image_id"] for r in rows[4]] == [r["image_id"] for r in rows[0]]          # the dataset's order
    assert [r["image_path"] for r in rows[4]] == [r["image_path"] for r in rows[0]]
    assert all(set(a) == set(b) for a, b in zip(rows[4], rows[0]))
    with pytest.raises(SystemExit):
        eval_aqa.parse_args(["--cfg-path", fx["eval_yaml"], "--beam-sample"])
