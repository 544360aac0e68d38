"""Beam-search multinomial sampling on the device: mh_beam_sample_topk / mh_beam_seen_update against tests/beam_sample_ref.py
(every output a window inside a poisoned buffer, logit rows padded with what a row must never read), the deterministic form
against mh_beam_topk bit for bit, the draw against the exact Plackett-Luce probabilities, the overflow hand-over to the host's
rule, the launchers' refusals, and LlamaHIP.beam_generate / MyriadHIP.generate / Chat.answer with the beam sampling switch on."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from myriad_amd.decode_host import beam_sample_select  # noqa: E402
from myriad_amd.llama import LlamaHIP  # noqa: E402
from tests import beam_fixture as bf  # noqa: E402
from tests import beam_sample_ref as BR  # noqa: E402
from tests.fp64_bounds import assert_frame_untouched, assert_untouched, poisoned, untouched  # noqa: E402
from tests.test_beam_gpu import _oracle_fn  # noqa: E402
from tests.test_entrypoints_gpu import _batch, fx, model  # noqa: E402,F401

DEV = "cuda"
F32, I32 = torch.float32, torch.int32
PAD = 8
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
GAPS = {"acc": 0.0, "key": 0.0, "items": 0, "near": 0}      # the largest |got - ref| / max(1, |ref|) seen over the grid


def _win(n, dtype):
    """(buffer, window): n contiguous elements inside a poisoned [1, n + 2 PAD] buffer."""
    buf = poisoned((1, n + 2 * PAD), dtype, DEV)
    return buf, buf[0, PAD:PAD + n]


def _buffers(B, nb, keys=True):
    R, K = B * nb, 2 * nb
    wins = dict(part_k=_win(R * K, F32), part_a=_win(R * K, F32), part_i=_win(R * K, I32), part_f=_win(R, I32),
                out_s=_win(B * K, F32), out_i=_win(B * K, I32), out_f=_win(B, I32))
    if keys:
        wins["out_k"] = _win(B * K, F32)
    return wins


def _prm(inv_temp, top_p, top_k, penalty):
    return torch.tensor([inv_temp, top_p, float(top_k), penalty], dtype=F32).to(DEV)


def _seed(seed):
    return torch.tensor([seed], dtype=torch.long).to(DEV)


def _run(logits_dev, scores, B, nb, prm, seed, seen=None, ban=-1, draw=True, t=0, keys=True, what=""):
    """One ops.beam_sample_topk into bordered windows; (acc [B, K], flat [B, K], key [B, K] or None, flag [B]) on the host after
    the checks every launch gets: frames untouched, every owned element written."""
    wins = _buffers(B, nb, keys)
    w = {k: v[1] for k, v in wins.items()}
    ops.beam_sample_topk(logits_dev, scores, w["part_k"], w["part_a"], w["part_i"], w["part_f"], w["out_s"], w["out_i"], w["out_f"],
                         B, nb, ban_id=ban, draw=draw, params=prm, seed=seed, seen=seen, t_add=t, out_k=w.get("out_k"))
    torch.cuda.synchronize()
    for name, (buf, win) in wins.items():
        assert_frame_untouched(buf, slice(0, 1), slice(PAD, PAD + win.numel()), f"{what} {name}")
        assert not bool(untouched(win).any()), f"{what}: {name} has elements nothing wrote"
    K = 2 * nb
    return (w["out_s"].cpu().view(B, K).numpy(), w["out_i"].cpu().view(B, K).long().numpy(),
            w["out_k"].cpu().view(B, K).numpy() if keys else None, w["out_f"].cpu().numpy())


def _device_logits(logits, extra, fill=float("nan")):
    """[R, V + extra] on the device, the columns past V filled with what a row must never read; the [R, V] view."""
    R, V = logits.shape
    host = torch.full((R, V + extra), fill, dtype=F32)
    host[:, :V] = logits
    return host.to(DEV)[:, :V]


def _tol(ref):
    return BR.TOL * np.maximum(1.0, np.abs(np.asarray(ref, dtype=np.float64)))


def _check_item(name, it, acc, flat, key, V):
    """What the issue asks of one item's record against the reference's kept set."""
    flat = [int(f) for f in flat]
    assert len(set(flat)) == len(flat), (name, flat)
    assert all(f in it.acc for f in flat), (name, "a selected candidate is outside the reference's kept set", flat)
    acc_ref = np.array([it.acc[f] for f in flat], dtype=np.float64)
    key_ref = np.array([it.key[f] for f in flat], dtype=np.float64)
    da, dk = np.abs(acc - acc_ref), np.abs(key - key_ref)
    GAPS["acc"] = max(GAPS["acc"], float((da / np.maximum(1.0, np.abs(acc_ref))).max()))
    GAPS["key"] = max(GAPS["key"], float((dk / np.maximum(1.0, np.abs(key_ref))).max()))
    assert np.all(da <= _tol(acc_ref)), (name, acc, acc_ref)
    assert np.all(dk <= _tol(key_ref)), (name, key, key_ref)
    for k in range(len(flat) - 1):                          # keys do not increase; equal keys in ascending flat order
        assert key[k] > key[k + 1] or (key[k] == key[k + 1] and flat[k] < flat[k + 1]), (name, k, key, flat)
    low = float(key.min())
    left = np.array([it.key[f] for f in it.key if f not in set(flat)], dtype=np.float64)
    if left.size:
        assert np.all(left <= low + BR.TOL * max(1.0, abs(low))), (name, "a kept candidate beats a selected one", float(left.max()), low)


@pytest.mark.parametrize("name", [c.name for c in BR.CASES])
def test_kernel_matches_the_reference_on_the_grid(name):
    c = next(c for c in BR.CASES if c.name == name)
    inp, ref = c.inputs(), c.ref()
    logits = _device_logits(inp["logits"], c.ldl_extra)
    assert logits.stride(0) == c.V + c.ldl_extra
    seen = BR.seen_bitmap(inp["seen"], c.V).to(DEV)
    acc, flat, key, flag = _run(logits, inp["scores"].to(DEV), c.B, c.nb, _prm(c.inv_temp, c.top_p, c.top_k, c.penalty),
                                _seed(inp["seed"]), seen=seen, ban=c.ban, t=0 if c.first else c.t, what=name)
    assert not flag.any()
    for b, it in enumerate(ref):
        GAPS["items"] += 1
        if it.near:
            GAPS["near"] += 1
            continue
        _check_item(f"{name} item {b}", it, acc[b], flat[b], key[b], c.V)
    print(f"{name}: largest relative gap so far acc {GAPS['acc']:.3e} key {GAPS['key']:.3e}; near items {GAPS['near']} of {GAPS['items']}")


def test_near_items_skipped_stay_under_two_percent():
    """What the grid test skips, counted from the reference (the CPU suite asserts the same condition)."""
    items = [it for c in BR.CASES for it in c.ref()]
    assert sum(it.near for it in items) <= 0.02 * len(items)


@pytest.mark.parametrize("V,nb,B", [(32000, 4, 3), (4100, 8, 1), (36, 2, 3), (16, 8, 1)])
def test_deterministic_form_equals_beam_topk_bit_for_bit(V, nb, B):
    g = torch.Generator().manual_seed(V + nb)
    R, K = B * nb, 2 * nb
    logits = _device_logits(torch.randn(R, V, generator=g) * 3.0, 4)
    scores = -torch.rand(R, generator=g) * 5.0
    scores[1::nb] = -1.0e9
    scores = scores.to(DEV)
    want = torch.zeros(2, B * K, dtype=I32, device=DEV)
    ps, pi = torch.empty(R * K, device=DEV), torch.empty(R * K, dtype=I32, device=DEV)
    ops.beam_topk(logits, scores, ps, pi, want[0].view(F32), want[1], B, nb, ban_id=2)
    empty = torch.zeros(R, (V + 31) // 32, dtype=I32, device=DEV)
    for seen, prm in ((None, None), (empty, _prm(1.0, 1.0, 50, 1.0)), (empty, _prm(0.5, 0.3, 5, 1.0))):
        acc, flat, key, flag = _run(logits, scores, B, nb, prm, None, seen=seen, ban=2, draw=False, what="draw=0")
        assert np.array_equal(acc.view(np.int32).reshape(-1), want[0].cpu().numpy()), (acc, want[0].view(F32))
        assert np.array_equal(flat.reshape(-1), want[1].cpu().long().numpy())
        assert np.array_equal(key.view(np.int32), acc.view(np.int32)) and not flag.any()


def test_penalised_deterministic_form_matches_the_reference():
    c = next(c for c in BR.CASES if c.penalty != 1.0 and c.V == 32000 and c.nb == 3)
    inp = c.inputs()
    ref = BR.step(inp["logits"], inp["scores"], inp["seen"], c.B, c.nb, c.ban, 1.0, 50, 1.0, c.penalty, 0, 0, draw=False)
    seen = BR.seen_bitmap(inp["seen"], c.V).to(DEV)
    acc, flat, key, flag = _run(inp["logits"].to(DEV), inp["scores"].to(DEV), c.B, c.nb, _prm(1.0, 1.0, 50, c.penalty), None, seen=seen,
                                ban=c.ban, draw=False, what="penalised")
    for b, it in enumerate(ref):
        assert flat[b].tolist() == it.sel_flat
        assert np.all(np.abs(acc[b] - np.array(it.sel_acc)) <= _tol(it.sel_acc))
    hit = [f % c.V for b in range(c.B) for f in flat[b] if (f % c.V) in inp["seen"][b * c.nb + f // c.V]]
    unpen = BR.step(inp["logits"], inp["scores"], [[]] * (c.B * c.nb), c.B, c.nb, c.ban, 1.0, 50, 1.0, 1.0, 0, 0, draw=False)
    assert hit or any(u.sel_flat != r.sel_flat for u, r in zip(unpen, ref))      # the penalty decided something in this case


def test_draws_follow_plackett_luce():
    """N = 4096 on the device: 8 launches (t = 0..7) of 512 items, the CPU test's bounds."""
    d = BR.DIST
    logits = BR.dist_logits().repeat(d["items"], 1).to(DEV)
    scores = torch.tensor(d["scores"]).repeat(d["items"]).to(DEV)
    prm, seed = _prm(1.0, 1.0, 50, 1.0), _seed(d["seed"])
    firsts, pairs = [], []
    for t in range(d["steps"]):
        _, flat, _, flag = _run(logits, scores, d["items"], d["nb"], prm, seed, t=t, keys=False, what="dist")
        assert not flag.any()
        firsts += flat[:, 0].tolist()
        pairs += list(zip(flat[:, 0].tolist(), flat[:, 1].tolist()))
        if t == 3:                                          # and they are the host rule's draws, item by item
            for b in (0, 1, 255, 511):
                _, want, _ = beam_sample_select(BR.dist_logits().numpy(), np.array(d["scores"], dtype=np.float32), [[], []], -1, 1.0,
                                                50, 1.0, 1.0, d["seed"], t, b)
                assert flat[b].tolist() == want.tolist()
    worst = BR.check_counts(firsts, pairs)
    print(f"worst z: first draws {worst['first'][0]:.2f} over {worst['first'][1]}, pairs {worst['pair'][0]:.2f} over {worst['pair'][1]}")


def test_a_tie_past_the_cap_raises_the_flag_and_the_host_redoes_the_item():
    B, nb, V = 2, 2, 4100
    g = torch.Generator().manual_seed(77)
    x = torch.randn(B * nb, V, generator=g)
    x[3, :] = -4.0
    x[3, 100:1600] = 1.0                                     # 1500 tokens tied at what becomes the k-th value ...
    x[3, 2000:2010] = torch.arange(10).float() * 0.25 + 2.0  # ... below ten distinct ones
    scores = torch.tensor([-0.3, -1.1, -0.2, -0.4])
    seed, t, top_k, top_p, inv_temp = 991, 5, 50, 0.9, float(np.float32(1.0 / 0.7))
    acc, flat, key, flag = _run(_device_logits(x, 4), scores.to(DEV), B, nb, _prm(inv_temp, top_p, top_k, 1.0), _seed(seed), t=t,
                                what="tie")
    assert flag.tolist() == [0, 1]
    assert all(0 <= f < nb * V for f in flat[1]) and len(set(flat[1].tolist())) == 2 * nb      # valid indices all the same
    ref = BR.step(x, scores, [[]] * 4, B, nb, -1, inv_temp, top_k, top_p, 1.0, seed, t)
    _check_item("tie item 0", ref[0], acc[0], flat[0], key[0], V)
    h_acc, h_flat, h_key = beam_sample_select(x[2:4].numpy(), scores[2:4].numpy(), [[], []], -1, inv_temp, top_k, top_p, 1.0, seed, t, 1)
    assert h_flat.tolist() == ref[1].sel_flat
    assert np.all(np.abs(h_acc - np.array(ref[1].sel_acc)) <= _tol(ref[1].sel_acc))
    assert np.all(np.abs(h_key - np.array(ref[1].sel_key)) <= _tol(ref[1].sel_key))


def test_record_advances_step_pos_and_kvlen():
    B, nb, V = 2, 2, 64
    logits = torch.randn(B * nb, V, generator=torch.Generator().manual_seed(8)).to(DEV)
    wins = {k: v[1] for k, v in _buffers(B, nb).items()}
    pos = torch.full((B * nb,), 7, dtype=I32, device=DEV)
    kvlen = torch.full((B * nb,), 8, dtype=I32, device=DEV)
    step = torch.tensor([3], dtype=I32).to(DEV)
    args = (logits, torch.zeros(B * nb, device=DEV), wins["part_k"], wins["part_a"], wins["part_i"], wins["part_f"], wins["out_s"],
            wins["out_i"], wins["out_f"], B, nb)
    kw = dict(params=_prm(1.0, 1.0, 50, 1.0), seed=_seed(5))
    ops.beam_sample_topk(*args, step=step, t_add=1, pos=pos, kvlen=kvlen, **kw)
    first = wins["out_i"].cpu().clone()
    torch.cuda.synchronize()
    assert pos.tolist() == [8] * 4 and kvlen.tolist() == [9] * 4 and step.tolist() == [4]
    ops.beam_sample_topk(*args, t_add=4, **kw)               # the same Philox step without the counter: the same draws
    assert torch.equal(wins["out_i"].cpu(), first) and step.tolist() == [4]
    ops.beam_sample_topk(*args, step=step, t_add=1, **kw)    # t = 5: another draw; no advance asked for, so none happens
    assert not torch.equal(wins["out_i"].cpu(), first) and step.tolist() == [4] and pos.tolist() == [8] * 4


# ------------------------------------------------------------------------------------------------ seen bitmaps
@pytest.mark.parametrize("V", [36, 32000])
@pytest.mark.parametrize("nb", [2, 8])
def test_seen_update_follows_the_parents(nb, V):
    B, W = 3, (V + 31) // 32
    R = B * nb
    g = torch.Generator().manual_seed(nb * V)
    old = torch.randint(-2**31, 2**31 - 1, (R, W), generator=g, dtype=torch.long).to(I32)
    # parents that cross (a reversal), duplicate (everything from one row) and stay
    src = list(range(nb))[::-1] + [nb + (nb - 1)] * nb + [2 * nb + j for j in range(nb)]
    ids = torch.randint(0, V, (R,), generator=g)
    ids[1], ids[R - 1] = -1, V + 5                             # no bit for an id outside the vocabulary
    buf, win = _win(R * W, I32)
    win.copy_(old.reshape(-1))
    ops.beam_seen_update(win, torch.tensor(src, dtype=I32).to(DEV), ids.to(DEV), B, nb, V)
    torch.cuda.synchronize()
    assert_frame_untouched(buf, slice(0, 1), slice(PAD, PAD + R * W), "seen")
    want = old.numpy().view(np.uint32).copy()
    o = old.numpy().view(np.uint32)
    for r in range(R):
        want[r] = o[src[r]]
        if 0 <= int(ids[r]) < V:
            want[r, int(ids[r]) >> 5] |= np.uint32(1) << np.uint32(int(ids[r]) & 31)
    assert np.array_equal(win.cpu().numpy().view(np.uint32).reshape(R, W), want)


# ------------------------------------------------------------------------------------------------ refusals
def test_launchers_refuse_bad_arguments_before_any_launch():
    B, nb, V = 2, 2, 64
    R, K = B * nb, 2 * nb
    L = _lib.load()
    logits = torch.randn(R, V, device=DEV)
    scores = torch.zeros(R, device=DEV)
    seen_buf, seen = _win(R * 2, I32)
    wins = _buffers(B, nb)
    w = {k: v[1].data_ptr() for k, v in wins.items()}
    prm, seed = _prm(1.0, 0.9, 50, 1.2), _seed(3)
    pbuf, pos = _win(R, I32)
    pos.fill_(4)
    step = torch.zeros(1, dtype=I32, device=DEV)
    good = [logits.data_ptr(), V, scores.data_ptr(), seen.data_ptr(), w["part_k"], w["part_a"], w["part_i"], w["part_f"], w["out_s"],
            w["out_i"], w["out_f"], w["out_k"], B, nb, V, -1, 1, prm.data_ptr(), seed.data_ptr(), step.data_ptr(), 1, pos.data_ptr(),
            pos.data_ptr(), 0, None]
    LDL, SEEN, NB, V_AT, PRM, SEED, POS, KVL, NADV = 1, 3, 13, 14, 17, 18, 21, 22, 23
    refused = [({V_AT: 32772, LDL: 40000}, ERR_UNSUPPORTED), ({V_AT: 62, LDL: 64}, ERR_UNSUPPORTED), ({NB: 0}, ERR_UNSUPPORTED),
               ({NB: 9}, ERR_UNSUPPORTED), ({V_AT: 12, NB: 8}, ERR_UNSUPPORTED), ({NADV: -1}, ERR_UNSUPPORTED),
               ({LDL: V - 4}, ERR_ARG), ({V_AT: 0}, ERR_ARG), ({PRM: None}, ERR_ARG), ({SEED: None}, ERR_ARG),
               ({POS: None}, ERR_ARG), ({KVL: None}, ERR_ARG)]
    refused += [({at: None}, ERR_ARG) for at in (0, 2, 4, 5, 6, 7, 8, 9, 10)]
    for change, rc in refused:
        args = list(good)
        for at, v in change.items():
            args[at] = v
        assert L.mh_beam_sample_topk(*args) == rc, (change, rc)
    seen_good = [seen.data_ptr(), pos.data_ptr(), torch.zeros(R, dtype=torch.long, device=DEV).data_ptr(), B, nb, V, None]
    for change, rc in (({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: None}, ERR_ARG), ({5: 0}, ERR_ARG), ({4: 0}, ERR_UNSUPPORTED),
                       ({4: 9}, ERR_UNSUPPORTED), ({3: 65536}, ERR_UNSUPPORTED)):
        args = list(seen_good)
        for at, v in change.items():
            args[at] = v
        assert L.mh_beam_seen_update(*args) == rc, (change, rc)
    torch.cuda.synchronize()
    for name, (buf, _) in dict(wins, seen=(seen_buf, seen), pos=(pbuf, pos)).items():
        if name != "pos":
            assert_untouched(buf, f"refusal {name}")
    assert pos.tolist() == [4] * R and step.tolist() == [0]
    assert L.mh_beam_sample_topk(*good) == OK and L.mh_beam_sample_topk(*[0 if i == 12 else a for i, a in enumerate(good)]) == OK
    torch.cuda.synchronize()
    # the wrappers: a short or mistyped buffer never reaches the library
    t = {k: v[1] for k, v in wins.items()}
    base = dict(params=prm, seed=seed)
    pos_args = [logits, scores, t["part_k"], t["part_a"], t["part_i"], t["part_f"], t["out_s"], t["out_i"], t["out_f"], B, nb]
    for at, bad in ((2, t["part_k"][:R * K - 1]), (4, t["part_a"]), (5, t["part_f"][:R - 1]), (8, t["out_f"][:B - 1]), (9, 3)):
        args = list(pos_args)
        args[at] = bad
        with pytest.raises(_lib.MyriadHipError):
            ops.beam_sample_topk(*args, **base)
    for kw in (dict(params=prm[:3], seed=seed), dict(params=prm, seed=None), dict(base, seen=seen[:R * 2 - 1]), dict(base, pos=pos),
               dict(base, out_k=t["out_k"][:B * K - 1])):
        with pytest.raises(_lib.MyriadHipError):
            ops.beam_sample_topk(*pos_args, **kw)
    with pytest.raises(_lib.MyriadHipError):
        ops.beam_seen_update(seen[:R * 2 - 1], pos, torch.zeros(R, dtype=torch.long, device=DEV), B, nb, V)
    with pytest.raises(_lib.MyriadHipError):
        ops.beam_seen_update(seen, pos, torch.zeros(R, dtype=I32, device=DEV), B, nb, V)


# ------------------------------------------------------------------------------------------------ beam_generate
SAMPLE = dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.95, repetition_penalty=1.3)


@pytest.fixture(scope="module")
def trap():
    lm = LlamaHIP(bf.weights(), bf.BEAM_TRAP["heads"], DEV, need_backward=False)
    lm.beam_sampling = True
    return lm


def _gen(lm, rows, nb, seed=None, use_graph=True, nrs=2, **kw):
    g = None if seed is None else torch.Generator().manual_seed(seed)
    return lm.beam_generate(bf.inputs(rows).to(DEV), nb, max_new_tokens=bf.MAX_NEW, stop_ids=bf.STOPS, eos_id=bf.EOS,
                            min_length=bf.MIN_LENGTH, length_penalty=1.0, num_return_sequences=nrs, use_graph=use_graph,
                            return_scores=True, generator=g, **kw)


def test_sampled_search_is_reproducible_per_seed_and_graph_equals_eager(trap):
    ids, sc = _gen(trap, [0, 1, 2], 3, seed=11, **SAMPLE)
    st = dict(trap.last_generate_stats)
    assert st["num_beams"] == 3 and st["beam_sampled_steps"] == st["steps"] > 0 and st["beam_host_steps"] == 0
    again, sc2 = _gen(trap, [0, 1, 2], 3, seed=11, **SAMPLE)
    assert torch.equal(ids, again) and torch.equal(sc, sc2)
    assert trap.last_generate_stats["graph_replays"] > 0
    eager, sc3 = _gen(trap, [0, 1, 2], 3, seed=11, use_graph=False, **SAMPLE)
    assert trap.last_generate_stats["graph_replays"] == 0
    assert torch.equal(ids, eager) and torch.equal(sc, sc3)              # bit for bit


def test_sampled_hypotheses_rescore_through_the_oracle(trap):
    """Every returned hypothesis teacher-forced through the oracle: each id lies in its step's kept set and the processed values
    sum to sequences_scores -- a bitmap or a KV row that followed the wrong parent would miss both."""
    rows, nb = [0, 1], 4
    ids, sc = _gen(trap, rows, nb, seed=5, **SAMPLE)
    st = trap.last_generate_stats
    fn = _oracle_fn(rows)
    inv_temp = float(np.float32(1.0 / SAMPLE["temperature"]))
    for r in range(ids.shape[0]):
        seq = ids[r, :st["lengths"][r]].tolist()
        total = torch.zeros((), dtype=F32)
        for t in range(len(seq)):
            w, _ = BR.processed(fn([(r // 2, tuple(seq[:t]))])[0], seq[:t], SAMPLE["repetition_penalty"], bf.EOS if t < bf.MIN_LENGTH else -1,
                                inv_temp, SAMPLE["top_k"], SAMPLE["top_p"])
            assert bool(torch.isfinite(w[seq[t]])), (r, t, seq)
            total = total + w[seq[t]]
        assert abs(float(total / len(seq)) - float(sc[r])) < 2e-2, (r, seq, float(total / len(seq)), float(sc[r]))


def test_penalised_deterministic_search_equals_the_reference_search(trap):
    rows, nb = [0, 1, 2], 2
    ids, sc = _gen(trap, rows, nb, repetition_penalty=1.3)
    st = trap.last_generate_stats
    assert st["beam_sampled_steps"] == st["steps"] and st["beam_host_steps"] == 0
    seqs, want = BR.beam_search(_oracle_fn(rows), len(rows), nb, bf.MAX_NEW, bf.EOS, bf.MIN_LENGTH, 1.0, bf.STOPS, penalty=1.3,
                                num_return_sequences=2)
    got = [tuple(ids[r, :st["lengths"][r]].tolist()) for r in range(ids.shape[0])]
    assert got == [tuple(s) for s in seqs], (got, seqs)                 # the fixture is decisive at every boundary (>= 0.05 nats)
    assert float((sc - want).abs().max()) < 2e-2


def test_flagged_items_are_redone_by_the_host_rule(trap, monkeypatch):
    """Every item flagged at every step (the flag forced after the launch): the search then runs on decode_host's rule alone and
    returns what the device's selection returned -- they are one rule."""
    ids, sc = _gen(trap, [0, 1], 3, seed=21, use_graph=False, **SAMPLE)
    steps = trap.last_generate_stats["steps"]
    launch = ops.beam_sample_topk

    def flagged(*args, **kw):
        out = launch(*args, **kw)
        out[2].fill_(1)
        return out
    monkeypatch.setattr(ops, "beam_sample_topk", flagged)
    again, sc2 = _gen(trap, [0, 1], 3, seed=21, use_graph=False, **SAMPLE)
    st = trap.last_generate_stats
    assert st["beam_host_steps"] == 2 * st["steps"] and st["steps"] == steps
    assert torch.equal(ids, again) and float((sc - sc2).abs().max()) < 1e-4


def test_refusals_of_the_sampled_search(trap):
    x = bf.inputs([0]).to(DEV)
    for kw, exc in ((dict(do_sample=True, top_k=0), NotImplementedError), (dict(do_sample=True, top_k=1025), NotImplementedError),
                    (dict(do_sample=True, top_k=None), NotImplementedError), (dict(do_sample=True, temperature=0.0), ValueError),
                    (dict(do_sample=True, temperature=-1.0), ValueError), (dict(repetition_penalty=0.0), ValueError)):
        with pytest.raises(exc):
            trap.beam_generate(x, 2, max_new_tokens=4, **kw)
    trap.beam_sampling = False
    try:
        for kw in (dict(do_sample=True), dict(repetition_penalty=1.3)):
            with pytest.raises(NotImplementedError):
                trap.beam_generate(x, 2, max_new_tokens=4, **kw)
    finally:
        trap.beam_sampling = True


def test_default_beam_search_issues_the_launches_it_did(monkeypatch):
    """The switch on, no new argument: the launch list and the ids of tests/golden/decode_launches.json's beam case, noted as
    tests/test_decode_launches_gpu.py notes them."""
    from tests import test_decode_launches_gpu as T
    lm = T._chain_model(T.gu.decode_chain_weights())
    lm.beam_sampling = True
    x = T._rows(1)
    lib, calls = _lib.load(), []
    ops.ensure_workspace(T.DEV)                                          # once per process: not a call of any case
    proxy = T._Noting(lib, calls)
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    ids = lm.beam_generate(x, num_beams=2, max_new_tokens=5, stop_ids=((835,),), eos_id=2, min_length=1, use_graph=False)
    T._check("beam2", calls, ids.tolist())
    del calls[:]
    ids = lm.beam_generate(x, num_beams=2, max_new_tokens=5, stop_ids=((835,),), eos_id=2, min_length=1, use_graph=False,
                           do_sample=False, repetition_penalty=1.0, top_k=7, top_p=0.5, temperature=2.0)
    assert "mh_beam_sample_topk" not in calls and "mh_beam_seen_update" not in calls and "mh_beam_topk" in calls
    del calls[:]
    lm.beam_generate(x, num_beams=2, max_new_tokens=5, stop_ids=((835,),), eos_id=2, min_length=1, use_graph=False, do_sample=True)
    assert "mh_beam_sample_topk" in calls and "mh_beam_seen_update" in calls and "mh_beam_topk" not in calls


# ------------------------------------------------------------------------------------------------ generate / Chat.answer
def test_generate_and_chat_take_beam_sampling_behind_the_switch(model):
    from myriad_amd.chat import CONV_VISION, Chat
    samples = _batch(2, train=False, seed=5)
    kw = dict(max_new_tokens=8, min_length=1, num_beams=3, do_sample=True, top_p=0.9, temperature=1.0, repetition_penalty=1.2)
    model.eval()
    prev = model.llama.beam_sampling
    try:
        model.llama.beam_sampling = False
        with pytest.raises(NotImplementedError):
            model.generate(samples, **kw)
        model.llama.beam_sampling = True
        outs = [model.generate(samples, generator=torch.Generator().manual_seed(s), **kw)["token_ids"] for s in (3, 3, 4, 5, 6)]
        st = dict(model.last_generate_stats)
        assert st["num_beams"] == 3 and st["beam_sampled_steps"] > 0 and st["beam_host_steps"] == 0
        assert torch.equal(outs[0], outs[1])
        assert any(o.shape != outs[0].shape or not torch.equal(o, outs[0]) for o in outs[2:])     # flat logits: another seed differs
        with pytest.raises(NotImplementedError):
            model.generate(samples, **dict(kw, top_k=0))
        with pytest.raises(NotImplementedError):
            model.generate(samples, output_scores=True, **kw)
        turns = []
        for _ in range(2):
            chat, conv, imgs = Chat(model, device=DEV), CONV_VISION.copy(), []
            chat.upload_img(samples["image"][:1], conv, imgs, anomaly_maps=samples["anomaly_maps"][:1])
            chat.ask("Is there a defect?", conv)
            chat.answer(conv, imgs, max_new_tokens=8, num_beams=2, repetition_penalty=1.2, generator=torch.Generator().manual_seed(9))
            turns.append(chat.last_token_ids.clone())
            cs = chat.last_stats
            assert cs["num_beams"] == 2 and cs["beam_sampled_steps"] > 0 and cs["beam_host_steps"] == 0
            assert cs["full_reprefill_reason"] == "num_beams"
        assert torch.equal(turns[0], turns[1])
    finally:
        model.llama.beam_sampling = prev
        model.train()
