"""Device sampling, the repetition penalty and min_length in decode slots: the per-row ("slots") forms of the sampler, the greedy
pick, the penalty and the bookkeeping launch against tests/sampling_ref.py and the uniform entry points, and the slot engine
(LlamaHIP.slot_decoder, MyriadHIP.generate_stream, eval_aqa --slots) with one random stream per request against batch-1 decoding."""
import itertools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from myriad_amd.llama import LlamaHIP  # noqa: E402
from tests import sampling_ref as S  # noqa: E402
from tests.test_decode_slots_gpu import _ragged_batches, _requests  # noqa: E402
from tests.test_entrypoints_gpu import DEV, _batch, fx, model  # noqa: E402,F401
from tests.test_sampling_gpu import SEED, _tiny  # noqa: E402

I32 = torch.int32
EOS = 2
LIVE = [1, 0, 1, 1, 0, 1]
POISON = 123.0


def _i32(v):
    return torch.tensor(v, dtype=I32, device=DEV)


def _out(R_):
    """The sampler's five outputs, each with two poisoned entries behind its R_ rows: (whole buffers, the [:R_] views)."""
    full = dict(out=torch.full((R_ + 2,), -77, dtype=torch.long, device=DEV), mar=torch.full((R_ + 2,), POISON, device=DEV),
                pmx=torch.full((R_ + 2,), POISON, device=DEV), kept=torch.full((R_ + 2,), -99, dtype=I32, device=DEV),
                u=torch.full((R_ + 2,), POISON, device=DEV))
    return full, {k: v[:R_] for k, v in full.items()}


def _poisoned(full, rows=0):
    """Every entry from `rows` on still holds its poison."""
    want = dict(out=-77, mar=POISON, pmx=POISON, kept=-99, u=POISON)
    return all(bool((v[rows:] == want[k]).all()) for k, v in full.items())


def _bordered_logits(R_, V, g):
    """[R, V] f32 view of a NaN-filled [R, ldl] buffer, ldl = V rounded up to 4 plus 4: every row ends in NaN columns."""
    ldl = (V + 3) // 4 * 4 + 4
    full = torch.full((R_, ldl), float("nan"))
    full[:, :V] = torch.randn(R_, V, generator=g) * 3.0
    full = full.to(DEV)
    return full, full[:, :V]


def _bitmap(seen_ids, V):
    bits = np.zeros((len(seen_ids), (V + 31) // 32), dtype=np.uint32)
    for r, ids in enumerate(seen_ids):
        for i in ids:
            bits[r, i // 32] |= np.uint32(1 << (i % 32))
    return torch.from_numpy(bits.view(np.int32)).to(DEV)


def _prm(inv_temp, top_p, top_k, penalty, min_length, eos_id):
    return torch.tensor([inv_temp, top_p, float(top_k), penalty, float(min_length), float(eos_id)], dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------------ kernels
def test_slot_sampler_equals_the_reference_over_the_grid():
    """R = 6 rows, two of them idle.  Live rows: u, the penalised logits, kept and out against tests/sampling_ref.py with the row's
    own seed, step gen[r] and ban (eos while gen[r] < min_length); margin and p_max against mh_argmax_pmax_rows on the same row and
    ban.  Idle rows: logits, bitmap and outputs untouched.  On this grid the reference marks 1 of the 144 live rows `near`, 58 have
    the ban on and none overflows the candidate cap (computed on the CPU from this recipe)."""
    g = torch.Generator().manual_seed(11)
    extra = list(itertools.product((0.7, 1.0, 1.3), (1.0, 1.3), (1, 3)))               # (T, penalty, min_length) cycled over the grid
    R_, live = len(LIVE), _i32(LIVE)
    rows = near = banned = 0
    for n, (V, top_k, top_p) in enumerate(itertools.product((32000, 1000, 999), (1, 50, 1024), (0.01, 0.5, 0.9, 1.0))):
        T, pen, min_length = extra[n % len(extra)]
        full, x = _bordered_logits(R_, V, g)
        seen_ids = [torch.randint(0, V, (6,), generator=g).tolist() for _ in range(R_)]
        seen = _bitmap(seen_ids, V)
        gen_h = [(r + n) % 5 for r in range(R_)]
        seed_h = [SEED + 97 * n + r for r in range(R_)]
        prm = _prm(1.0 / T, top_p, top_k, pen, min_length, EOS)
        full0, seen0 = full.cpu(), seen.cpu()
        if pen != 1.0:
            ops.repetition_penalty_rows_slots(x, seen, None, prm[3:], live)
        bf, b = _out(R_)
        ops.sample_rows_slots(x, b["out"], b["mar"], b["pmx"], b["kept"], prm, torch.tensor(seed_h, dtype=torch.long, device=DEV),
                              _i32(gen_h), live, u_out=b["u"])
        torch.cuda.synchronize()
        assert _poisoned(bf, R_), n
        full1 = full.cpu()
        assert torch.equal(seen.cpu(), seen0)                                       # no prev_ids: no bitmap changes at all
        for r in range(R_):
            if not LIVE[r]:
                assert torch.equal(full1[r].view(I32), full0[r].view(I32)), (n, r)  # bit for bit, the NaN border included
                assert int(b["out"][r]) == -1 and int(b["kept"][r]) == 0 and float(b["mar"][r]) == 0 and float(b["pmx"][r]) == 0
                assert float(b["u"][r]) == POISON
                continue
            assert bool(torch.isnan(full1[r, V:]).all())
            ban = EOS if gen_h[r] < min_length else -1
            banned += ban >= 0
            u = S.uniform(seed_h[r], gen_h[r], 0)
            assert float(b["u"][r]) == u, (n, r)                                    # the host Philox, bit for bit
            row = full1[r, :V]
            assert torch.allclose(row, S.penalize(full0[r, :V], seen_ids[r], pen), rtol=1e-6, atol=0)
            _, am = _out(1)
            ops.argmax_pmax_rows(x[r:r + 1], am["out"], am["mar"], am["pmx"], ban_id=ban, inv_temp=1.0 / T)
            assert torch.equal(b["mar"][r:r + 1], am["mar"]) and torch.equal(b["pmx"][r:r + 1], am["pmx"]), (n, r)
            ref = S.sample_row(row, top_k, top_p, 1.0 / T, ban, u=u)
            assert ref["kept"] != -1
            if ref["near"]:
                near += 1
                continue
            assert int(b["kept"][r]) == ref["kept"], (n, r)
            assert int(b["out"][r]) == ref["out"], (n, r, top_k, top_p, T)
            rows += 1
    print("slot sampler grid: compared", rows, "near", near, "banned", banned)
    assert rows + near == 144
    assert near <= 0.02 * (rows + near), (near, rows)


def test_slot_draw_is_the_uniform_entry_for_row_0_with_the_same_seed():
    """Row r at (seed[r], gen[r]) draws what mh_sample_rows draws for row 0 of a one-row call with that seed at t = gen[r]; the
    greedy pick with the per-row ban is mh_argmax_pmax_rows with that ban.  A tied top-k set past the cap still reports -1."""
    V, R_ = 1000, 4
    g = torch.Generator().manual_seed(2)
    _, x = _bordered_logits(R_, V, g)
    gen_h, seed_h = [0, 3, 1, 7], [SEED + 5, SEED, 77, 2**63 - 1]
    prm = _prm(1.0 / 0.8, 0.9, 50, 1.0, 2, EOS)
    _, b = _out(R_)
    ops.sample_rows_slots(x, b["out"], b["mar"], b["pmx"], b["kept"], prm, torch.tensor(seed_h, dtype=torch.long, device=DEV),
                          _i32(gen_h), None, u_out=b["u"])                          # live = None: every row is live
    _, p = _out(R_)
    ops.argmax_pmax_rows_slots(x, p["out"], p["mar"], p["pmx"], prm, _i32(gen_h), _i32([1, 1, 0, 1]))
    for r in range(R_):
        ban = EOS if gen_h[r] < 2 else -1
        _, one = _out(1)
        ops.sample_rows(x[r:r + 1], one["out"], one["mar"], one["pmx"], one["kept"], prm[:4],
                        torch.tensor([seed_h[r]], dtype=torch.long, device=DEV), ban_id=ban, t_add=gen_h[r], u_out=one["u"])
        for k in one:
            assert torch.equal(b[k][r:r + 1], one[k]), (k, r)
        if r == 2:
            assert int(p["out"][r]) == -1 and float(p["mar"][r]) == 0 and float(p["pmx"][r]) == 0
            continue
        _, am = _out(1)
        ops.argmax_pmax_rows(x[r:r + 1], am["out"], am["mar"], am["pmx"], ban_id=ban, inv_temp=1.0 / 0.8)
        for k in ("out", "mar", "pmx"):
            assert torch.equal(p[k][r:r + 1], am[k]), (k, r)
    # 1,500 tied maxima: more than the 1,024 candidates the sort takes
    V = 4000
    y = torch.randn(2, V, generator=g)
    y[0, :1500] = 9.0
    y = y.to(DEV)
    _, t = _out(2)
    ops.sample_rows_slots(y, t["out"], t["mar"], t["pmx"], t["kept"], prm, torch.tensor([7, 8], dtype=torch.long, device=DEV),
                          _i32([4, 4]), _i32([1, 1]))
    assert int(t["kept"][0]) == -1 and int(t["out"][0]) == 0 and 1 <= int(t["kept"][1]) <= 50


def test_slot_penalty_marks_prev_ids_of_live_rows_only():
    V, R_ = 1000, 4
    x0 = torch.randn(R_, V, generator=torch.Generator().manual_seed(4)) * 2.0
    seen = torch.zeros((R_, (V + 31) // 32), dtype=I32, device=DEV)
    pen = torch.tensor([1.3], device=DEV)
    history, live = [[17, 999], [17, 17], [0, 640], [5, 31]], [1, 0, 1, 1]
    for t in range(2):
        x = x0.to(DEV)
        ops.repetition_penalty_rows_slots(x, seen, torch.tensor([h[t] for h in history], device=DEV), pen, _i32(live))
    for r in range(R_):
        bits = seen[r].cpu().numpy().view(np.uint32)
        marked = {w * 32 + b for w in range(len(bits)) for b in range(32) if bits[w] >> b & 1}
        if live[r]:
            assert torch.allclose(x[r].cpu(), S.penalize(x0[r], history[r], 1.3), rtol=1e-6, atol=0)
            assert marked == set(history[r])
        else:
            assert torch.equal(x[r].cpu(), x0[r]) and not marked


def test_masked_advance_with_kept_and_gen_is_exact():
    R_, live = 5, [1, 0, 1, 1, 0]
    g = torch.Generator().manual_seed(5)
    x = dict(nxt=torch.randint(0, 32000, (R_,), generator=g), mar=torch.rand(R_, generator=g), pmx=torch.rand(R_, generator=g),
             kept=torch.tensor([3, 9, -1, 1024, 1], dtype=I32), ids=torch.randint(0, 32000, (R_,), generator=g),
             pos=torch.randint(1, 200, (R_,), generator=g).to(I32), kvl=torch.randint(1, 200, (R_,), generator=g).to(I32),
             gen=torch.randint(1, 90, (R_,), generator=g).to(I32))
    for with_kept in (True, False):
        d = {k: v.to(DEV) for k, v in x.items()}
        rec = torch.full((4 * R_ + 3,), 7.0, device=DEV)
        step = _i32([4])
        ops.decode_advance_kept_rows(d["nxt"], d["mar"], d["pmx"], d["kept"] if with_kept else None, rec[:4 * R_].view(4, R_), d["ids"],
                                     step, d["pos"], d["kvl"], d["gen"], _i32(live))
        assert rec[4 * R_:].tolist() == [7.0] * 3
        rc = rec[:4 * R_].view(4, R_).cpu()
        for r in range(R_):                                          # the kernel, restated
            want = [float(x["nxt"][r]), float(x["mar"][r]), float(x["pmx"][r]), float(x["kept"][r]) if with_kept else 0.0]
            assert rc[:, r].tolist() == (want if live[r] else [-1.0, 0.0, 0.0, 0.0]), r
            assert int(d["ids"][r]) == int(x["nxt"][r] if live[r] else x["ids"][r])
            for k in ("pos", "kvl", "gen"):
                assert int(d[k][r]) == int(x[k][r]) + live[r], (k, r)
        assert int(step) == 5
        assert all(torch.equal(d[k].cpu(), x[k]) for k in ("nxt", "mar", "pmx", "kept"))


def test_slot_entries_refuse_bad_arguments_and_launch_nothing():
    R_, V = 2, 1000
    x = torch.zeros((R_, V), device=DEV)
    seed, gen, live, prm = torch.zeros(R_, dtype=torch.long, device=DEV), _i32([0] * R_), _i32([1] * R_), _prm(1.0, 0.9, 50, 1.0, 1, EOS)
    bf, b = _out(R_)

    def sample(logits=x, **kw):
        a = dict(out=b["out"], mar=b["mar"], pmx=b["pmx"], kept=b["kept"], prm=prm, seed=seed, gen=gen)
        a.update(kw)
        ops.sample_rows_slots(logits, a["out"], a["mar"], a["pmx"], a["kept"], a["prm"], a["seed"], a["gen"], live, u_out=b["u"])

    def pick(logits=x, **kw):
        a = dict(out=b["out"], mar=b["mar"], pmx=b["pmx"], prm=prm, gen=gen)
        a.update(kw)
        ops.argmax_pmax_rows_slots(logits, a["out"], a["mar"], a["pmx"], a["prm"], a["gen"], live)

    for k in ("out", "mar", "pmx", "kept", "prm", "seed", "gen"):
        with pytest.raises(_lib.MyriadHipError, match="MH_ERR_ARG"):
            sample(**{k: None})
    for k in ("out", "mar", "pmx", "prm", "gen"):
        with pytest.raises(_lib.MyriadHipError, match="MH_ERR_ARG"):
            pick(**{k: None})
    wide = torch.zeros((R_, 32772), device=DEV)                                     # V > 32768
    odd = torch.zeros((R_, V + 2), device=DEV)[:, :V]                               # ldl % 4 != 0
    for fn in (sample, pick):
        for bad in (wide, odd):
            with pytest.raises(_lib.MyriadHipError, match="MH_ERR_UNSUPPORTED"):
                fn(logits=bad)
    seen = torch.zeros((R_, 32), dtype=I32, device=DEV)
    for a in ((x, None, None, prm[3:], live), (x, seen, None, None, live), (x, seen, None, prm[3:], None)):
        with pytest.raises(_lib.MyriadHipError, match="MH_ERR_ARG"):
            ops.repetition_penalty_rows_slots(*a)
    rec, step = torch.full((4, R_), 7.0, device=DEV), _i32([0])
    good = [b["out"], b["mar"], b["pmx"], b["kept"], rec, seed.clone(), step, _i32([3] * R_), _i32([4] * R_), gen, live]
    for i in (0, 1, 2, 4, 5, 6, 7, 8, 9, 10):                                       # kept (3) may be null
        with pytest.raises(_lib.MyriadHipError, match="MH_ERR_ARG"):
            ops.decode_advance_kept_rows(*[None if j == i else a for j, a in enumerate(good)])
    torch.cuda.synchronize()
    assert _poisoned(bf) and bool((rec == 7.0).all()) and int(step) == 0 and not bool(seen.any())


# ------------------------------------------------------------------------------------------------ engine, tiny LLaMA
@pytest.fixture(scope="module")
def lm():
    gd, sd, heads = _tiny()
    m = LlamaHIP(sd, heads, DEV, need_backward=False)
    m.device_sampling = True
    return m


def _ids(results):
    return {i: ids.tolist() for i, ids, _ in results}


def _alone(lm, reqs, gen_seed=None, **kw):
    """Every request through greedy_generate at batch 1, in input order, one generator across the calls."""
    g = None if gen_seed is None else torch.Generator().manual_seed(gen_seed)
    return [lm.greedy_generate(x[None].to(DEV), generator=g, **kw)[0].tolist() for x in reqs]


def test_sampled_slots_equal_batch_1_decoding_with_the_same_seeds(lm):
    reqs = _requests([3, 9, 5, 7, 4], lm.D, 21)
    dec = lm.slot_decoder(1, 64)
    # the ground the comparison stands on: at one slot the step's logits are batch-1 decoding's, bit for bit
    gkw = dict(max_new_tokens=10, stop_ids=(), eos_id=-5, min_length=0)
    got = {i: (ids, mar) for i, ids, mar in dec.run(reqs, **gkw)}
    for i, x in enumerate(reqs):
        ids, mar = lm.greedy_generate(x[None].to(DEV), return_margins=True, **gkw)
        assert torch.equal(got[i][0], ids[0]) and torch.equal(got[i][1], mar[0]), i
    kw = dict(max_new_tokens=10, stop_ids=(), do_sample=True, top_p=0.9)
    out = _ids(dec.run(reqs, generator=torch.Generator().manual_seed(5), **kw))
    st = dict(dec.last_stats)
    want = _alone(lm, reqs, gen_seed=5, **kw)
    for i in range(len(reqs)):
        assert out[i] == want[i], (i, out[i], want[i])
    assert st["host_sampled_rows"] == 0 and st["device_sampled_rows"] == sum(len(w) for w in want) > 0
    assert len({tuple(w) for w in want}) > 1 and out != _ids(dec.run(reqs, **gkw))  # draws, not the arg-max


def test_a_sampled_request_does_not_depend_on_its_neighbours(lm):
    reqs = _requests([3, 8, 5, 9, 4, 7, 6], lm.D, 22)
    seeds = [SEED + 1000 * i for i in range(len(reqs))]
    dec = lm.slot_decoder(4, 64)
    kw = dict(max_new_tokens=10, stop_ids=(), do_sample=True, top_p=0.9)
    out = _ids(dec.run(reqs, seeds=seeds, **kw))
    assert len(out) == len(reqs)
    for i, x in enumerate(reqs):
        assert _ids(dec.run([x], seeds=[seeds[i]], **kw))[0] == out[i], i
    back = _ids(dec.run(reqs[::-1], seeds=seeds[::-1], **kw))
    assert [back[len(reqs) - 1 - i] for i in range(len(reqs))] == [out[i] for i in range(len(reqs))]
    a = _ids(dec.run(reqs, generator=torch.Generator().manual_seed(3), **kw))
    assert a == _ids(dec.run(reqs, generator=torch.Generator().manual_seed(3), **kw))
    assert a != _ids(dec.run(reqs, generator=torch.Generator().manual_seed(4), **kw))
    assert dec.last_stats["host_sampled_rows"] == 0
    with pytest.raises(ValueError):
        list(dec.run(reqs, seeds=seeds[:3], **kw))
    with pytest.raises(ValueError):
        list(dec.run(reqs, seeds=seeds, max_new_tokens=4))           # greedy: there is no stream to seed


def test_a_sampled_run_stays_on_the_device_in_one_graph(lm):
    reqs = _requests([4, 7, 5, 6, 3], lm.D, 23)
    dec = lm.slot_decoder(2, 64)
    kw = dict(max_new_tokens=8, stop_ids=(), do_sample=True)
    list(dec.run(reqs, top_p=0.9, repetition_penalty=1.1, generator=torch.Generator().manual_seed(1), **kw))
    st = dict(dec.last_stats)
    assert st["graph_replays"] >= st["steps"] - 2 and st["graph_replays"] > 0 and st["host_sampled_rows"] == 0
    captures = dec.graph_captures
    assert captures == 1
    list(dec.run(reqs, top_p=0.5, temperature=1.7, top_k=7, min_length=3, repetition_penalty=1.3,
                 generator=torch.Generator().manual_seed(1), **kw))
    assert dec.graph_captures == captures and dec.last_stats["graph_replays"] == dec.last_stats["steps"]
    assert dec.ws["prm"].tolist() == pytest.approx([1 / 1.7, 0.5, 7.0, 1.3, 3.0, 2.0])


def test_penalised_greedy_slots_equal_batch_1_and_the_bitmap_is_cleared_at_a_refill(lm):
    reqs = _requests([5, 8, 4], lm.D, 24)
    kw = dict(max_new_tokens=10, stop_ids=(), eos_id=-5, min_length=0, repetition_penalty=1.3)
    dec = lm.slot_decoder(1, 64)
    out = _ids(dec.run(reqs, **kw))
    want = _alone(lm, reqs, **kw)
    plain = _alone(lm, reqs, **dict(kw, repetition_penalty=1.0))
    assert [out[i] for i in range(3)] == want and want != plain
    twice = _ids(dec.run([reqs[1], reqs[1]], **kw))
    assert twice[0] == twice[1] == want[1]
    lm.device_sampling = False
    try:
        with pytest.raises(NotImplementedError, match="device sampling switch"):
            list(dec.run(reqs, **kw))
    finally:
        lm.device_sampling = True


@pytest.mark.parametrize("sampled", [False, True])
def test_min_length_is_a_per_row_ban(lm, sampled):
    reqs = _requests([6, 3, 9, 5, 7], lm.D, 25)
    dec = lm.slot_decoder(4, 64)
    kw = dict(max_new_tokens=8, stop_ids=())
    if sampled:
        kw.update(do_sample=True, top_p=0.9)
    run = lambda **k: _ids(dec.run(reqs, generator=torch.Generator().manual_seed(6), **kw, **k))   # noqa: E731
    free = run(eos_id=-5)
    j = next(i for i in range(len(reqs)) if free[i][1] != free[i][0])
    eos = free[j][1]                                                 # declared EOS: what request j produced at index 1
    if not sampled:                                                  # (a ban at index 0 moves no arg-max that is not EOS itself)
        assert run(eos_id=eos, min_length=1)[j] == free[j][:2]
    out = run(eos_id=eos, min_length=3)
    want = _alone(lm, reqs, gen_seed=6, eos_id=eos, min_length=3, **kw)
    for i in range(len(reqs)):                                       # request 4 starts in a refilled slot beside rows past the ban
        assert out[i] == want[i], (i, out[i], want[i])
        assert eos not in out[i][:3]
    assert len(out[j]) >= 3 and dec.last_stats["host_sampled_rows"] == 0
    if sampled:                                                      # the host-draw path takes the same per-row ban
        lm.device_sampling = False
        try:
            host = run(eos_id=eos, min_length=3)
            assert all(eos not in host[i][:3] for i in range(len(reqs))) and dec.last_stats["device_sampled_rows"] == 0
        finally:
            lm.device_sampling = True


def test_packed_prefill_takes_its_first_picks_from_one_sampler_launch(lm):
    reqs = _requests([3, 8, 5, 9, 4, 7, 6], lm.D, 26)
    dec = lm.slot_decoder(4, 64)
    kw = dict(max_new_tokens=8, stop_ids=(), do_sample=True, top_p=0.9, prefill_batch=4, refill_min=2)
    a = _ids(dec.run(reqs, generator=torch.Generator().manual_seed(8), **kw))
    st = dict(dec.last_stats)
    assert len(a) == 7 and st["prefills"] == 7 and st["prefill_passes"] < st["prefills"]
    assert st["host_sampled_rows"] == 0 and st["device_sampled_rows"] == sum(len(v) for v in a.values())
    assert a == _ids(dec.run(reqs, generator=torch.Generator().manual_seed(8), **kw))
    assert a != _ids(dec.run(reqs, generator=torch.Generator().manual_seed(9), **kw))


# ------------------------------------------------------------------------------------------------ public surface
def test_generate_stream_samples_on_the_device_reproducibly(model):
    model.eval()
    prev = model.llama.device_sampling
    try:
        model.llama.device_sampling = True
        batches = _ragged_batches(model, (2, 3), seed=5)
        kw = dict(max_new_tokens=8, stop_ids=((835,), (2277, 29937)), do_sample=True, top_p=0.9, repetition_penalty=1.05,
                  min_length=2)
        runs = []
        for gs in (1, 1, 2):
            outs = list(model.generate_stream(iter(batches), slots=2, generator=torch.Generator().manual_seed(gs), **kw))
            assert [o["index"] for o in outs] == [0, 1, 2, 3, 4]
            st = model.last_generate_stats
            assert st["host_sampled_rows"] == 0 and st["device_sampled_rows"] == sum(len(o["token_ids"]) for o in outs)
            runs.append([o["token_ids"].tolist() for o in outs])
        assert runs[0] == runs[1] and runs[0] != runs[2]
        assert all(len(ids) >= 2 for ids in runs[0])
        seeded = [[o["token_ids"].tolist() for o in model.generate_stream(iter(batches), slots=2, seeds=range(10, 15), **kw)]
                  for _ in range(2)]
        assert seeded[0] == seeded[1] and len(seeded[0]) == 5                       # explicit seeds: no generator in sight
        model.llama.device_sampling = False
        with pytest.raises(NotImplementedError):
            model.generate_stream(iter(batches), slots=2, **kw)
    finally:
        model.llama.device_sampling = prev
        model.train()


def test_eval_entry_point_streams_through_slots_with_device_sampling(fx, tmp_path, monkeypatch):
    import eval_aqa
    monkeypatch.setenv("MYRIAD_DEVICE_SAMPLING", "1")
    path, records = eval_aqa.main(["--cfg-path", fx["eval_yaml"], "--dataset", "synthetic", "--bs", "2", "--limit", "2", "--slots", "2",
                                   "--out", str(tmp_path / "res.jsonl")])
    rows = [json.loads(ln) for ln in open(path)]
    assert len(rows) == len(records) == 4
