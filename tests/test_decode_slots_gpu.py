"""Decode slots on the HIP decode path: the per-row token-step attention (mh_attn_decode_rope_rows) and the masked bookkeeping
launch (mh_decode_advance_rows) at their edges, both replayed from one graph while the host moves the per-row state, and the slot
engine (LlamaHIP.slot_decoder, MyriadHIP.generate_stream, eval_aqa --slots) against the batched and the batch-1 decode paths on
the model built from the reference's on-disk files (the fixtures of tests/test_entrypoints_gpu.py)."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import ops  # noqa: E402
from myriad_amd.llama import SlotScheduler  # noqa: E402
from oracle import myriad_ref as R  # noqa: E402
from tests import fp8_ref as F  # noqa: E402
from tests import golden_utils as gu  # noqa: E402
from tests.test_entrypoints_gpu import DEV, _batch, fx, model  # noqa: E402,F401

BF16 = torch.bfloat16
I32 = torch.int32


# ------------------------------------------------------------------ kernels
def _tables(T, D):
    fr = torch.arange(T).float()[:, None] * (1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D)))[None]
    return fr.cos().contiguous(), fr.sin().contiguous()


def _rotate(x, c, s):
    """rotate-half in fp32 of a bf16 [.., D] head, rounded to bf16 once (modeling_llama.py:109-123)."""
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h].float(), x[..., h:].float()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(BF16)


def _reference(qkv, cache_after, pos, kv_len, cos, sin, H, D, scale):
    """fp64 attention of the rotated (bf16-rounded) query over the first kv_len[b] rows of the cache after the append (the helper
    of tests/test_chat_gpu.py, restated)."""
    B, W = qkv.shape[0], H * D
    out = torch.zeros((B, W), dtype=torch.float64)
    for b in range(B):
        p = int(pos[b])
        q = _rotate(qkv[b, :W].view(H, D), cos[p], sin[p]).double()
        n = int(kv_len[b])
        k = cache_after[b, :n, :W].view(n, H, D).double()
        v = cache_after[b, :n, W:].view(n, H, D).double()
        s = torch.einsum("hd,nhd->hn", q, k) * scale
        out[b] = torch.einsum("hn,nhd->hd", torch.softmax(s, -1), v).reshape(W)
    return out


def _i32(v):
    return torch.tensor(v, dtype=I32, device=DEV)


@pytest.mark.parametrize("H,D", [(2, 16), (32, 128)])
def test_rows_attention_at_its_edges(H, D):
    """Rows at the first cache row, inside a 64-key pass, at its last key and at the cache's last row; one idle row among them."""
    torch.manual_seed(11 * H + D)
    B, T, W = 4, 256, H * D
    scale = 1.0 / D ** 0.5
    cos, sin = _tables(T, D)
    pos_h, live_h = [0, 5, 63, 255], [1, 1, 0, 1]
    kvl_h = [p + 1 for p in pos_h]
    qkv0 = (torch.randn(B, 3 * W) * 0.7).to(BF16)
    cache0 = (torch.randn(B, T, 2 * W) * 0.7).to(BF16)              # every row poisoned: a read past kv_len[b] shows
    dcos, dsin = cos.to(DEV), sin.to(DEV)
    runs = []
    for _ in range(2):
        q, c = qkv0.to(DEV), cache0.to(DEV)
        o = ops.attn_decode_rope_rows(q, c, _i32(pos_h), _i32(kvl_h), _i32(live_h), dcos, dsin, H, D, scale)
        torch.cuda.synchronize()
        runs.append((o.cpu(), q.cpu(), c.cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)                                     # run to run: the same bits
    o, q, c = runs[0]
    for b in range(B):
        if not live_h[b]:
            assert torch.equal(q[b], qkv0[b]) and torch.equal(c[b], cache0[b])
            assert int((o[b].view(torch.int16) != 0).sum()) == 0     # +0.0 exactly
            continue
        q1, c1 = qkv0[b:b + 1].to(DEV), cache0[b:b + 1].to(DEV)
        p1 = _i32([pos_h[b]])
        o1 = ops.attn_decode_rope(q1, c1, p1, p1, _i32([kvl_h[b]]), dcos, dsin, H, D, scale)
        assert torch.equal(o[b], o1.cpu()[0]), b                     # the row alone through the uniform entry: the same bits
        assert torch.equal(q[b], q1.cpu()[0]), b
        assert torch.equal(c[b, pos_h[b]], c1.cpu()[0, pos_h[b]]), b
        other = torch.ones(T, dtype=torch.bool)
        other[pos_h[b]] = False
        assert torch.equal(c[b, other], cache0[b, other]), b
    livei = [b for b in range(B) if live_h[b]]
    ref = _reference(qkv0, c, pos_h, kvl_h, cos, sin, H, D, scale)[livei]
    err = (o[livei].double() - ref).abs()
    # bf16 output: half an ulp (2^-9 relative) of the value, plus fp32 accumulation over <= 256 keys
    bound = ref.abs() * 2.0 ** -8 + 1e-4
    print("rows attention: max err", float(err.max()), "max err - bound", float((err - bound).max()))
    assert bool((err <= bound).all()), float((err - bound).max())
    # every row live at one position: the uniform entry at B = 4
    p4, k4 = _i32([37] * B), _i32([38] * B)
    qa, ca, qb, cb = qkv0.to(DEV), cache0.to(DEV), qkv0.to(DEV), cache0.to(DEV)
    oa = ops.attn_decode_rope_rows(qa, ca, p4, k4, _i32([1] * B), dcos, dsin, H, D, scale)
    ob = ops.attn_decode_rope(qb, cb, p4, p4, k4, dcos, dsin, H, D, scale)
    assert torch.equal(oa, ob) and torch.equal(qa, qb) and torch.equal(ca, cb)


def _advance_inputs(R_):
    g = torch.Generator().manual_seed(5)
    return dict(nxt=torch.randint(0, 32000, (R_,), generator=g), mar=torch.rand(R_, generator=g), pmx=torch.rand(R_, generator=g),
                ids=torch.randint(0, 32000, (R_,), generator=g), pos=torch.randint(1, 200, (R_,), generator=g).to(I32),
                kvl=torch.randint(1, 200, (R_,), generator=g).to(I32))


def _run_advance(x, live, R_):
    d = {k: v.to(DEV) for k, v in x.items()}
    rec = torch.full((3, R_), 7.0, device=DEV)
    step = _i32([4])
    if live is None:
        ops.decode_advance(d["nxt"], d["mar"], d["pmx"], rec, d["ids"], step, d["pos"], d["kvl"])
    else:
        ops.decode_advance_rows(d["nxt"], d["mar"], d["pmx"], rec, d["ids"], step, d["pos"], d["kvl"], _i32(live))
    return [t.cpu() for t in (rec, d["ids"], d["pos"], d["kvl"], step)]


def test_masked_advance_is_exact():
    R_, live = 5, [1, 0, 1, 1, 0]
    x = _advance_inputs(R_)
    rec, ids, pos, kvl, step = _run_advance(x, live, R_)
    for r in range(R_):                                              # the kernel, restated
        want = [float(x["nxt"][r]), float(x["mar"][r]), float(x["pmx"][r])] if live[r] else [-1.0, 0.0, 0.0]
        assert rec[:, r].tolist() == want, r
        assert int(ids[r]) == int(x["nxt"][r] if live[r] else x["ids"][r])
        assert int(pos[r]) == int(x["pos"][r]) + live[r] and int(kvl[r]) == int(x["kvl"][r]) + live[r]
    assert int(step) == 5
    for a, b in zip(_run_advance(x, [1] * R_, R_), _run_advance(x, None, R_)):
        assert torch.equal(a, b)                                     # finite, non-zero floats: equal values are equal bits


def test_rows_step_replays_from_a_graph_while_the_host_moves_the_row_state():
    torch.manual_seed(3)
    B, H, D, T = 3, 4, 32, 128
    W = H * D
    cos, sin = (t.to(DEV) for t in _tables(T, D))
    cache = (torch.randn(B, T, 2 * W, device=DEV) * 0.7).to(BF16)
    qkv0 = (torch.randn(B, 3 * W, device=DEV) * 0.7).to(BF16)
    st = dict(qkv=qkv0.clone(), pos=_i32([0] * B), kvl=_i32([0] * B), live=_i32([0] * B), step=_i32([0]),
              nxt=torch.arange(B, device=DEV) + 100, mar=torch.rand(B, device=DEV), pmx=torch.rand(B, device=DEV),
              rec=torch.zeros((3, B), device=DEV), ids=torch.zeros((B,), dtype=torch.long, device=DEV),
              out=torch.zeros((B, W), dtype=BF16, device=DEV))

    def step(s, c):
        s["out"].copy_(ops.attn_decode_rope_rows(s["qkv"], c, s["pos"], s["kvl"], s["live"], cos, sin, H, D, 0.17))
        ops.decode_advance_rows(s["nxt"], s["mar"], s["pmx"], s["rec"], s["ids"], s["step"], s["pos"], s["kvl"], s["live"])

    def put(pos, live):
        st["pos"].copy_(_i32(pos))
        st["kvl"].copy_(_i32([p + 1 for p in pos]))
        st["live"].copy_(_i32(live))
        st["qkv"].copy_(qkv0)

    put([9, 20, 64], [1, 1, 1])
    warm = {k: v.clone() for k, v in st.items()}
    step(warm, cache.clone())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(st, cache)
    # all live; row 1 finishes; row 1 is refilled at a smaller position while row 0 runs on; the last cache row
    for pos, live in (([9, 20, 64], [1, 1, 1]), ([10, 21, 65], [1, 0, 1]), ([11, 4, 66], [1, 1, 1]), ([12, 5, 127], [0, 1, 1])):
        put(pos, live)
        eager = {k: v.clone() for k, v in st.items()}
        eager_c = cache.clone()
        g.replay()
        step(eager, eager_c)
        torch.cuda.synchronize()
        assert torch.equal(cache, eager_c), pos
        for k in st:
            assert torch.equal(st[k], eager[k]), (k, pos)
        assert st["pos"].tolist() == [p + l for p, l in zip(pos, live)]


# ------------------------------------------------------------------ engine
def _requests(lengths, D, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, D, generator=g) * 0.3 for n in lengths]


def _predict(slots, max_new, stops, eos, seqs):
    """The CPU scheduler replayed on known outputs (seqs[i] = request i's ids): its counters for that run."""
    sched, nxt, cur = SlotScheduler(slots, max_new, stops, eos), 0, {}
    while True:
        for s in sched.free():
            while nxt < len(seqs) and sched.rows[s] is None:
                if sched.admit(s, seqs[nxt][0], 0.0):
                    cur[s] = [nxt, 1]
                nxt += 1
        if not sched.live():
            return sched
        ids = [0] * slots
        for s in sched.live():
            ids[s] = seqs[cur[s][0]][cur[s][1]]
            cur[s][1] += 1
        sched.step(ids, [0.0] * slots)


def test_full_slots_equal_the_batched_path_bit_for_bit(model):
    """Four-row prompts: the engine prefills a request alone (4 rows) and greedy_generate the batch (16 rows), and both are
    products of the <= 16-row weight-streaming kernel, whose rows do not depend on the row count -- above 16 rows the GEMM plan
    (tile, K split) follows the row count and the two prefills round differently."""
    lm = model.llama
    reqs = _requests([4] * 4, lm.D, 1)
    kw = dict(max_new_tokens=8, stop_ids=(), eos_id=-5, min_length=0)
    ids, mar = lm.greedy_generate(torch.stack(reqs).to(DEV), return_margins=True, **kw)
    dec = lm.slot_decoder(4, 64)
    got = sorted(dec.run(reqs, **kw), key=lambda r: r[0])
    assert [r[0] for r in got] == [0, 1, 2, 3]
    assert torch.equal(torch.stack([r[1] for r in got]), ids)
    assert torch.equal(torch.stack([r[2] for r in got]), mar)
    st = dec.last_stats
    assert st["steps"] == 7 and st["live_row_steps"] == 28 and st["occupancy"] == 1.0 and st["prefills"] == 4


def test_slots_are_isolated(model):
    lm = model.llama
    kw = dict(max_new_tokens=10, stop_ids=(), eos_id=-5, min_length=0)
    target = _requests([11], lm.D, 2)[0]
    dec = lm.slot_decoder(3, 64)
    (_, ids_a, mar_a), = list(dec.run([target], **kw))
    others = _requests([5, 17, 8, 23, 6, 14], lm.D, 3)
    got = {i: (ids, mar) for i, ids, mar in dec.run(others[:1] + [target] + others[1:], **kw)}
    assert len(got) == 7
    assert torch.equal(got[1][0], ids_a) and torch.equal(got[1][1], mar_a)
    assert dec.last_stats["graph_captures"] == 1                     # the second run replays the first one's graph


def test_one_decoder_serves_runs_at_different_temperatures(model):
    """The captured step's p_max is taken at the run's own temperature, whatever an earlier run of the same decoder used: after
    each run the last step's recorded p_max equals an eager arg-max launch on that step's logits at that temperature.  Then the
    draw branch itself: top_p = 1 draws every pick on the host, reproducibly per generator."""
    lm = model.llama
    reqs = _requests([6, 9], lm.D, 4)
    dec = lm.slot_decoder(2, 64)
    kw = dict(max_new_tokens=6, stop_ids=(), eos_id=-5, min_length=0)
    pm = {}
    for temp in (None, 2.0, 0.5, 2.0):                               # greedy first: its graph holds inv_temp = 1
        skw = {} if temp is None else dict(do_sample=True, temperature=temp, top_p=0.0)      # p_max < 0 never: no draw
        got = list(dec.run(reqs, **kw, **skw))
        assert [len(ids) for _, ids, _ in got] == [6, 6] and dec.last_stats["graph_replays"] >= 1
        assert dec.last_stats["host_sampled_rows"] == 0
        ws = dec.ws
        nxt, mar, pmx = torch.empty_like(ws["nxt"]), torch.empty_like(ws["mar"]), torch.empty_like(ws["pmx"])
        ops.argmax_pmax_rows(ws["logits"], nxt, mar, pmx, ban_id=-1, inv_temp=1.0 if temp is None else 1.0 / temp)
        assert torch.equal(ws["rec"][2], pmx), (temp, ws["rec"][2], pmx)
        assert torch.equal(ws["rec"][0].long(), nxt) and torch.equal(ws["rec"][1], mar)
        pm[temp] = pmx.cpu()
    assert bool((pm[0.5] > pm[None]).all()) and bool((pm[None] > pm[2.0]).all())     # a sharper / flatter softmax of the same logits
    assert dec.graph_captures == 3                                   # one per temperature, the second T = 2 run replays
    runs = []
    for _ in range(2):
        g = torch.Generator().manual_seed(9)
        out = sorted(dec.run(reqs, do_sample=True, temperature=2.0, top_p=1.0, generator=g, **kw), key=lambda r: r[0])
        assert dec.last_stats["host_sampled_rows"] == 12             # p_max < 1: every pick of both requests is a host draw
        runs.append([ids for _, ids, _ in out])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert dec.graph_captures == 3


def test_ragged_requests_and_per_request_stops_match_batch_1_decoding():
    """Fixture: the peaked token-transition LLaMA of tests/golden/decode_chain.npz (golden_utils.decode_chain_weights), prompts
    of 5 to 23 noise rows that end in a chain's start token.  The CPU oracle's greedy_generate on these seven requests has no
    step below the two-ulp gate: its smallest top-2 margin over all steps is 8.79 logits (request 3's first pick), at least 35
    times the gate 2 * 2^-7 * max|logit| of its own step (per-step logit scales 14.1 to 21.0; the smallest margin / gate ratio is
    35.8), so all seven requests are compared over their full length."""
    c = gu.DECODE_CHAIN
    sd = gu.decode_chain_weights()
    from myriad_amd.llama import LlamaHIP
    lm = LlamaHIP(sd, c["heads"], DEV, need_backward=False)
    starts = ["row0", "row1", "row2", "row3", "stop835", "row1", "row3"]
    lengths = [5, 23, 9, 14, 7, 18, 11]
    g = torch.Generator().manual_seed(77)
    emb_w = sd["llama_model.model.embed_tokens.weight"]
    reqs = []
    for name, n in zip(starts, lengths):
        x = torch.randn(n, c["D"], generator=g) * 0.3
        x[-1] = emb_w[gu.DECODE_CHAINS[name][0]]
        reqs.append(x)
    max_new = 12
    free = [lm.greedy_generate(x[None].to(DEV), max_new_tokens=max_new, stop_ids=(), eos_id=2, min_length=1,
                               return_margins=True)[0][0].tolist() for x in reqs]
    stops = ((free[3][1],), (free[0][4],))                           # request 3's second token, request 0's fifth
    want = [lm.greedy_generate(x[None].to(DEV), max_new_tokens=max_new, stop_ids=stops, eos_id=2, min_length=1,
                               return_margins=True) for x in reqs]
    want_ids = [w[0][0].tolist() for w in want]
    lens = [len(w) for w in want_ids]
    assert len({n for n in lens if n < max_new}) >= 3 and sum(n == max_new for n in lens) >= 2, lens
    dec = lm.slot_decoder(3, 64)
    got = {i: ids.tolist() for i, ids, _ in dec.run(reqs, max_new_tokens=max_new, stop_ids=stops, eos_id=2, min_length=1)}
    full = 0
    for i, x in enumerate(reqs):
        with torch.no_grad():
            _, o_mar, o_sc = R.greedy_generate(sd, x[None], c["heads"], max_new_tokens=max_new, stop_ids=stops, eos_id=2,
                                               min_length=1, return_margins=True, return_scales=True)
        first = F.two_ulp_horizon(o_mar, o_sc)
        print("request", i, "len", lens[i], "horizon", first, "min oracle margin", float(o_mar.min()), "ids", got[i])
        n = min(first, lens[i], len(got[i]))
        assert got[i][:n] == want_ids[i][:n], (i, got[i], want_ids[i])
        if first >= o_mar.shape[1]:                                  # no near tie anywhere: the whole request, its length too
            assert got[i] == want_ids[i], (i, got[i], want_ids[i])
            full += 1
    assert full >= 5, full
    st = dec.last_stats
    pred = _predict(3, max_new, stops, 2, want_ids)
    assert st["graph_captures"] == 1 and st["prefills"] == 7
    assert st["steps"] == pred.steps and st["live_row_steps"] == pred.live_row_steps and st["occupancy"] == pred.occupancy


def _ragged_batches(model, sizes, seed):
    """Loader batches with integer prompt ids whose lengths differ from row to row (the tokenised question, cut differently)."""
    tok, out, k = model.llama_tokenizer, [], 0
    for bi, n in enumerate(sizes):
        smp = _batch(n, train=False, seed=seed + bi)
        bs, as_ = [], []
        for q in smp["question2"]:
            pb, pa = ("###Human: " + q + " ###Assistant: ").split("<ImageHere>")
            b = tok(pb, return_tensors="pt", add_special_tokens=False).input_ids[0]
            a = tok(pa, return_tensors="pt", add_special_tokens=False).input_ids[0]
            bs.append(b[k % 3:])
            as_.append(a[:len(a) - (k % 4)])
            k += 1
        out.append(dict(image=smp["image"], anomaly_maps=smp["anomaly_maps"], before_ids=bs, after_ids=as_))
    return out


def test_generate_stream_matches_generate_per_sample(model, fx):
    model.eval()
    try:
        batches = _ragged_batches(model, (2, 3), seed=5)
        assert len({len(b) for bt in batches for b in bt["before_ids"]}) > 1
        kw = dict(max_new_tokens=8, stop_ids=((835,), (2277, 29937)), min_length=1)
        outs = list(model.generate_stream(iter(batches), slots=2, **kw))
        assert [o["index"] for o in outs] == [0, 1, 2, 3, 4]
        assert model.last_generate_stats["prefills"] == 5 and 0 < model.last_generate_stats["occupancy"] <= 1
        k = 0
        for bt in batches:
            for i in range(bt["image"].shape[0]):
                one = dict(image=bt["image"][i:i + 1], anomaly_maps=bt["anomaly_maps"][i:i + 1],
                           before_ids=bt["before_ids"][i][None], after_ids=bt["after_ids"][i][None])
                ref = model.generate(one, **kw)
                ids_ref = ref["token_ids"][0].cpu()
                assert torch.equal(outs[k]["ve_anomaly_map"], ref["ve_anomaly_maps"][0])
                with torch.no_grad():
                    img = one["image"].to(DEV, torch.float32)
                    parts = model.encode_img(img, one["anomaly_maps"].to(DEV, torch.float32), 1, False)
                    emb = model._assemble(parts, one["before_ids"], one["after_ids"], None, None)[0][:, 1:].contiguous()
                    _, o_mar, o_sc = R.greedy_generate(fx["sd"], emb.cpu(), 32, max_new_tokens=8, stop_ids=kw["stop_ids"], eos_id=2,
                                                       min_length=1, return_margins=True, return_scales=True)
                ids = outs[k]["token_ids"]
                n = min(F.two_ulp_horizon(o_mar, o_sc), ids.shape[0], ids_ref.shape[0])
                assert ids.dtype == torch.long and ids.dim() == 1 and torch.equal(ids[:n], ids_ref[:n]), (k, ids, ids_ref)
                k += 1
        for bad in (dict(repetition_penalty=1.2), dict(num_beams=2), dict(min_length=2)):
            with pytest.raises(NotImplementedError):
                model.generate_stream(iter(batches), slots=2, **dict(kw, **bad))
        with pytest.raises(TypeError):
            model.generate_stream(iter(batches), slots=2, bogus_flag=1, **kw)
    finally:
        model.train()


def test_eval_entry_point_streams_through_slots(fx, tmp_path):
    import eval_aqa
    rows = {}
    for slots in (0, 2):
        res = str(tmp_path / f"res{slots}.jsonl")
        path, records = eval_aqa.main(["--cfg-path", fx["eval_yaml"], "--dataset", "synthetic", "--bs", "2", "--limit", "2",
                                       "--slots", str(slots), "--out", res])
        rows[slots] = [json.loads(l) for l in open(path)]
        assert len(rows[slots]) == len(records) == 4
    assert [r["image_id"] for r in rows[2]] == [r["image_id"] for r in rows[0]]          # the dataset's order
    assert [r["image_path"] for r in rows[2]] == [r["image_path"] for r in rows[0]]
    assert all(set(a) == set(b) for a, b in zip(rows[2], rows[0]))
    assert set(rows[2][0]) == {"image_id", "image_path", "is_anomaly", "error", "output", "anomaly_score"}
