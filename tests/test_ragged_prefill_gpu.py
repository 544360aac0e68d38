"""Packed prefill of several decode slots: the ragged attention kernel (mh_attn_prefill_ragged) bit for bit against the three
launches it replaces and, independently, against fp64; its argument refusals; and the slot engine with prefill_batch > 1
(LlamaHIP._prefill_packed, SlotDecoder.run, MyriadHIP.generate_stream) against batch-1 decoding and a CPU replay of the refill
logic (myriad_amd.llama.replay_slot_run)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from myriad_amd.llama import LlamaHIP, replay_slot_run  # noqa: E402
from oracle import myriad_ref as R  # noqa: E402
from tests import fp8_ref as F  # noqa: E402
from tests import fp64_bounds as fb  # noqa: E402
from tests import golden_utils as gu  # noqa: E402
from tests import lora_merge_ref as LM  # noqa: E402
from tests.test_entrypoints_gpu import DEV, _batch, fx, model  # noqa: E402,F401

BF16, I32 = torch.bfloat16, torch.int32

from tests.ragged_case import GAP, H, N_SLOTS, T_CAP, TAIL, ragged_inputs  # noqa: E402


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module", params=[16, 128])
def ragged_case(request):
    """One launch of the kernel per head dim on the poisoned frame, shared by the bit-equality and the fp64 test."""
    D = request.param
    W, scale = H * D, D ** -0.5
    qkv, seg, M, pos = ragged_inputs(D, DEV)
    qkv0 = qkv.clone()
    cos, sin = fb.rope_tables(D, device=DEV)
    o = fb.poisoned((M, W), BF16, DEV)
    cache = fb.poisoned((N_SLOTS, T_CAP, 2 * W), BF16, DEV)
    seg_host = torch.tensor(seg, dtype=I32)
    pos_dev = pos.clamp_min(0).to(DEV)
    out = ops.attn_prefill_ragged(qkv, pos_dev, seg_host.to(DEV), seg_host, cache, cos, sin, H, D, scale, out=o)
    torch.cuda.synchronize()
    assert out is o
    return dict(D=D, W=W, scale=scale, qkv=qkv, qkv0=qkv0, seg=seg, M=M, pos=pos_dev, cos=cos, sin=sin, o=o, cache=cache)


def test_kernel_equals_rope_copy_attention_per_segment_bit_for_bit(ragged_case):
    c = ragged_case
    D, W, qkv, o, cache = c["D"], c["W"], c["qkv"], c["o"], c["cache"]
    assert torch.equal(_bits(qkv), _bits(c["qkv0"]))                 # qkv is only read
    owned = torch.zeros(c["M"], dtype=torch.bool)
    for r0, n, slot in c["seg"]:
        owned[r0:r0 + n] = True
        x = c["qkv0"][r0:r0 + n].clone()                             # the segment as a B = 1 batch through the three launches
        ops.rope_(x, 0, 2 * H, D, c["pos"][r0:r0 + n].contiguous(), c["cos"], c["sin"], 1.0)
        q3 = x.view(1, n, x.shape[1])
        kv = torch.zeros((1, n, 2 * W), dtype=BF16, device=DEV)
        ops.copy3d_bf16(q3[:, :, W:3 * W], kv)
        o_ref, _ = ops.attn_fwd(q3[:, :, :W], q3[:, :, W:2 * W], q3[:, :, 2 * W:3 * W], H, D, c["scale"], causal=True, need_lse=False)
        assert torch.equal(_bits(o[r0:r0 + n]), _bits(o_ref[0])), (D, n, "o")
        assert torch.equal(_bits(cache[slot, :n]), _bits(kv[0])), (D, n, "cache")
        fb.assert_untouched(cache[slot, n:], f"D={D} cache rows >= len of slot {slot}")
    fb.assert_untouched(o[~owned.to(DEV)], f"D={D} gap and padding rows of o")
    assert int((~owned).sum()) == GAP + TAIL
    fb.assert_untouched(cache[2], f"D={D} the unnamed slot")


def _heads(t, n, D):
    return t.reshape(1, n, H, D).transpose(1, 2)


def _tok(t):
    return t.transpose(1, 2).reshape(t.shape[2], -1)


def test_kernel_is_within_the_fp64_bound_per_segment(ragged_case):
    """Independent of the tiled kernel: fp64 attention of the bf16-rounded fp64 rotation (fp64_bounds.rope_bf16 / attn_ref_bound),
    the rotation's rounding ambiguities passed as q_err / k_err; the exempt share is a condition (<= 1 %, no whole row)."""
    c = ragged_case
    D, W = c["D"], c["W"]
    for r0, n, slot in c["seg"]:
        x = c["qkv0"][r0:r0 + n].float()
        q, k, v = (_heads(x[:, i * W:(i + 1) * W], n, D) for i in range(3))
        pl = c["pos"][r0:r0 + n].long()[None]
        qr, qe = fb.rope_bf16(q, pl, c["cos"], c["sin"])
        kr, ke = fb.rope_bf16(k, pl, c["cos"], c["sin"])
        if n > 1:                                                    # a one-row segment is too few elements for a share
            fb.assert_rope_exempt_share(qe, f"D={D} len={n} q"), fb.assert_rope_exempt_share(ke, f"D={D} len={n} k")
        r = fb.attn_ref_bound(qr, kr, v, c["scale"], fb.attn_mask(1, n, n, True, None, DEV), q_err=qe, k_err=ke)
        worst = fb.assert_within(c["o"][r0:r0 + n], _tok(r["o"]), _tok(r["o_bound"]), f"D={D} len={n} o")
        # the cache holds the rotated keys (one bf16 ulp where the rotation is ambiguous) and the values as they are
        fb.assert_within(c["cache"][slot, :n, :W], _tok(kr), _tok(ke), f"D={D} len={n} cached k")
        assert torch.equal(c["cache"][slot, :n, W:], c["qkv0"][r0:r0 + n, 2 * W:3 * W])
        print(f"D={D} len={n}: o max err / bound {worst:.3f}")


def _refusal_case(D):
    W = H * D
    qkv = (fb.rnd(64, 3 * W + 64, seed=D) * 0.5).to(BF16).to(DEV)
    cos, sin = fb.rope_tables(D, device=DEV)
    return qkv, torch.arange(64, dtype=I32, device=DEV) % 16, cos, sin, W


@pytest.mark.parametrize("D,seg,code", [
    (16, [(0, 10, 1), (10, 10, 1)], "MH_ERR_ARG"),                   # a duplicate slot
    (16, [(0, 10, 0), (10, 10, 3)], "MH_ERR_ARG"),                   # slot = n_slots
    (16, [(0, 65, 0)], "MH_ERR_ARG"),                                # len = T_cap + 1
    (16, [(0, 10, 0), (9, 10, 1)], "MH_ERR_ARG"),                    # overlapping segments
    (16, [(60, 10, 0)], "MH_ERR_ARG"),                               # past the last row
    (16, [(0, 0, 0)], "MH_ERR_ARG"),                                 # an empty segment
    (88, [(0, 10, 0)], "MH_ERR_UNSUPPORTED"),
    (24, [(0, 10, 0)], "MH_ERR_UNSUPPORTED"),
])
def test_bad_arguments_are_refused_before_any_launch(D, seg, code):
    qkv, pos, cos, sin, W = _refusal_case(D)
    o = fb.poisoned((64, W), BF16, DEV)
    cache = fb.poisoned((3, 64, 2 * W), BF16, DEV)
    seg_host = torch.tensor(seg, dtype=I32)
    with pytest.raises(_lib.MyriadHipError, match=code):
        ops.attn_prefill_ragged(qkv, pos, seg_host.to(DEV), seg_host, cache, cos, sin, H, D, D ** -0.5, out=o)
    torch.cuda.synchronize()
    fb.assert_untouched(o, "o"), fb.assert_untouched(cache, "cache")


# ------------------------------------------------------------------ engine, peaked fixture
MAX_NEW = 12


@pytest.fixture(scope="module")
def peaked():
    """The peaked token-transition LLaMA of tests/golden/decode_chain.npz and the seven ragged requests and two stop sequences of
    tests/test_decode_slots_gpu.py::test_ragged_requests_and_per_request_stops_match_batch_1_decoding (built the same way), their
    batch-1 greedy ids and the oracle's two-ulp horizon per request, computed once."""
    c = gu.DECODE_CHAIN
    sd = gu.decode_chain_weights()
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
    free = [lm.greedy_generate(x[None].to(DEV), max_new_tokens=MAX_NEW, stop_ids=(), eos_id=2, min_length=1)[0].tolist() for x in reqs]
    stops = ((free[3][1],), (free[0][4],))                           # request 3's second token, request 0's fifth
    want = [lm.greedy_generate(x[None].to(DEV), max_new_tokens=MAX_NEW, stop_ids=stops, eos_id=2, min_length=1)[0].tolist()
            for x in reqs]
    horizon, whole = [], []
    for x in reqs:
        with torch.no_grad():
            _, o_mar, o_sc = R.greedy_generate(sd, x[None], c["heads"], max_new_tokens=MAX_NEW, stop_ids=stops, eos_id=2,
                                               min_length=1, return_margins=True, return_scales=True)
        horizon.append(F.two_ulp_horizon(o_mar, o_sc))
        whole.append(horizon[-1] >= o_mar.shape[1])
    return dict(lm=lm, sd=sd, reqs=reqs, lengths=lengths, stops=stops, want=want, horizon=horizon, whole=whole)


def _check_ids(p, got):
    full = 0
    for i, want in enumerate(p["want"]):
        n = min(p["horizon"][i], len(want), len(got[i]))
        assert got[i][:n] == want[:n], (i, got[i], want)
        if p["whole"][i]:                                            # no near tie anywhere: the whole request, its length too
            assert got[i] == want, (i, got[i], want)
            full += 1
    assert full >= 5, full


def _check_counters(p, st, slots, **plan):
    pred = replay_slot_run(p["lengths"], p["want"], slots, MAX_NEW, p["stops"], 2, **plan)
    assert st["prefills"] == pred["prefills"] == 7
    for k in ("prefill_passes", "packed_rows", "steps", "live_row_steps", "occupancy"):
        assert st[k] == pred[k], (k, st[k], pred[k])
    return pred


def test_packed_prefill_matches_batch_1_decoding_on_ragged_requests(peaked):
    p = peaked
    dec = p["lm"].slot_decoder(3, 64)
    got = {i: ids.tolist() for i, ids, _ in dec.run(p["reqs"], max_new_tokens=MAX_NEW, stop_ids=p["stops"], eos_id=2, min_length=1,
                                                    prefill_batch=3)}
    _check_ids(p, got)
    pred = _check_counters(p, dec.last_stats, 3, prefill_batch=3)
    assert dec.last_stats["graph_captures"] == 1
    assert pred["prefill_passes"] < 7                                # some pass held more than one request
    print("prefill_batch=3:", dec.last_stats)


def test_refill_min_packs_fuller_passes_with_the_same_ids(peaked):
    p = peaked
    kw = dict(max_new_tokens=MAX_NEW, stop_ids=p["stops"], eos_id=2, min_length=1, prefill_batch=3)
    dec = p["lm"].slot_decoder(3, 64)
    got = {i: ids.tolist() for i, ids, _ in dec.run(p["reqs"], refill_min=2, **kw)}
    _check_ids(p, got)
    st2 = dict(dec.last_stats)
    _check_counters(p, st2, 3, prefill_batch=3, refill_min=2)
    st1 = replay_slot_run(p["lengths"], p["want"], 3, MAX_NEW, p["stops"], 2, prefill_batch=3)
    print("refill_min=2:", st2, "refill_min=1:", st1)
    assert st2["packed_rows"] / st2["prefill_passes"] > st1["packed_rows"] / st1["prefill_passes"]


def test_a_segment_sees_nothing_of_its_neighbours_through_the_whole_model(peaked):
    """An 11-row request in the middle of a first pass of lengths [5, 11, 17], twice with different neighbours of the same lengths:
    equal packed shapes give equal GEMM plans and rows are independent everywhere but in the attention, so its ids and margins can
    differ only through a leak across a segment boundary."""
    lm = peaked["lm"]
    g = torch.Generator().manual_seed(5)
    target = torch.randn(11, lm.D, generator=g) * 0.3
    dec = lm.slot_decoder(3, 64)
    runs = []
    for seed in (6, 7):
        gs = torch.Generator().manual_seed(seed)
        a, b = torch.randn(5, lm.D, generator=gs) * 0.3, torch.randn(17, lm.D, generator=gs) * 0.3
        got = {i: (ids, mar) for i, ids, mar in dec.run([a, target, b], max_new_tokens=10, stop_ids=(), eos_id=-5, min_length=0,
                                                        prefill_batch=3)}
        assert dec.last_stats["prefill_passes"] == 1 and dec.last_stats["packed_rows"] == 33
        runs.append(got)
    assert torch.equal(runs[0][1][0], runs[1][1][0]) and torch.equal(runs[0][1][1], runs[1][1][1])
    assert not torch.equal(runs[0][0][1], runs[1][0][1])             # the neighbours did differ


# ------------------------------------------------------------------ LoRA attached
TINY = dict(D=128, layers=2, heads=4, inter=172, V=320, seed=401)


def _lora_model(seed=77, r=8):
    """The tiny LoRA model of tests/test_fp4_decode_gpu.py (llama_tiny's flat-logit recipe at D = 128, r = 8 on q / v), restated."""
    from myriad_amd.lora import PEFT_PREFIX, LoraQV, lora_param_specs
    from myriad_amd.myriad import ParamStore
    t = TINY
    sd = {k: (v.to(BF16).float() if v.is_floating_point() and v.dim() == 2 else v)
          for k, v in gu.llama_weights(t["D"], t["layers"], t["inter"], t["V"], seed=t["seed"], std=0.2).items()}
    emb = torch.randn(3, 12, t["D"], generator=torch.Generator().manual_seed(t["seed"] + 1)) * 0.5
    st = ParamStore(lora_param_specs(t["layers"], t["D"], r), DEV)
    gen = torch.Generator().manual_seed(seed)
    osd = dict(sd)
    for name, ishape, _ in st.specs:
        w = (torch.randn(ishape, generator=gen) * (0.05 if "lora_A" in name else 0.1)).to(BF16).float()
        st.p[name].copy_(w)
        osd[name.replace(PEFT_PREFIX, "llama_model.model.layers.")] = w
    lm = LlamaHIP(sd, t["heads"], DEV, need_backward=False)
    lm.attach_lora(LoraQV(t["layers"], t["D"], r, 16.0, 0.0, st.p, st.g, DEV))
    return emb, osd, t["heads"], lm


@pytest.mark.parametrize("merge", [False, True])
def test_packed_prefill_with_lora_attached(merge):
    """Which check: the ids of three ragged requests (5, 7 and 9 rows) equal the reference loop's (tests/fp8_ref.greedy_decode: the
    prefill with the exact LoRA, every later step on the bordered weights or, with decode_merge_lora, on the merged copy) at every
    step before that loop's first two-ulp near tie -- the rule of the FP8 / FP4 decode tests, through their helpers unchanged.  The
    packed prefill keeps the bordered LoRA either way.  Floors are asserted so that the test cannot pass on a handful of steps."""
    emb, osd, heads, lm = _lora_model()
    lm.decode_merge_lora = merge
    lora = dict(r=8, alpha=16.0, dropout_mask=None)
    step_sd = LM.merged_step_state_dict(osd, TINY["layers"], 2.0) if merge else osd
    reqs = [emb[i, :n].contiguous() for i, n in enumerate((5, 7, 9))]
    dec = lm.slot_decoder(3, 64)
    got = {i: ids for i, ids, _ in dec.run(reqs, max_new_tokens=16, stop_ids=(), eos_id=2, min_length=1, prefill_batch=3)}
    assert dec.last_stats["prefill_passes"] == 1 and dec.last_stats["prefills"] == 3
    checked = 0
    for i, e in enumerate(reqs):
        with torch.no_grad():
            ids_ref, _, margins, scales = F.greedy_decode(osd, step_sd, e[None], heads, 16, lora=lora)
        first = min(F.two_ulp_horizon(margins, scales), ids_ref.shape[1])
        assert len(got[i]) >= first and torch.equal(got[i][:first], ids_ref[0, :first]), (i, first, got[i], ids_ref)
        checked += first
    print("LoRA merge =", merge, ": steps compared", checked)
    assert checked >= 17, checked                                    # the reference alone admits 17 (bordered) and 27 (merged)
    assert (lm._packed["qkv_key"] == "merged") is merge


# ------------------------------------------------------------------ public entry point
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


def test_generate_stream_with_packed_prefill_matches_generate_per_sample(model, fx):
    model.eval()
    try:
        batches = _ragged_batches(model, (2, 3), seed=5)
        assert len({len(b) for bt in batches for b in bt["before_ids"]}) > 1
        kw = dict(max_new_tokens=8, stop_ids=((835,), (2277, 29937)), min_length=1)
        outs = list(model.generate_stream(iter(batches), slots=3, prefill_batch=3, **kw))
        assert [o["index"] for o in outs] == [0, 1, 2, 3, 4]         # input order
        st = model.last_generate_stats
        assert st["prefills"] == 5 and st["prefill_passes"] < 5 and 0 < st["occupancy"] <= 1
        k = 0
        for bt in batches:
            for i in range(bt["image"].shape[0]):
                one = dict(image=bt["image"][i:i + 1], anomaly_maps=bt["anomaly_maps"][i:i + 1],
                           before_ids=bt["before_ids"][i][None], after_ids=bt["after_ids"][i][None])
                ref = model.generate(one, **kw)
                ids_ref = ref["token_ids"][0].cpu()
                assert torch.equal(outs[k]["ve_anomaly_map"], ref["ve_anomaly_maps"][0])     # paired with its own sample
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
    finally:
        model.train()
