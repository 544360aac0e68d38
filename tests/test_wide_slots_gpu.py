"""The slot engine above 16 slots (LlamaHIP.slot_decoder, MyriadHIP.generate_stream, eval_aqa --slots), where its token step runs
ops.gemv_packed_wide on the packed copies.  A row of the wide product carries the bits of the 16-row kernel and the rows attention,
the per-row sampler and the bookkeeping launches are row-independent, so a request's ids AND margins at 24 or 32 slots must be
torch.equal to the same request through ONE slot: no tolerance an indexing mistake could hide behind.  Models: the peaked
token-transition LLaMA of tests/golden/decode_chain.npz (tests/test_decode_slots_gpu.py's) and llama_tiny's flat-logit recipe at
D = 128 (tests/test_fp4_decode_gpu.py's: every K a multiple of 128), both built here the same way."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import ops  # noqa: E402
from myriad_amd.llama import LlamaHIP  # noqa: E402
from tests import golden_utils as gu  # noqa: E402
from tests.test_decode_slots_gpu import _ragged_batches  # noqa: E402
from tests.test_entrypoints_gpu import DEV, fx, model  # noqa: E402,F401

BF16 = torch.bfloat16
MAX_NEW = 10
N_REQ = 40
TINY = dict(D=128, layers=2, heads=4, inter=172, V=320, seed=401)


def _lengths(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(3, 24, (n,), generator=g).tolist()          # 3 .. 23 rows


def _run(dec, reqs, **kw):
    return {i: (ids, mar) for i, ids, mar in dec.run(reqs, **kw)}


def _assert_same(got, want, n, what):
    assert sorted(got) == sorted(want) == list(range(n)), what
    for i in range(n):
        assert torch.equal(got[i][0], want[i][0]), (what, i, got[i][0].tolist(), want[i][0].tolist())
        assert torch.equal(got[i][1], want[i][1]), (what, i, "margins")


# ------------------------------------------------------------------ the peaked model: bf16, stops, packed prefill, graph replay
@pytest.fixture(scope="module")
def peaked():
    """40 ragged requests (3 to 23 noise rows ending in a chain's start token), two per-request stop sequences taken from a free run,
    and every request's ids and margins through ONE slot, computed once."""
    c = gu.DECODE_CHAIN
    sd = gu.decode_chain_weights()
    lm = LlamaHIP(sd, c["heads"], DEV, need_backward=False)
    emb_w = sd["llama_model.model.embed_tokens.weight"]
    names = ["row0", "row1", "row2", "row3", "stop835"]
    g = torch.Generator().manual_seed(78)
    reqs = []
    for i, n in enumerate(_lengths(N_REQ, 5)):
        x = torch.randn(n, c["D"], generator=g) * 0.3
        x[-1] = emb_w[gu.DECODE_CHAINS[names[i % len(names)]][0]]
        reqs.append(x)
    one = lm.slot_decoder(1, 64)
    free = _run(one, reqs, max_new_tokens=MAX_NEW, stop_ids=(), eos_id=2, min_length=1)
    stops = ((int(free[3][0][1]),), (int(free[0][0][4]),))           # request 3's second token, request 0's fifth
    kw = dict(max_new_tokens=MAX_NEW, stop_ids=stops, eos_id=2, min_length=1)
    want = _run(one, reqs, **kw)
    lens = [len(want[i][0]) for i in range(N_REQ)]
    assert len(set(lens)) >= 3 and max(lens) == MAX_NEW, lens         # requests do end at different steps
    return dict(lm=lm, reqs=reqs, kw=kw, want=want)


def test_ragged_requests_at_32_slots_equal_one_slot_bit_for_bit(peaked):
    p = peaked
    dec = p["lm"].slot_decoder(32, 64)
    got = _run(dec, p["reqs"], **p["kw"])
    _assert_same(got, p["want"], N_REQ, "32 slots")
    st = dict(dec.last_stats)
    print("32 slots:", st)
    assert st["prefills"] == N_REQ and 0 < st["occupancy"] <= 1 and st["graph_captures"] == 1
    assert st["live_row_steps"] <= st["steps"] * 32
    # a second run on the same decoder replays the captured graph
    again = _run(dec, p["reqs"][::-1], **p["kw"])
    _assert_same({N_REQ - 1 - i: v for i, v in again.items()}, p["want"], N_REQ, "32 slots, reversed")
    assert dec.graph_captures == 1 and dec.last_stats["graph_replays"] == dec.last_stats["steps"] > 0


@pytest.mark.parametrize("slots", [17, 64])
def test_the_ends_of_the_wide_range(peaked, slots):
    p = peaked
    got = _run(p["lm"].slot_decoder(slots, 64), p["reqs"], **p["kw"])
    _assert_same(got, p["want"], N_REQ, f"{slots} slots")


def test_packed_prefill_at_32_slots_gives_the_one_request_refills_ids(peaked):
    p = peaked
    dec = p["lm"].slot_decoder(32, 64)
    got = _run(dec, p["reqs"], prefill_batch=8, refill_min=2, **p["kw"])
    st = dict(dec.last_stats)
    print("32 slots, prefill_batch=8 refill_min=2:", st)
    assert st["prefills"] == N_REQ and st["prefill_passes"] < N_REQ
    assert sorted(got) == list(range(N_REQ))
    for i in range(N_REQ):
        assert got[i][0].tolist() == p["want"][i][0].tolist(), i


def test_slot_limit_is_the_wide_row_limit(peaked):
    lm = peaked["lm"]
    assert ops.GEMV_WIDE_MAX_ROWS == 64
    with pytest.raises(ValueError, match="64"):
        lm.slot_decoder(65, 64)
    with pytest.raises(ValueError):
        lm.slot_decoder(0, 64)
    lm.slot_decoder(64, 64)


def test_other_decode_loops_keep_the_gemm_above_16_rows(peaked):
    """greedy_generate at 20 rows before and after a 32-slot run of the same model: the same ids and margins, and the stats still
    report the row-major bf16 matrices (the wide product is the slot engine's alone)."""
    lm = peaked["lm"]
    x = torch.stack([r[-3:] for r in peaked["reqs"][:20]]).to(DEV)
    kw = dict(max_new_tokens=6, stop_ids=(), eos_id=-5, min_length=0, return_margins=True)
    fresh = LlamaHIP(gu.decode_chain_weights(), gu.DECODE_CHAIN["heads"], DEV, need_backward=False)
    ids0, mar0 = fresh.greedy_generate(x, **kw)
    ids1, mar1 = lm.greedy_generate(x, **kw)                          # lm has packed copies live from the slot runs
    assert torch.equal(ids0, ids1) and torch.equal(mar0, mar1)
    rowmajor = sum(m.numel() * m.element_size() for L in lm.layers for m in (L["wqkv"], L["wo"], L["wgu"], L["wd"]))
    assert lm.last_generate_stats["decode_weight_bytes"] == rowmajor + lm.lm_head.numel() * lm.lm_head.element_size()


# ------------------------------------------------------------------ the flat-logit model: fp8, fp4, LoRA, sampling
def _tiny_sd():
    t = TINY
    return {k: (v.to(BF16).float() if v.is_floating_point() and v.dim() == 2 else v)
            for k, v in gu.llama_weights(t["D"], t["layers"], t["inter"], t["V"], seed=t["seed"], std=0.2).items()}


def _tiny_model(lora=False, seed=77, r=8):
    t = TINY
    lm = LlamaHIP(_tiny_sd(), t["heads"], DEV, need_backward=False)
    if lora:
        from myriad_amd.lora import LoraQV, lora_param_specs
        from myriad_amd.myriad import ParamStore
        st = ParamStore(lora_param_specs(t["layers"], t["D"], r), DEV)
        gen = torch.Generator().manual_seed(seed)
        for name, ishape, _ in st.specs:
            st.p[name].copy_((torch.randn(ishape, generator=gen) * (0.05 if "lora_A" in name else 0.1)).to(BF16).float())
        lm.attach_lora(LoraQV(t["layers"], t["D"], r, 16.0, 0.0, st.p, st.g, DEV))
    return lm


def _tiny_requests(seed=31):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, TINY["D"], generator=g) * 0.5 for n in _lengths(N_REQ, seed)]


@pytest.mark.parametrize("mode", ["fp8", "fp4", "lora_bordered", "lora_merged", "lora_merged_fp8"])
def test_other_weight_kinds_at_24_slots_equal_their_own_one_slot_run(mode):
    lm = _tiny_model(lora=mode.startswith("lora"))
    lm.decode_fp8 = mode.endswith("fp8")
    lm.decode_fp4 = mode == "fp4"
    lm.decode_merge_lora = "merged" in mode
    reqs = _tiny_requests()
    one = lm.slot_decoder(1, 64)
    free = _run(one, reqs[:4], max_new_tokens=MAX_NEW, stop_ids=(), eos_id=-5, min_length=0)
    kw = dict(max_new_tokens=MAX_NEW, stop_ids=((int(free[3][0][1]),), (int(free[0][0][4]),)), eos_id=int(free[1][0][6]), min_length=1)
    want = _run(one, reqs, **kw)
    dec = lm.slot_decoder(24, 64)
    got = _run(dec, reqs, **kw)
    _assert_same(got, want, N_REQ, mode)
    assert len({len(want[i][0]) for i in range(N_REQ)}) >= 3          # the stops did cut requests at different steps
    P = lm._packed
    assert P["kind"] == ("fp8" if lm.decode_fp8 else "fp4" if lm.decode_fp4 else "bf16")
    assert P["qkv_key"] == ("merged" if lm.decode_merge_lora else "wqkv_ext" if lm.lora is not None else "wqkv")
    assert dec.last_stats["prefills"] == N_REQ and dec.last_stats["graph_captures"] == 1


def test_device_sampling_at_32_slots_draws_each_requests_own_stream():
    lm = _tiny_model()
    lm.device_sampling = True
    reqs = _tiny_requests(32)
    seeds = [900 + 1000 * i for i in range(N_REQ)]
    kw = dict(max_new_tokens=MAX_NEW, stop_ids=(), do_sample=True, top_p=0.9)
    want = _run(lm.slot_decoder(1, 64), reqs, seeds=seeds, **kw)
    dec = lm.slot_decoder(32, 64)
    got = _run(dec, reqs, seeds=seeds, **kw)
    st = dict(dec.last_stats)
    for i in range(N_REQ):
        assert got[i][0].tolist() == want[i][0].tolist(), i
    assert st["host_sampled_rows"] == 0 and st["device_sampled_rows"] == sum(len(want[i][0]) for i in range(N_REQ)) > 0
    greedy = _run(dec, reqs, max_new_tokens=MAX_NEW, stop_ids=())
    assert any(greedy[i][0].tolist() != got[i][0].tolist() for i in range(N_REQ))    # draws, not the arg-max


# ------------------------------------------------------------------ public surface
def test_generate_stream_at_32_slots_yields_every_sample_in_order_with_the_ids_of_one_slot(model):
    model.eval()
    try:
        batches = _ragged_batches(model, (2, 3), seed=5)
        kw = dict(max_new_tokens=8, stop_ids=((835,), (2277, 29937)), min_length=1)
        outs = {s: list(model.generate_stream(iter(batches), slots=s, **kw)) for s in (1, 32)}
        assert [o["index"] for o in outs[32]] == [0, 1, 2, 3, 4]
        assert model.last_generate_stats["prefills"] == 5 and 0 < model.last_generate_stats["occupancy"] <= 1
        for a, b in zip(outs[32], outs[1]):
            assert torch.equal(a["token_ids"], b["token_ids"]), (a["index"], a["token_ids"], b["token_ids"])
            assert torch.equal(a["ve_anomaly_map"], b["ve_anomaly_map"])
    finally:
        model.train()


def test_eval_entry_point_streams_through_32_slots(fx, tmp_path):
    import eval_aqa
    path, records = eval_aqa.main(["--cfg-path", fx["eval_yaml"], "--dataset", "synthetic", "--bs", "2", "--limit", "2", "--slots", "32",
                                   "--out", str(tmp_path / "res32.jsonl")])
    rows = [json.loads(ln) for ln in open(path)]
    assert len(rows) == len(records) == 4
    assert set(rows[0]) == {"image_id", "image_path", "is_anomaly", "error", "output", "anomaly_score"}
