"""Draft-and-verify decoding in the decode slots (SlotDecoder.run(draft=, draft_k=), generate_stream, eval_aqa.py --slots N --draft-k
K).  The contract is exact: whatever the drafter proposes, whatever the slot count, K, the refill settings and the neighbours, a
request's ids and margins are bit for bit those of the same run without `draft` and of greedy_generate on that request alone -- no
margin gate, no tolerance -- and the step counts are the ones decode_host.replay_slot_run(draft=, draft_k=) works out without a
device."""
import json
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import ops  # noqa: E402
from myriad_amd.decode_host import NgramDrafter, replay_slot_run  # noqa: E402
from myriad_amd.llama import LlamaHIP  # noqa: E402
from tests import golden_utils as gu  # noqa: E402
from tests.test_draft_decode_gpu import Noise, Wrong, flat  # noqa: E402,F401
from tests.test_entrypoints_gpu import _batch, fx, model  # noqa: E402,F401

DEV = "cuda:0"
ROWS = ["row0", "row1", "row2", "row3", "stop835"]
EXTRA = [0, 3, 1, 5, 2, 4, 0, 2, 7, 1]                                       # rows of noise in front of each request's six
KW = dict(max_new_tokens=90, min_length=1)
CAP = 128                                                                      # 13 prompt rows + 90 tokens
COUNTS = ("steps", "verify_steps", "plain_steps", "draft_proposed", "draft_accepted", "occupancy", "live_row_steps", "prefills",
          "prefill_passes", "packed_rows", "emitted")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """{index: (ids, margins)} equal bit for bit."""
    return a.keys() == b.keys() and all(torch.equal(a[i][0], b[i][0]) and torch.equal(_bits(a[i][1]), _bits(b[i][1])) for i in a)


def _run(dec, reqs, **kw):
    out = {i: (ids, mar) for i, ids, mar in dec.run(reqs, **kw)}
    return out, dict(dec.last_stats)


def _solo(lm, reqs, **kw):
    """greedy_generate on every request alone: {index: (ids [L], margins [L])} on the CPU."""
    out = {}
    for i, e in enumerate(reqs):
        ids, mar = lm.greedy_generate(e[None].to(DEV), return_margins=True, **kw)
        out[i] = (ids[0].cpu(), mar[0].cpu())
    return out


@pytest.fixture(scope="module")
def chain():
    """The peaked-chain model, ten ragged requests (the five rows twice, prompts of 6 to 13 rows), every request's answer alone
    and through the slots without `draft`: computed once.  One engine per slot count, kept for the module."""
    lm = LlamaHIP(gu.decode_chain_weights(), gu.DECODE_CHAIN["heads"], DEV, need_backward=False)
    assert lm.slot_draft is False                                              # off by default
    lm.slot_draft = True
    g = torch.Generator().manual_seed(31)
    names = ROWS + ROWS
    reqs = [torch.cat([torch.randn(n, gu.DECODE_CHAIN["D"], generator=g) * 0.3, gu.decode_chain_inputs([r])[0]]) for r, n in zip(names, EXTRA)]
    solo = _solo(lm, reqs, **KW)
    decs = {s: lm.slot_decoder(s, CAP) for s in (1, 2, 4, 8)}
    plain, plain_st = _run(decs[4], reqs, **KW)
    assert _same(plain, solo) and "draft_k" not in plain_st and "verify_steps" not in plain_st
    ids = [solo[i][0].tolist() for i in range(len(reqs))]
    return types.SimpleNamespace(lm=lm, reqs=reqs, names=names, solo=solo, ids=ids, lens=[int(e.shape[0]) for e in reqs], decs=decs)


def _drafter(kind, chain):
    return {"taught": lambda: NgramDrafter(chain.ids), "wrong": Wrong, "noise": lambda: Noise(gu.DECODE_CHAIN["vocab"], seed=9)}[kind]()


@pytest.mark.parametrize("kind", ["taught", "wrong", "noise"])
@pytest.mark.parametrize("slots,K", [(2, 4), (4, 4), (8, 4), (8, 8)])
def test_every_request_has_the_bits_of_the_run_without_draft_and_of_greedy_generate_alone(chain, slots, K, kind):
    dec = chain.decs[slots]
    plain, plain_st = _run(dec, chain.reqs, **KW)
    d = _drafter(kind, chain)
    out, st = _run(dec, chain.reqs, draft=d, draft_k=K, **KW)
    assert _same(out, plain) and _same(out, chain.solo), (slots, K, kind)
    assert st["draft_k"] == K and st["draft_off"] is None and st["verify_steps"] > 0 and st["steps"] == st["verify_steps"] + st["plain_steps"]
    assert st["emitted"] == sum(len(i) - 1 for i in chain.ids) and st["graph_replays"] == st["verify_graph_replays"] + st["plain_graph_replays"]
    if kind == "taught":                                                       # the counts the host works out without a device
        want = replay_slot_run(chain.lens, chain.ids, slots, 90, draft=NgramDrafter(chain.ids), draft_k=K, stop_ids=((835,), (2277, 29937)))
        assert {k: st[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, (st, want)
        assert st["draft_accepted"] > 0 and st["steps"] < plain_st["steps"]
    if kind == "wrong":
        assert st["draft_accepted"] == 0 and st["draft_proposed"] > 0
        assert st["steps"] == plain_st["steps"]                                # a wrong guess costs rows, never a step
    assert "draft_k" not in plain_st and {k: plain_st[k] for k in ("steps", "prefills")} == {
        k: replay_slot_run(chain.lens, chain.ids, slots, 90, stop_ids=((835,), (2277, 29937)))[k] for k in ("steps", "prefills")}


def test_an_untaught_drafter_runs_only_plain_steps_on_the_plain_graph(chain):
    dec = chain.decs[4]
    out, st = _run(dec, chain.reqs, draft=NgramDrafter(), draft_k=4, **KW)
    plain, plain_st = _run(dec, chain.reqs, **KW)
    assert _same(out, plain)
    assert st["verify_steps"] == 0 and st["draft_proposed"] == 0 and st["plain_steps"] == st["steps"] == plain_st["steps"]
    assert st["verify_graph_replays"] == 0 and st["plain_graph_replays"] == st["graph_replays"] == plain_st["graph_replays"] > 0
    out1, st1 = _run(dec, chain.reqs, draft=NgramDrafter(chain.ids), draft_k=1, **KW)      # K = 1: the plain step only
    assert _same(out1, plain) and st1["verify_steps"] == 0 and st1["plain_steps"] == plain_st["steps"] and st1["draft_k"] == 1


def test_both_graphs_replay_in_one_run_when_half_of_the_requests_are_unknown(chain):
    known = [i for i, r in enumerate(chain.names) if r in ("row2", "row3", "stop835")]
    order = known[:5] + [i for i in range(10) if i not in known[:5]]           # the short known answers first, the long unknown ones last
    reqs, ids, lens = [chain.reqs[i] for i in order], [chain.ids[i] for i in order], [chain.lens[i] for i in order]
    d = NgramDrafter([chain.ids[i] for i in known])
    out, st = _run(chain.decs[2], reqs, draft=d, draft_k=4, **KW)
    assert _same(out, {n: chain.solo[i] for n, i in enumerate(order)})
    want = replay_slot_run(lens, ids, 2, 90, draft=d, draft_k=4, stop_ids=((835,), (2277, 29937)))
    assert {k: st[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, (st, want)
    assert st["verify_steps"] >= 3 and st["plain_steps"] >= 3 and st["verify_graph_replays"] > 0 and st["plain_graph_replays"] > 0


def test_flat_logits_are_bit_equal_with_no_margin_gate(flat, monkeypatch):
    monkeypatch.setattr(flat.lm, "slot_draft", True)
    kw = dict(max_new_tokens=40, stop_ids=())
    reqs = [flat.emb[r, :s0].contiguous() for r, s0 in ((0, 5), (1, 9), (0, 7), (1, 6), (0, 8), (1, 4))]
    solo = _solo(flat.lm, reqs, **kw)
    dec = flat.lm.slot_decoder(4, 64)
    plain, _ = _run(dec, reqs, **kw)
    out, st = _run(dec, reqs, draft=Noise(flat.V), draft_k=4, **kw)
    assert _same(out, plain) and _same(out, solo)
    assert st["draft_off"] is None and st["verify_steps"] > 0 and st["draft_proposed"] > 0


@pytest.mark.parametrize("lora", ["bordered", "merged"])
@pytest.mark.parametrize("kind", ["bf16", "fp8", "fp4"])
def test_every_kind_of_decode_weights_is_bit_equal_to_its_own_run_without_draft(kind, lora):
    from tests.test_fp4_decode_gpu import _lora_model
    emb, _, _, lm = _lora_model()
    lm.decode_fp8, lm.decode_fp4, lm.decode_merge_lora, lm.slot_draft = kind == "fp8", kind == "fp4", lora == "merged", True
    kw = dict(max_new_tokens=24, stop_ids=())
    reqs = [emb[r, :s0].contiguous() for r, s0 in ((0, 7), (1, 5), (2, 9), (0, 4), (1, 12), (2, 6))]
    dec = lm.slot_decoder(4, 64)
    plain, _ = _run(dec, reqs, **kw)
    assert lm._packed["kind"] == kind and (lm._packed["qkv_key"] == "merged") is (lora == "merged")
    d = NgramDrafter([plain[i][0].tolist() for i in range(0, len(reqs), 2)])   # every other answer known: right and wrong guesses
    out, st = _run(dec, reqs, draft=d, draft_k=4, **kw)
    assert _same(out, plain), (kind, lora)
    assert st["draft_off"] is None and st["verify_steps"] > 0 and st["draft_accepted"] > 0


def test_the_packed_prefill_with_draft_equals_the_one_request_refill(chain):
    d = NgramDrafter(chain.ids)
    out, st = _run(chain.decs[4], chain.reqs, draft=d, draft_k=4, prefill_batch=4, refill_min=2, **KW)
    assert _same(out, chain.solo) and st["prefill_passes"] < st["prefills"] == 10 and st["verify_steps"] > 0
    want = replay_slot_run(chain.lens, chain.ids, 4, 90, prefill_batch=4, refill_min=2, draft=d, draft_k=4, stop_ids=((835,), (2277, 29937)))
    assert {k: st[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, (st, want)


def test_the_evaluation_scripts_sampling_arguments_are_greedy(chain):
    """do_sample=True, top_p=0.01: the arg-max wherever p_max >= 0.01.  The requests whose logits are peaked to their end (all but
    row1's) draw nothing.  row1 runs past its taught transitions into flat logits over 32,000 ids, where p_max < 0.01 with or
    without `draft` (test_draft_decode_gpu.py leaves it out of this check for that reason): all ten requests draw exactly as
    often as the run without `draft`, and a draw at top_p = 0.01 keeps one candidate, the arg-max."""
    kw = dict(do_sample=True, top_p=0.01, temperature=1.0, **KW)
    peaked = [i for i, r in enumerate(chain.names) if r != "row1"]
    out, st = _run(chain.decs[4], [chain.reqs[i] for i in peaked], draft=NgramDrafter(chain.ids), draft_k=4, **kw)
    assert _same(out, {n: chain.solo[i] for n, i in enumerate(peaked)}) and st["host_sampled_rows"] == 0 and st["verify_steps"] > 0
    ref, ref_st = _run(chain.decs[4], chain.reqs, **kw)
    out, st = _run(chain.decs[4], chain.reqs, draft=NgramDrafter(chain.ids), draft_k=4, **kw)
    assert ref_st["host_sampled_rows"] >= 1                                    # row1's flat tail draws without `draft` too
    assert _same(out, chain.solo) and _same(ref, chain.solo) and st["host_sampled_rows"] == ref_st["host_sampled_rows"]
    assert st["verify_steps"] > 0


def test_one_slot_draws_on_the_host_at_the_same_tokens_as_without_draft(flat, monkeypatch):
    monkeypatch.setattr(flat.lm, "slot_draft", True)
    kw = dict(max_new_tokens=12, stop_ids=(), do_sample=True, top_p=0.9)
    reqs = [flat.emb[0, :7].contiguous(), flat.emb[1, :5].contiguous()]
    dec = flat.lm.slot_decoder(1, 64)
    ref, ref_st = _run(dec, reqs, generator=torch.Generator().manual_seed(5), **kw)
    assert ref_st["host_sampled_rows"] > 0
    for d in (NgramDrafter([ref[i][0].tolist() for i in ref]), Noise(flat.V)):
        out, st = _run(dec, reqs, generator=torch.Generator().manual_seed(5), draft=d, draft_k=4, **kw)
        assert all(torch.equal(out[i][0], ref[i][0]) for i in ref), (type(d).__name__, out, ref)
        assert st["host_sampled_rows"] == ref_st["host_sampled_rows"] and st["verify_steps"] > 0


def test_refusals(chain, monkeypatch):
    lm, dec, d = chain.lm, chain.decs[4], NgramDrafter(chain.ids)
    run = lambda **kw: list(dec.run(chain.reqs[:2], draft=d, **dict(KW, **kw)))
    monkeypatch.setattr(lm, "slot_draft", False)                             # the switch: off, `draft` is refused as before
    with pytest.raises(NotImplementedError, match="MYRIAD_SLOT_DRAFT"):
        run()
    monkeypatch.setattr(lm, "slot_draft", True)
    for kw, what in ((dict(min_length=2), "min_length"), (dict(return_scores=True), "return_scores"), (dict(num_beams=2), "num_beams")):
        with pytest.raises(NotImplementedError, match=what):
            run(**kw)
    with pytest.raises(NotImplementedError, match="repetition_penalty"):
        run(repetition_penalty=1.2)
    with pytest.raises(NotImplementedError, match="run_turns"):
        dec.run_turns([("s", chain.reqs[0], list(range(chain.lens[0])))], draft=d)
    monkeypatch.setattr(lm, "device_sampling", True)
    with pytest.raises(NotImplementedError, match="device sampling"):
        run(do_sample=True, top_p=0.9, top_k=50)
    with pytest.raises(NotImplementedError, match="repetition_penalty"):
        run(repetition_penalty=1.2)
    monkeypatch.setattr(lm, "device_sampling", False)
    for k in (0, 9):
        with pytest.raises(ValueError, match="draft_k"):
            run(draft_k=k)
    with pytest.raises(ValueError, match="rows"):                              # 8 x 8 = 64 rows run, 16 x 8 do not
        list(lm.slot_decoder(16, CAP).run(chain.reqs[:2], draft=d, draft_k=8, **KW))


def test_the_split_kv_view_and_an_unsupported_shape_run_plain_steps_and_say_so(chain, monkeypatch):
    d = NgramDrafter(chain.ids)
    out, st = _run(chain.lm.slot_decoder(4, CAP, split_kv=True), chain.reqs, draft=d, draft_k=4, **KW)
    assert _same(out, chain.solo) and st["draft_off"] == "split_kv" and st["split_kv"] and st["verify_steps"] == 0
    assert st["plain_steps"] == st["steps"] and st["draft_proposed"] == 0
    monkeypatch.setattr(ops, "attn_decode_draft_supported", lambda *a: False)
    out, st = _run(chain.decs[4], chain.reqs, draft=d, draft_k=4, **KW)
    assert _same(out, chain.solo) and st["draft_off"] == "unsupported" and st["verify_steps"] == 0 and st["plain_steps"] == st["steps"]


def test_generate_stream_yields_the_token_ids_of_the_call_without_draft(model, monkeypatch):
    model.eval()
    try:
        with pytest.raises(NotImplementedError, match="MYRIAD_SLOT_DRAFT"):   # off by default
            model.generate_stream(iter([_batch(1, train=False, seed=5)]), slots=2, max_new_tokens=4, draft=NgramDrafter())
        monkeypatch.setattr(model.llama, "slot_draft", True)
        batches = lambda: iter([_batch(3, train=False, seed=5), _batch(2, train=False, seed=6)])
        kw = dict(slots=4, max_new_tokens=12, do_sample=False)
        ref = [o["token_ids"] for o in model.generate_stream(batches(), **kw)]
        ref_st = dict(model.last_generate_stats)
        d = NgramDrafter([t.tolist() for t in ref[::2]])
        out = [o["token_ids"] for o in model.generate_stream(batches(), draft=d, draft_k=4, **kw)]
        st = model.last_generate_stats
        assert len(out) == len(ref) == 5 and all(torch.equal(a, b) for a, b in zip(out, ref))
        assert st["draft_k"] == 4 and st["draft_off"] is None and st["verify_steps"] > 0 and "draft_k" not in ref_st
        with pytest.raises(ValueError):
            list(model.generate_stream(batches(), slots=16, max_new_tokens=4, draft=d, draft_k=8))
    finally:
        model.train()


def test_eval_entry_point_with_slots_writes_the_records_of_the_run_without_draft_k(fx, tmp_path, capsys, monkeypatch):
    import eval_aqa
    monkeypatch.setenv("MYRIAD_SLOT_DRAFT", "1")
    base = ["--cfg-path", fx["eval_yaml"], "--dataset", "synthetic", "--bs", "2", "--limit", "3", "--slots", "4"]
    _, ref = eval_aqa.main(base + ["--out", str(tmp_path / "plain.jsonl")])
    capsys.readouterr()
    path, rec = eval_aqa.main(base + ["--draft-k", "4", "--out", str(tmp_path / "draft.jsonl")])
    assert rec == ref and [json.loads(ln) for ln in open(path)] == [json.loads(ln) for ln in open(tmp_path / "plain.jsonl")]
    assert "draft-and-verify (K = 4)" in capsys.readouterr().out
    _, rec2 = eval_aqa.main(base + ["--draft-k", "4", "--draft-corpus", str(tmp_path / "plain.jsonl"), "--out", str(tmp_path / "d2.jsonl")])
    assert rec2 == ref
