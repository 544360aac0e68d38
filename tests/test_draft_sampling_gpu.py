"""Draft-and-verify decoding in the decode slots under the device sampler, the repetition penalty, min_length > 1 and the token
scores (behind `draft_sampling`, MYRIAD_DRAFT_SAMPLING=1).  The contract is the greedy one, extended: row (g, j) of the verify step
draws / penalises / bans exactly as the plain step does for token gen[g] + j of that request, so with the switch on every request's
ids, margins, sampled-row counts and scores are bit for bit those of the run without `draft` -- and of greedy_generate on that
request alone with the same seed -- whatever the drafter proposes.  A taught drafter's step counts are the ones
decode_host.replay_slot_run works out without a device, and fewer than the plain run's: the verify path is really taken."""
import json
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd.decode_host import NgramDrafter, predict_draft_run, replay_slot_run  # noqa: E402
from myriad_amd.llama import DecodeSession, LlamaHIP  # noqa: E402
from tests import golden_utils as gu  # noqa: E402
from tests.test_draft_decode_gpu import Noise, Wrong, flat  # noqa: E402,F401
from tests.test_draft_decode_gpu import chain as solo_chain  # noqa: E402,F401
from tests.test_entrypoints_gpu import _batch, fx, model  # noqa: E402,F401
from tests.test_draft_slots_gpu import CAP, COUNTS, DEV, EXTRA, ROWS, _bits  # noqa: E402

STOPS = ((835,), (2277, 29937))
KW = dict(max_new_tokens=90, min_length=1)
MODES = {
    "sampled": dict(do_sample=True, top_p=0.9, top_k=50),                      # the device draws; the chains are peaked
    "penalty": dict(repetition_penalty=1.2),                                   # greedy + penalty
    "sampled+penalty": dict(do_sample=True, top_p=0.9, top_k=50, temperature=1.5, repetition_penalty=1.2),
    "min_length": dict(min_length=3),                                          # the ban ends inside a window
    "min_length5": dict(min_length=5),                                         # ... and holds row2's EOS (its 4th token) back
    "scores": dict(return_scores=True, watch_ids=(2, 835)),
    "scores+host": dict(return_scores=True, watch_ids=(2, 835), do_sample=True, top_p=0.01),
    "scores+sampled": dict(return_scores=True, watch_ids=(2, 835), do_sample=True, top_p=0.9, top_k=50, temperature=1.5),
}
DEVICE = ("sampled", "sampled+penalty", "scores+sampled")                      # the modes that run with device_sampling on


def _run(dec, reqs, seed=5, **kw):
    out = {r[0]: r[1:] for r in dec.run(reqs, generator=torch.Generator().manual_seed(seed), **kw)}
    return out, dict(dec.last_stats)


def _same(a, b):
    """{index: (ids, margins[, scores])} equal bit for bit."""
    if a.keys() != b.keys():
        return False
    for i in a:
        if not (torch.equal(a[i][0], b[i][0]) and torch.equal(_bits(a[i][1]), _bits(b[i][1])) and len(a[i]) == len(b[i])):
            return False
        if len(a[i]) == 3 and not all(torch.equal(_bits(a[i][2][k]), _bits(b[i][2][k])) for k in ("token_logprobs", "watch_logprobs")):
            return False
    return True


def _alone(lm, reqs, seed=5, **kw):
    """greedy_generate on every request alone, one generator across the calls: the seeds the slot run hands out."""
    g, out = torch.Generator().manual_seed(seed), {}
    for i, e in enumerate(reqs):
        r = lm.greedy_generate(e[None].to(DEV), return_margins=True, generator=g, **kw)
        out[i] = (r[0][0].cpu(), r[1][0].cpu()) + ((dict(token_logprobs=r[2]["token_logprobs"][0].cpu(),
                                                         watch_logprobs=r[2]["watch_logprobs"][0].cpu()),) if len(r) > 2 else ())
    return out


def _switches(lm, mode):
    lm.slot_draft, lm.draft_sampling = True, True
    lm.device_sampling = mode in DEVICE or "penalty" in mode                   # the penalty needs the sampling switch too


@pytest.fixture(scope="module")
def chain():
    """test_draft_slots_gpu's model and ten ragged requests, with a model of its own (the switches differ) and engines at 2 and 8
    slots; per mode the run without `draft`, computed once."""
    lm = LlamaHIP(gu.decode_chain_weights(), gu.DECODE_CHAIN["heads"], DEV, need_backward=False)
    assert lm.draft_sampling is False                                          # off by default
    g = torch.Generator().manual_seed(31)
    names = ROWS + ROWS
    reqs = [torch.cat([torch.randn(n, gu.DECODE_CHAIN["D"], generator=g) * 0.3, gu.decode_chain_inputs([r])[0]]) for r, n in zip(names, EXTRA)]
    ns = types.SimpleNamespace(lm=lm, reqs=reqs, names=names, lens=[int(e.shape[0]) for e in reqs],
                               decs={s: lm.slot_decoder(s, CAP) for s in (2, 8)}, plain={})

    def plain(mode, slots):
        if (mode, slots) not in ns.plain:
            _switches(lm, mode)
            ns.plain[mode, slots] = _run(ns.decs[slots], reqs, **dict(KW, **MODES[mode]))
        return ns.plain[mode, slots]
    ns.plain_of = plain
    return ns


def _drafter(kind, ids):
    return {"taught": lambda: NgramDrafter(ids), "wrong": Wrong, "noise": lambda: Noise(gu.DECODE_CHAIN["vocab"], seed=9)}[kind]()


@pytest.mark.parametrize("kind", ["taught", "wrong", "noise"])
@pytest.mark.parametrize("slots,K", [(2, 4), (8, 8)])
@pytest.mark.parametrize("mode", list(MODES))
def test_every_request_has_the_bits_of_the_run_without_draft(chain, mode, slots, K, kind):
    plain, plain_st = chain.plain_of(mode, slots)
    _switches(chain.lm, mode)
    kw = dict(KW, **MODES[mode])
    ids = [plain[i][0].tolist() for i in range(len(chain.reqs))]
    out, st = _run(chain.decs[slots], chain.reqs, draft=_drafter(kind, ids), draft_k=K, **kw)
    assert _same(out, plain), (mode, slots, K, kind)
    for k in ("device_sampled_rows", "host_sampled_rows"):
        assert st[k] == plain_st[k], (k, st[k], plain_st[k])
    assert st["draft_off"] is None and st["verify_steps"] > 0 and st["steps"] == st["verify_steps"] + st["plain_steps"]
    if mode in DEVICE:
        assert st["device_sampled_rows"] == sum(len(i) for i in ids) and st["host_sampled_rows"] == 0
    if kind == "taught":                                                       # the counts the host works out without a device
        assert st["draft_accepted"] > 0 and st["verify_steps"] < plain_st["steps"]
        if st["host_sampled_rows"] == 0:                                       # (a host draw ends a window: row1's flat tail at top_p 0.01)
            want = replay_slot_run(chain.lens, ids, slots, 90, draft=NgramDrafter(ids), draft_k=K, stop_ids=STOPS)
            assert {k: st[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, (st, want)
        assert st["host_sampled_rows"] == 0 or mode == "scores+host"
    if kind == "wrong":
        assert st["draft_accepted"] == 0 and st["steps"] == plain_st["steps"]


@pytest.mark.parametrize("mode", list(MODES))
def test_every_request_has_the_bits_of_greedy_generate_alone_with_the_same_seed(chain, mode):
    plain, _ = chain.plain_of(mode, 2)
    _switches(chain.lm, mode)
    alone = _alone(chain.lm, chain.reqs, **dict(KW, **MODES[mode]))
    assert _same(plain, alone), mode
    if mode == "min_length5":                                                  # the ban changed an answer: row2 stops at its 4th token without it
        assert all(len(plain[i][0]) > 4 for i, r in enumerate(chain.names) if r == "row2")


def test_an_untaught_drafter_replays_only_the_plain_graph(chain):
    chain.plain_of("sampled+penalty", 2)                                       # (the view's graph exists from here on)
    _switches(chain.lm, "sampled+penalty")
    plain, plain_st = _run(chain.decs[2], chain.reqs, **dict(KW, **MODES["sampled+penalty"]))
    out, st = _run(chain.decs[2], chain.reqs, draft=NgramDrafter(), draft_k=4, **dict(KW, **MODES["sampled+penalty"]))
    assert _same(out, plain) and st["verify_steps"] == 0 and st["plain_steps"] == st["steps"] == plain_st["steps"]
    assert st["verify_graph_replays"] == 0 and st["plain_graph_replays"] == st["graph_replays"] == plain_st["graph_replays"] > 0


@pytest.mark.parametrize("penalty", [1.0, 1.3])
def test_flat_logits_where_every_pick_is_a_draw(flat, monkeypatch, penalty):
    lm = flat.lm
    for name in ("slot_draft", "draft_sampling", "device_sampling"):
        monkeypatch.setattr(lm, name, True)
    kw = dict(max_new_tokens=24, stop_ids=(), do_sample=True, top_p=0.95, top_k=50, temperature=2.0, repetition_penalty=penalty)
    reqs = [flat.emb[r, :s0].contiguous() for r, s0 in ((0, 5), (1, 9), (0, 7), (1, 6), (0, 8), (1, 4))]
    dec = lm.slot_decoder(4, 64)
    plain, plain_st = _run(dec, reqs, **kw)
    assert _same(plain, _alone(lm, reqs, **kw))
    greedy, _ = _run(dec, reqs, max_new_tokens=24, stop_ids=())
    assert sum(plain[i][0].tolist() != greedy[i][0].tolist() for i in plain) >= 4     # draws, not the arg-max
    ids = [plain[i][0].tolist() for i in range(len(reqs))]
    for d in (NgramDrafter(ids), Noise(flat.V), NgramDrafter(ids[::2])):
        out, st = _run(dec, reqs, draft=d, draft_k=4, **kw)
        assert _same(out, plain), type(d).__name__
        assert st["device_sampled_rows"] == plain_st["device_sampled_rows"] == sum(len(i) for i in ids) and st["verify_steps"] > 0
    assert st["draft_accepted"] > 0


@pytest.mark.parametrize("kind,lora", [("fp8", "bordered"), ("fp4", "bordered"), ("bf16", "merged")])
def test_every_kind_of_decode_weights_is_bit_equal_to_its_own_run_without_draft(kind, lora):
    from tests.test_fp4_decode_gpu import _lora_model
    emb, _, _, lm = _lora_model()
    lm.decode_fp8, lm.decode_fp4, lm.decode_merge_lora = kind == "fp8", kind == "fp4", lora == "merged"
    lm.slot_draft = lm.draft_sampling = lm.device_sampling = True
    kw = dict(max_new_tokens=24, stop_ids=(), do_sample=True, top_p=0.9, top_k=50, temperature=1.5, repetition_penalty=1.2,
              return_scores=True, watch_ids=(1, 3))
    reqs = [emb[r, :s0].contiguous() for r, s0 in ((0, 7), (1, 5), (2, 9), (0, 4), (1, 12), (2, 6))]
    dec = lm.slot_decoder(4, 64)
    plain, _ = _run(dec, reqs, **kw)
    assert lm._packed["kind"] == kind and (lm._packed["qkv_key"] == "merged") is (lora == "merged")
    d = NgramDrafter([plain[i][0].tolist() for i in range(0, len(reqs), 2)])   # every other answer known: right and wrong guesses
    out, st = _run(dec, reqs, draft=d, draft_k=4, **kw)
    assert _same(out, plain), (kind, lora)
    assert st["draft_off"] is None and st["verify_steps"] > 0 and st["draft_accepted"] > 0


def test_the_packed_prefill_with_draft_equals_the_one_request_refill(chain):
    mode = "sampled+penalty"
    plain, _ = chain.plain_of(mode, 8)
    _switches(chain.lm, mode)
    ids = [plain[i][0].tolist() for i in range(len(chain.reqs))]
    d = NgramDrafter(ids)
    out, st = _run(chain.decs[8], chain.reqs, draft=d, draft_k=4, prefill_batch=4, refill_min=2, **dict(KW, **MODES[mode]))
    assert _same(out, plain) and st["prefill_passes"] < st["prefills"] == 10 and st["verify_steps"] > 0
    want = replay_slot_run(chain.lens, ids, 8, 90, prefill_batch=4, refill_min=2, draft=d, draft_k=4, stop_ids=STOPS)
    assert {k: st[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, (st, want)


def test_refusals(chain, monkeypatch):
    lm, dec = chain.lm, chain.decs[2]
    d = NgramDrafter()
    run = lambda **kw: list(dec.run(chain.reqs[:2], draft=d, **dict(KW, **kw)))
    for name, v in (("slot_draft", True), ("device_sampling", True), ("draft_sampling", False)):
        monkeypatch.setattr(lm, name, v)
    for kw, what in ((dict(min_length=2), "min_length"), (dict(return_scores=True), "return_scores"),
                     (dict(repetition_penalty=1.2), "repetition_penalty"), (dict(do_sample=True, top_p=0.9, top_k=50), "device sampling")):
        with pytest.raises(NotImplementedError, match=what):                  # the switch off: refused as before
            run(**kw)
    monkeypatch.setattr(lm, "draft_sampling", True)
    for kw in (dict(min_length=2), dict(return_scores=True), dict(repetition_penalty=1.2), dict(do_sample=True, top_p=0.9, top_k=50)):
        assert len(run(**kw)) == 2
    with pytest.raises(NotImplementedError, match="num_beams"):               # still refused with it on
        run(num_beams=2)
    with pytest.raises(NotImplementedError, match="run_turns"):
        dec.run_turns([("s", chain.reqs[0], list(range(chain.lens[0])))], draft=d)
    monkeypatch.setattr(lm, "slot_draft", False)
    with pytest.raises(NotImplementedError, match="MYRIAD_SLOT_DRAFT"):
        run(repetition_penalty=1.2)


# ------------------------------------------------------------------------------------------------ one request (G = 1)
SOLO_COUNTS = ("verify_steps", "plain_steps", "draft_proposed", "draft_accepted")


def _solo(lm, x, seed=5, **kw):
    r = lm.greedy_generate(x, return_margins=True, generator=torch.Generator().manual_seed(seed), **kw)
    st = dict(lm.last_generate_stats)
    out = (r[0][0].cpu(), r[1][0].cpu()) + ((dict(token_logprobs=r[2]["token_logprobs"][0].cpu(),
                                                  watch_logprobs=r[2]["watch_logprobs"][0].cpu()),) if len(r) > 2 else ())
    return out, st


@pytest.mark.parametrize("K", [2, 4, 8])
@pytest.mark.parametrize("mode", [m for m in MODES if not m.startswith("min_length")])
def test_one_request_has_the_bits_of_the_call_without_draft(solo_chain, monkeypatch, mode, K):
    lm = solo_chain.lm
    monkeypatch.setattr(lm, "draft_sampling", True)
    monkeypatch.setattr(lm, "device_sampling", mode in DEVICE or "penalty" in mode)
    kw = dict(KW, **MODES[mode])
    for r in ("row0", "row1", "stop835"):
        ref, ref_st = _solo(lm, solo_chain.x[r], **kw)
        ids = ref[0].tolist()
        for d in (NgramDrafter([ids]), Wrong(), Noise(gu.DECODE_CHAIN["vocab"], seed=3)):
            out, st = _solo(lm, solo_chain.x[r], draft=d, draft_k=K, **kw)
            assert _same({0: out}, {0: ref}), (mode, K, r, type(d).__name__, out[0], ref[0])
            for k in ("device_sampled_rows", "host_sampled_rows", "sampled_rows", "steps"):
                assert st[k] == ref_st[k], (k, st[k], ref_st[k])
            assert st["draft_off"] is None and st["verify_steps"] > 0
            if isinstance(d, NgramDrafter):                                    # the path is taken, in the predicted steps
                assert st["verify_steps"] < len(ids) - 1 and st["draft_accepted"] > 0
                if st["host_sampled_rows"] == 0:                               # (a host draw ends a window: row1's flat tail at top_p 0.01)
                    assert {k: st[k] for k in SOLO_COUNTS} == predict_draft_run(d, ids, K), (mode, K, r)
                assert st["host_sampled_rows"] == 0 or (mode, r) == ("scores+host", "row1")
        if mode in DEVICE:
            assert ref_st["device_sampled_rows"] == len(ids) and ref_st["host_sampled_rows"] == 0


def test_one_request_on_flat_logits_where_every_pick_is_a_draw(flat, monkeypatch):
    lm = flat.lm
    for name in ("draft_sampling", "device_sampling"):
        monkeypatch.setattr(lm, name, True)
    kw = dict(max_new_tokens=24, stop_ids=(), do_sample=True, top_p=0.95, top_k=50, temperature=2.0, repetition_penalty=1.3,
              return_scores=True, watch_ids=(1, 3))
    e = flat.emb[:1, :7].to(DEV)
    ref, ref_st = _solo(lm, e, **kw)
    greedy, _ = _solo(lm, e, max_new_tokens=24, stop_ids=())
    n = len(ref[0])
    assert ref[0].tolist() != greedy[0].tolist() and ref_st["device_sampled_rows"] == n > 4
    for d in (NgramDrafter([ref[0].tolist()]), Noise(flat.V)):
        out, st = _solo(lm, e, draft=d, draft_k=4, **kw)
        assert _same({0: out}, {0: ref}), (type(d).__name__, out[0], ref[0])
        assert st["device_sampled_rows"] == n and st["verify_steps"] > 0
    assert _same({0: _solo(lm, e, draft=NgramDrafter(), draft_k=4, **kw)[0]}, {0: ref})        # untaught: plain steps only
    assert lm.last_generate_stats["verify_steps"] == 0


def test_one_request_refusals(solo_chain, monkeypatch):
    lm, d, x = solo_chain.lm, NgramDrafter(), solo_chain.x["row0"]
    monkeypatch.setattr(lm, "device_sampling", True)
    assert lm.draft_sampling is False
    for kw in (dict(repetition_penalty=1.2), dict(return_scores=True), dict(do_sample=True, top_p=0.9, top_k=50)):
        with pytest.raises(NotImplementedError):                              # the switch off: refused as before
            lm.greedy_generate(x, draft=d, **kw)
        with pytest.raises(NotImplementedError):
            DecodeSession(lm, 128).generate(x, [[("r", j) for j in range(x.shape[1])]], draft=d, **kw)
    monkeypatch.setattr(lm, "draft_sampling", True)
    with pytest.raises(NotImplementedError):                                  # still one sequence only
        lm.greedy_generate(gu.decode_chain_inputs(["row0", "row1"]).to(DEV), draft=d, repetition_penalty=1.2)


# ------------------------------------------------------------------------------------------------ the public entries
def test_a_chat_turn_with_draft_and_a_penalty_equals_the_turn_without_draft(model, monkeypatch):
    from myriad_amd.chat import CONV_VISION, Chat
    model.eval()
    try:
        for name in ("device_sampling", "draft_sampling"):
            monkeypatch.setattr(model.llama, name, True)
        one = _batch(1, train=False, seed=5)

        def two_turns(**kw):
            chat, conv, imgs, outs = Chat(model, device=DEV), CONV_VISION.copy(), [], []
            chat.upload_img(one["image"][:1], conv, imgs, anomaly_maps=one["anomaly_maps"][:1])
            for q in ("Is there a defect?", "Where is it?"):
                chat.ask(q, conv)
                chat.answer(conv, imgs, max_new_tokens=12, repetition_penalty=1.1, generator=torch.Generator().manual_seed(3), **kw)
                outs.append((chat.last_token_ids[0].tolist(), dict(chat.last_stats)))
            return outs

        plain = two_turns()
        got = two_turns(draft=NgramDrafter([ids for ids, _ in plain]), draft_k=4)
        assert [ids for ids, _ in got] == [ids for ids, _ in plain]
        assert [s_["reused_tokens"] for _, s_ in got] == [s_["reused_tokens"] for _, s_ in plain]
        assert all(s_["draft_off"] is None and s_["verify_steps"] > 0 for _, s_ in got)
        monkeypatch.setattr(model.llama, "draft_sampling", False)
        with pytest.raises(NotImplementedError):
            two_turns(draft=NgramDrafter(), draft_k=4)
    finally:
        model.train()


@pytest.mark.parametrize("slots", [0, 4])
def test_eval_entry_point_with_llm_score_writes_the_records_of_the_run_without_draft_k(fx, tmp_path, capsys, monkeypatch, slots):
    import eval_aqa
    base = ["--cfg-path", fx["eval_yaml"], "--dataset", "synthetic", "--limit", "3", "--llm-score"]
    base += ["--bs", "2", "--slots", "4"] if slots else ["--bs", "1"]
    monkeypatch.setenv("MYRIAD_SLOT_DRAFT", "1")
    monkeypatch.delenv("MYRIAD_DRAFT_SAMPLING", raising=False)
    with pytest.raises(SystemExit):                                           # the switch off: refused as before
        eval_aqa.main(base + ["--draft-k", "4", "--out", str(tmp_path / "no.jsonl")])
    monkeypatch.setenv("MYRIAD_DRAFT_SAMPLING", "1")
    _, ref = eval_aqa.main(base + ["--out", str(tmp_path / "plain.jsonl")])
    capsys.readouterr()
    path, rec = eval_aqa.main(base + ["--draft-k", "4", "--draft-corpus", str(tmp_path / "plain.jsonl"), "--out", str(tmp_path / "d.jsonl")])
    rows = [json.loads(ln) for ln in open(path)]
    assert rec == ref and rows == [json.loads(ln) for ln in open(tmp_path / "plain.jsonl")]
    assert all("llm_anomaly_score" in r for r in rows) and "draft-and-verify (K = 4)" in capsys.readouterr().out
