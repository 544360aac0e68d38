"""Draft-and-verify greedy decoding end to end (LlamaHIP.greedy_generate(draft=...), DecodeSession, eval_aqa.py --draft-k): whatever
the drafter proposes, ids and margins are those of the call without `draft`, bit for bit and with no margin gate -- every row of the
K-row verify step carries the bits of the one-row step at its position -- and the step counts are the ones
decode_host.predict_draft_run works out from the drafter and the true chain."""
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import ops  # noqa: E402
from myriad_amd.decode_host import NgramDrafter, predict_draft_run  # noqa: E402
from myriad_amd.llama import DecodeSession, LlamaHIP  # noqa: E402
from tests import chat_pool_case as C  # noqa: E402
from tests import golden_utils as gu  # noqa: E402
from tests.test_entrypoints_gpu import _batch, fx, model  # noqa: E402,F401

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROWS = ["row0", "row1", "row2", "row3", "stop835"]
COUNTS = ("verify_steps", "plain_steps", "draft_proposed", "draft_accepted")
KW = dict(max_new_tokens=90, min_length=1, return_margins=True)


class Wrong:
    """A drafter whose guesses are never right (id 7 is in no chain)."""

    def propose(self, history, k):
        return [7] * k

    def observe(self, ids):
        pass


class Noise:
    """Seeded random guesses below `vocab`."""

    def __init__(self, vocab, seed=5):
        self.vocab, self.g = vocab, torch.Generator().manual_seed(seed)

    def propose(self, history, k):
        return torch.randint(0, self.vocab, (k,), generator=self.g).tolist()

    def observe(self, ids):
        pass


def _same(a, b):
    """(ids, margins) pairs equal bit for bit."""
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.fixture(scope="module")
def chain():
    """The peaked-chain model and, per row taken alone at B = 1, its input and the plain call's (ids, margins): computed once."""
    lm = LlamaHIP(gu.decode_chain_weights(), gu.DECODE_CHAIN["heads"], DEV, need_backward=False)
    x = {r: gu.decode_chain_inputs([r]).to(DEV) for r in ROWS}
    plain = {r: lm.greedy_generate(x[r], **KW) for r in ROWS}
    assert "verify_steps" not in lm.last_generate_stats
    return types.SimpleNamespace(lm=lm, x=x, plain=plain, ids={r: plain[r][0][0].tolist() for r in ROWS})


@pytest.mark.parametrize("K", [2, 4, 8])
def test_a_drafter_taught_the_chains_gives_the_same_bits_in_the_predicted_steps(chain, K):
    d = NgramDrafter([chain.ids[r] for r in ROWS])
    for r in ROWS:
        out = chain.lm.greedy_generate(chain.x[r], draft=d, draft_k=K, **KW)
        st = chain.lm.last_generate_stats
        assert _same(out, chain.plain[r]), (r, out[0], chain.plain[r][0])
        want = predict_draft_run(d, chain.ids[r], K)
        assert {k: st[k] for k in COUNTS} == want and st["draft_off"] is None and st["draft_k"] == K, (r, st, want)
        L = len(chain.ids[r])
        assert st["steps"] == L
        if r != "row1":          # row1 runs past its taught transitions into flat logits, where a context may repeat: counts only
            assert st["plain_steps"] == 0 and st["verify_steps"] == -(-(L - 1) // K), (r, st)       # K tokens per step to the end
            assert st["draft_accepted"] == (L - 1) - st["verify_steps"]


def test_row_lengths_and_stops_are_those_of_the_fixture(chain):
    """row0: EOS banned at the first pick, the two-token stop ends inside a window; row2: EOS inside a window; stop835."""
    g = np.load(os.path.join(GOLDEN, "decode_chain.npz"))
    assert chain.ids["row0"][-2:] == [2277, 29937] and chain.ids["row0"][0] == 101 and len(chain.ids["row0"]) == 32
    assert chain.ids["row2"] == [301, 302, 303, 2] and chain.ids["stop835"] == [501, 502, 835]
    d = NgramDrafter([chain.ids[r] for r in ROWS])
    for r in ("row0", "row2", "stop835"):
        ids = chain.lm.greedy_generate(chain.x[r], max_new_tokens=90, min_length=1, draft=d, draft_k=4)
        assert ids.tolist() == [chain.ids[r]] and chain.lm.last_generate_stats["verify_steps"] > 0
        if r != "row2":
            assert torch.equal(ids, torch.from_numpy(g[("b1" if r == "row0" else r) + "_ids"]))


def test_an_always_wrong_drafter_costs_one_step_per_token_and_changes_nothing(chain):
    for r in ("row0", "row1"):
        out = chain.lm.greedy_generate(chain.x[r], draft=Wrong(), draft_k=4, **KW)
        st = chain.lm.last_generate_stats
        assert _same(out, chain.plain[r])
        L = len(chain.ids[r])
        assert st["draft_accepted"] == 0 and st["verify_steps"] == L - 1 and st["plain_steps"] == 0 and st["draft_proposed"] == 3 * (L - 1)


def test_a_corrupted_corpus_gives_the_same_bits_and_the_predicted_mix_of_steps(chain):
    r = "row1"                                                             # 45 tokens
    bad = list(chain.ids[r])
    for i in (5, 6, 17, 30):
        bad[i] = 9000 + i
    d = NgramDrafter([bad])
    for K in (4, 8):
        out = chain.lm.greedy_generate(chain.x[r], draft=d, draft_k=K, **KW)
        st = chain.lm.last_generate_stats
        assert _same(out, chain.plain[r])
        want = predict_draft_run(d, chain.ids[r], K)
        assert {k: st[k] for k in COUNTS} == want, (K, st, want)
        assert want["plain_steps"] > 0 and want["verify_steps"] > 0 and 0 < want["draft_accepted"] < want["draft_proposed"]
    assert st["verify_graph_replays"] > 0 and st["plain_graph_replays"] > 0          # both views replay a graph of their own
    assert st["graph_replays"] == st["verify_graph_replays"] + st["plain_graph_replays"]


def test_the_evaluation_scripts_sampling_arguments(chain):
    kw = dict(do_sample=True, top_p=0.01, temperature=1.0, **KW)
    d = NgramDrafter([chain.ids[r] for r in ROWS])
    for r in ("row0", "row3"):
        ref = chain.lm.greedy_generate(chain.x[r], **kw)
        ref_st = dict(chain.lm.last_generate_stats)
        out = chain.lm.greedy_generate(chain.x[r], draft=d, draft_k=4, **kw)
        st = chain.lm.last_generate_stats
        assert _same(out, ref) and _same(out, chain.plain[r])
        assert st["sampled_rows"] == 0 and st["min_pmax"] == ref_st["min_pmax"] and st["verify_steps"] > 0


# ------------------------------------------------------------------------------------------------ flat logits
@pytest.fixture(scope="module")
def flat():
    """test_flat_logit_decode_ids_equal_up_to_the_first_two_ulp_near_tie's fixture: std-0.2 random weights, V = 320."""
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(GOLDEN, "llama_tiny.npz")).items()}
    D, layers, heads, inter, V, seed = [int(x) for x in g["meta"]]
    sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() and v.numel() > 4096 else v)
          for k, v in gu.llama_weights(D, layers, inter, V, seed=seed, std=0.2).items()}
    return types.SimpleNamespace(lm=LlamaHIP(sd, heads, DEV, need_backward=False), emb=g["emb"], V=V)


def test_flat_logits_ids_and_margins_are_bit_equal_with_no_margin_gate(flat):
    kw = dict(max_new_tokens=40, stop_ids=(), return_margins=True)
    for r, s0 in ((0, 5), (1, 9)):
        e = flat.emb[r:r + 1, :s0].to(DEV)
        ref = flat.lm.greedy_generate(e, **kw)
        for d in (NgramDrafter([ref[0][0].tolist()]), Noise(flat.V)):
            out = flat.lm.greedy_generate(e, draft=d, draft_k=4, **kw)
            st = flat.lm.last_generate_stats
            assert _same(out, ref), (r, s0, type(d).__name__, out[0], ref[0])
            assert st["draft_off"] is None and st["verify_steps"] > 0
            if isinstance(d, NgramDrafter):
                assert {k: st[k] for k in COUNTS} == predict_draft_run(d, ref[0][0].tolist(), 4)


def test_flat_logits_host_draws_happen_at_the_same_tokens_in_the_same_order(flat):
    kw = dict(max_new_tokens=12, stop_ids=(), do_sample=True, top_p=0.9)
    e = flat.emb[:1, :7].to(DEV)
    ref = flat.lm.greedy_generate(e, generator=torch.Generator().manual_seed(5), **kw)
    ref_st = dict(flat.lm.last_generate_stats)
    assert ref_st["host_sampled_rows"] > 0
    for d in (NgramDrafter([ref[0].tolist()]), Noise(flat.V)):
        out = flat.lm.greedy_generate(e, generator=torch.Generator().manual_seed(5), draft=d, draft_k=4, **kw)
        st = flat.lm.last_generate_stats
        assert torch.equal(out, ref), (type(d).__name__, out, ref)
        assert st["host_sampled_rows"] == ref_st["host_sampled_rows"] and st["sampled_rows"] == ref_st["sampled_rows"]
        assert st["verify_steps"] > 0


# ------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("lora", ["bordered", "merged"])
@pytest.mark.parametrize("kind", ["bf16", "fp8", "fp4"])
def test_every_kind_of_decode_weights_is_bit_equal_to_its_plain_call(kind, lora):
    from tests.test_fp4_decode_gpu import _lora_model
    emb, _, _, lm = _lora_model()
    lm.decode_fp8, lm.decode_fp4, lm.decode_merge_lora = kind == "fp8", kind == "fp4", lora == "merged"
    kw = dict(max_new_tokens=24, stop_ids=(), return_margins=True)
    e = emb[:1, :7].to(DEV)
    ref = lm.greedy_generate(e, **kw)
    assert lm.last_generate_stats["decode_weights"] == kind and lm.last_generate_stats["lora_merged"] is (lora == "merged")
    out = lm.greedy_generate(e, draft=NgramDrafter([ref[0][0].tolist()]), draft_k=4, **kw)
    st = lm.last_generate_stats
    assert _same(out, ref), (out[0], ref[0])
    assert st["decode_weights"] == kind and st["lora_merged"] is (lora == "merged") and st["draft_off"] is None
    assert st["verify_steps"] > 0 and st["draft_accepted"] > 0


# ------------------------------------------------------------------------------------------------ DecodeSession
def _two_turns(lm, emb_w, split, draft=None):
    sess = DecodeSession(lm, C.CAPACITY, split=split)
    kw = dict(max_new_tokens=C.MAX_NEW, stop_ids=C.STOPS, eos_id=C.EOS, min_length=1)
    if draft is not None:
        kw.update(draft=draft, draft_k=4)
    ctx, keys = C.first_turn("a", emb_w)
    ids1 = sess.generate(ctx[None].to(DEV), [keys], weights_version=0, **kw)[0].tolist()
    st1 = dict(sess.last_stats)
    ctx, keys = C.next_turn("a", 1, ctx, keys, ids1, emb_w[ids1].to(torch.bfloat16).float(), emb_w)
    ids2 = sess.generate(ctx[None].to(DEV), [keys], weights_version=0, **kw)[0].tolist()
    return [ids1, ids2], [st1, dict(sess.last_stats)]


def test_a_session_with_draft_decodes_and_reuses_what_a_session_without_it_does(chain):
    emb_w = gu.decode_chain_weights()["llama_model.model.embed_tokens.weight"]
    ids, st = _two_turns(chain.lm, emb_w, False)
    d = NgramDrafter(ids)
    ids_d, st_d = _two_turns(chain.lm, emb_w, False, draft=d)
    assert ids_d == ids and [s["reused_tokens"] for s in st_d] == [s["reused_tokens"] for s in st] and st_d[1]["reused_tokens"] > 0
    assert all(s["draft_off"] is None and s["verify_steps"] > 0 for s in st_d) and st_d[0]["draft_accepted"] > 0
    ids_s, st_s = _two_turns(chain.lm, emb_w, True, draft=d)                # the split-KV view decodes with plain steps
    assert ids_s == ids and all(s["draft_off"] == "split_kv" and s["verify_steps"] == 0 and s["split_kv"] for s in st_s)
    assert [s["reused_tokens"] for s in st_s] == [s["reused_tokens"] for s in st]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(chain, monkeypatch):
    lm, d = chain.lm, NgramDrafter([chain.ids["row0"]])
    x = chain.x["row0"]
    with pytest.raises(NotImplementedError):
        lm.greedy_generate(gu.decode_chain_inputs(["row0", "row1"]).to(DEV), draft=d)                # B > 1
    with pytest.raises(NotImplementedError):
        lm.greedy_generate(x, draft=d, repetition_penalty=1.2)
    with pytest.raises(NotImplementedError):
        lm.greedy_generate(x, draft=d, return_scores=True)
    for k in (0, 9):
        with pytest.raises(ValueError):
            lm.greedy_generate(x, draft=d, draft_k=k)
    monkeypatch.setattr(lm, "device_sampling", True)
    with pytest.raises(NotImplementedError):
        lm.greedy_generate(x, draft=d, do_sample=True, top_p=0.9, top_k=50)                          # device sampling
    monkeypatch.setattr(lm, "device_sampling", False)
    monkeypatch.setattr(lm, "decode_fused", False)
    with pytest.raises(ValueError, match="fused packed token step"):
        lm.greedy_generate(x, draft=d)
    monkeypatch.setattr(lm, "decode_fused", True)
    sess = DecodeSession(lm, 128)
    with pytest.raises(NotImplementedError):
        sess.generate(gu.decode_chain_inputs(["row0", "row1"]).to(DEV), [[("r", b, j) for j in range(6)] for b in range(2)], draft=d)
    with pytest.raises(ValueError, match="rotary table"):
        lm.greedy_generate(x, draft=d, draft_k=8, max_new_tokens=lm.cos.shape[0] - x.shape[1] - 4)
    # beams: the public entries refuse (beam_generate has no such argument)
    from myriad_amd.myriad import MyriadHIP
    stub = types.SimpleNamespace(pad_id=2, llama=lm)
    with pytest.raises(NotImplementedError, match="draft"):
        MyriadHIP._generate_args(stub, dict(max_new_tokens=5, num_beams=2, draft=d))
    a = MyriadHIP._generate_args(stub, dict(max_new_tokens=5, draft=d, draft_k=3))
    assert a["draft"] is d and a["draft_k"] == 3 and MyriadHIP._generate_args(stub, dict(max_new_tokens=5))["draft"] is None


def test_an_unsupported_shape_runs_plain_steps_and_says_so(chain, monkeypatch):
    monkeypatch.setattr(ops, "attn_decode_draft_supported", lambda *a: False)
    d = NgramDrafter([chain.ids["row0"]])
    out = chain.lm.greedy_generate(chain.x["row0"], draft=d, draft_k=4, **KW)
    st = chain.lm.last_generate_stats
    assert _same(out, chain.plain["row0"]) and st["draft_off"] == "unsupported"
    assert st["verify_steps"] == 0 and st["plain_steps"] == len(chain.ids["row0"]) - 1 and st["draft_proposed"] == 0


# ------------------------------------------------------------------------------------------------ eval_aqa.py
def test_generate_and_the_chat_take_the_arguments_and_return_what_they_return_without_them(model):
    from myriad_amd.chat import CONV_VISION, Chat
    model.eval()
    try:
        one = _batch(1, train=False, seed=5)
        ref = model.generate(one, max_new_tokens=12)["token_ids"]
        d = NgramDrafter([ref[0].tolist()])
        out = model.generate(one, max_new_tokens=12, draft=d, draft_k=4)["token_ids"]
        st = model.last_generate_stats
        assert torch.equal(out, ref) and st["draft_off"] is None and st["verify_steps"] > 0 and st["draft_accepted"] > 0
        for bad in (lambda: model.generate(_batch(2, train=False, seed=5), max_new_tokens=4, draft=d),
                    lambda: model.generate(one, max_new_tokens=4, draft=d, num_beams=2),
                    lambda: model.generate_stream(iter([one]), slots=2, max_new_tokens=4, draft=d)):
            with pytest.raises(NotImplementedError):
                bad()

        def two_turns(**kw):
            chat, conv, imgs, outs = Chat(model, device=DEV), CONV_VISION.copy(), [], []
            chat.upload_img(one["image"][:1], conv, imgs, anomaly_maps=one["anomaly_maps"][:1])
            for q in ("Is there a defect?", "Where is it?"):
                chat.ask(q, conv)
                chat.answer(conv, imgs, max_new_tokens=12, do_sample=False, **kw)
                outs.append((chat.last_token_ids[0].tolist(), dict(chat.last_stats)))
            return outs

        plain = two_turns()
        got = two_turns(draft=NgramDrafter([ids for ids, _ in plain]), draft_k=4)
        assert [ids for ids, _ in got] == [ids for ids, _ in plain]
        assert [s_["reused_tokens"] for _, s_ in got] == [s_["reused_tokens"] for _, s_ in plain] and got[1][1]["reused_tokens"] > 0
        assert all(s_["draft_off"] is None and s_["verify_steps"] > 0 for _, s_ in got) and "draft_off" not in plain[0][1]
        with pytest.raises(NotImplementedError):
            chat, conv, imgs = Chat(model, device=DEV), CONV_VISION.copy(), []
            chat.upload_img(one["image"][:1], conv, imgs, anomaly_maps=one["anomaly_maps"][:1])
            chat.ask("Is there a defect?", conv)
            chat.answer(conv, imgs, max_new_tokens=4, num_beams=2, draft=d)
    finally:
        model.train()


def test_eval_entry_point_writes_the_records_of_the_run_without_it(fx, tmp_path, capsys):
    import eval_aqa
    base = ["--cfg-path", fx["eval_yaml"], "--dataset", "synthetic", "--bs", "1", "--limit", "3"]
    _, ref = eval_aqa.main(base + ["--out", str(tmp_path / "plain.jsonl")])
    path, rec = eval_aqa.main(base + ["--draft-k", "4", "--out", str(tmp_path / "draft.jsonl")])
    assert rec == ref and [json.loads(ln) for ln in open(path)] == [json.loads(ln) for ln in open(tmp_path / "plain.jsonl")]
    assert "draft-and-verify (K = 4)" in capsys.readouterr().out
    # an earlier run's results teach the drafter up front
    _, rec2 = eval_aqa.main(base + ["--draft-k", "4", "--draft-corpus", str(tmp_path / "plain.jsonl"), "--out", str(tmp_path / "d2.jsonl")])
    assert rec2 == ref
    for bad in (["--draft-k", "4", "--bs", "2"], ["--draft-k", "4", "--slots", "2"], ["--draft-corpus", "x.json"], ["--draft-k", "9"]):
        with pytest.raises(SystemExit):
            eval_aqa.parse_args(["--cfg-path", fx["eval_yaml"]] + bad)
