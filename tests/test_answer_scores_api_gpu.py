"""Answer ranking at the public interface, on the model built from the reference's on-disk files (the fixtures of
tests/test_entrypoints_gpu.py): MyriadHIP.score_answers and eval_aqa --rank-answers / --rank-only."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import datasets as D  # noqa: E402
from myriad_amd import eval_protocol as EP  # noqa: E402
from myriad_amd.myriad import MyriadHIP  # noqa: E402
from tests.test_entrypoints_gpu import DEV, _batch, fx, model  # noqa: E402,F401

TODAY = {"image_id", "image_path", "is_anomaly", "error", "output", "anomaly_score"}


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


def test_score_answers_shapes_defaults_and_candidate_forms(model):
    model.eval()
    try:
        tok = model.llama_tokenizer
        samples = _batch(2, train=False, seed=5)
        kw = dict(max_new_tokens=6, stop_ids=((835,), (2277, 29937)), min_length=1)
        before = model.generate(samples, **kw)
        out = model.score_answers(samples)
        assert set(out) == {"answer_logprobs", "answer_token_logprobs", "best", "candidate_ids", "ve_anomaly_maps"}
        lp = out["answer_logprobs"]
        assert lp.shape == (2, 2) and lp.dtype == torch.float64 and bool((lp < 0).all())
        assert out["best"].shape == (2,) and out["best"].dtype == torch.int64 and torch.equal(out["best"], lp.argmax(1))
        assert out["ve_anomaly_maps"].shape == samples["anomaly_maps"].shape
        assert model.last_score_stats["passes"] == 2 and model.last_score_stats["candidates"] == 4
        # the default candidates are the two dataset sentences, tokenised as the training targets are
        pair = [D.ABNORMAL_DESCRIBE, D.NORMAL_DESCRIBE]
        ids = [torch.tensor(tok(c + model.end_sym, add_special_tokens=False).input_ids[:model.max_txt_len]) for c in pair]
        for row, toks in zip(out["candidate_ids"], out["answer_token_logprobs"]):
            assert len(row) == len(toks) == 2
            for got, want, t in zip(row, ids, toks):
                assert torch.equal(got, want) and t.shape == want.shape and t.dtype == torch.float32 and t.device.type == "cpu"
        for b in range(2):
            for c in range(2):
                assert float(lp[b, c]) == float(out["answer_token_logprobs"][b][c].double().sum())
        # a shared list = the same list per sample = the same ids
        for other in (model.score_answers(samples, candidates=pair), model.score_answers(samples, candidates=[pair, pair]),
                      model.score_answers(samples, candidate_ids=ids), model.score_answers(samples, candidate_ids=[ids, ids])):
            assert torch.equal(other["answer_logprobs"], lp) and _same(other["answer_token_logprobs"], out["answer_token_logprobs"])
        mean = model.score_answers(samples, normalize="mean")
        for b in range(2):
            for c in range(2):
                assert float(mean["answer_logprobs"][b, c]) == float(lp[b, c] / len(ids[c]))
        assert _same(mean["answer_token_logprobs"], out["answer_token_logprobs"])
        # ties go to the lower index: a candidate beside its own duplicate
        twice = model.score_answers(samples, candidates=[pair[1], pair[1], pair[0]])
        assert twice["answer_logprobs"].shape == (2, 3) and torch.equal(twice["answer_logprobs"][:, 0], twice["answer_logprobs"][:, 1])
        assert all(int(b) in (0, 2) for b in twice["best"])
        with pytest.raises(ValueError):
            model.score_answers(samples, normalize="median")
        with pytest.raises(ValueError):
            model.score_answers(samples, candidates=pair, candidate_ids=ids)
        with pytest.raises(ValueError):
            model.score_answers(samples, candidates=[pair])          # one list for a batch of two
        # generate() without the new call: today's keys and ids
        after = model.generate(samples, **kw)
        assert set(after) == {"token_ids", "ve_anomaly_maps"} and torch.equal(after["token_ids"], before["token_ids"])
    finally:
        model.train()


def test_the_training_answer_scores_the_training_loss_with_bos(model):
    """bos=True is the training wrap: -answer_logprobs / n_tokens of the sample's own text_input against forward()'s loss at
    batch 1, within the project's 2e-3 relative (header of tests/test_model_gpu.py).  Precondition: every token's probability is
    inside the loss's clamp [1e-7, 1 - 1e-7] by a factor of 10."""
    samples = _batch(1, train=False, seed=7)
    stage, task = model.fixed_stage, model.fixed_taskstage
    model.eval()
    try:
        model.fixed_stage, model.fixed_taskstage = 1, 0              # generate()'s prompt: question2 and the zero-shot maps
        with torch.no_grad():
            loss = float(model(samples)["loss"])
        out = model.score_answers(samples, candidates=[[samples["text_input"][0]]], bos=True)
        toks = out["answer_token_logprobs"][0][0].double()
        pr = torch.exp(toks)
        assert bool((pr >= 1e-6).all()) and bool((pr <= 1 - 1e-6).all()), pr
        got = -float(out["answer_logprobs"][0, 0]) / toks.numel()
        print(f"-mean log-prob {got:.6f}  forward loss {loss:.6f}  rel {abs(got - loss) / abs(loss):.2e}  n = {toks.numel()}")
        assert abs(got - loss) < 2e-3 * abs(loss)
        nobos = model.score_answers(samples, candidates=[[samples["text_input"][0]]])
        assert not torch.equal(nobos["answer_logprobs"], out["answer_logprobs"])       # the BOS row is part of the context
    finally:
        model.fixed_stage, model.fixed_taskstage = stage, task
        model.train()


def _spies(monkeypatch):
    calls = dict(scored=[], generate=0, stream=0)
    score, gen, stream = MyriadHIP.score_answers, MyriadHIP.generate, MyriadHIP.generate_stream

    def spy_score(self, samples, **kw):
        out = score(self, samples, **kw)
        calls["scored"].extend((out["answer_logprobs"][i].clone(), int(out["best"][i])) for i in range(out["best"].shape[0]))
        return out

    def spy_generate(self, samples, **kw):
        calls["generate"] += 1
        return gen(self, samples, **kw)

    def spy_stream(self, batches, **kw):
        calls["stream"] += 1
        return stream(self, batches, **kw)

    monkeypatch.setattr(MyriadHIP, "score_answers", spy_score)
    monkeypatch.setattr(MyriadHIP, "generate", spy_generate)
    monkeypatch.setattr(MyriadHIP, "generate_stream", spy_stream)
    return calls


@pytest.mark.parametrize("slots", [0, 2])
def test_eval_entry_point_writes_the_answer_ranking(fx, tmp_path, monkeypatch, slots):
    import eval_aqa
    calls = _spies(monkeypatch)
    path, records = eval_aqa.main(["--cfg-path", fx["eval_yaml"], "--dataset", "synthetic", "--bs", "2", "--limit", "2", "--slots",
                                   str(slots), "--rank-answers", "--out", str(tmp_path / "res.jsonl")])
    rows = [json.loads(ln) for ln in open(path)]
    assert len(rows) == len(records) == len(calls["scored"]) == 4
    assert (calls["generate"], calls["stream"]) == ((0, 1) if slots else (2, 0))
    pair = [D.ABNORMAL_DESCRIBE, D.NORMAL_DESCRIBE]
    for r, (lp, best) in zip(rows, calls["scored"]):
        assert set(r) == TODAY | {"llm_answer_score", "ranked_output"}
        assert 0.0 <= float(r["llm_answer_score"]) <= 1.0 and r["ranked_output"] == pair[best]
        assert abs(float(r["llm_answer_score"]) - EP.answer_anomaly_score(lp)) <= 0.5e-4 + 1e-9      # str(round(x, 4))


def test_rank_only_never_generates(fx, tmp_path, monkeypatch):
    import eval_aqa
    calls = _spies(monkeypatch)
    for slots in (0, 2):
        path, records = eval_aqa.main(["--cfg-path", fx["eval_yaml"], "--dataset", "synthetic", "--bs", "2", "--limit", "2",
                                       "--slots", str(slots), "--rank-only", "--out", str(tmp_path / f"res{slots}.jsonl")])
        rows = [json.loads(ln) for ln in open(path)]
        assert len(rows) == 4 and (calls["generate"], calls["stream"]) == (0, 0)
        pair = [D.ABNORMAL_DESCRIBE, D.NORMAL_DESCRIBE]
        for r, (lp, best) in zip(rows, calls["scored"][-4:]):
            assert set(r) == TODAY | {"llm_answer_score", "ranked_output"}
            assert r["output"] == r["ranked_output"] == pair[best]
            assert r["error"] == ("0" if (best == 0) == r["is_anomaly"] else "1")     # the existing parsing of "Yes" / "No"
        acc, auc, _ = EP.scene_performance(rows, score_key="llm_answer_score")          # needs no change: the records carry the key
        assert 0.0 <= acc <= 1.0 and 0.0 <= auc <= 1.0


def test_without_the_flags_the_records_have_todays_keys(fx, tmp_path, monkeypatch):
    import eval_aqa
    calls = _spies(monkeypatch)
    path, _ = eval_aqa.main(["--cfg-path", fx["eval_yaml"], "--dataset", "synthetic", "--bs", "2", "--limit", "1", "--out",
                             str(tmp_path / "res.jsonl")])
    rows = [json.loads(ln) for ln in open(path)]
    assert len(rows) == 2 and all(set(r) == TODAY for r in rows) and not calls["scored"] and calls["generate"] == 1
