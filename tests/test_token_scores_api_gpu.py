"""Token scores at the public interface, on the model built from the reference's on-disk files (the fixtures of
tests/test_entrypoints_gpu.py): MyriadHIP.generate(output_scores=True, watch_ids=...), generate_stream, eval_aqa --llm-score."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import datasets as D  # noqa: E402
from myriad_amd.myriad import MyriadHIP  # noqa: E402
from tests.test_entrypoints_gpu import DEV, _batch, fx, model  # noqa: E402,F401


def test_generate_returns_the_scores_and_the_stream_agrees_per_sample(model):
    model.eval()
    try:
        kw = dict(max_new_tokens=6, stop_ids=((835,), (2277, 29937)), min_length=1)
        samples = _batch(2, train=False, seed=5)
        plain = model.generate(samples, **kw)
        assert set(plain) == {"token_ids", "ve_anomaly_maps"}                          # without the flag: today's keys
        out = model.generate(samples, output_scores=True, watch_ids=[3, 5, 7], **kw)
        L = out["token_ids"].shape[1]
        assert set(out) == set(plain) | {"token_logprobs", "watch_logprobs"} and torch.equal(out["token_ids"], plain["token_ids"])
        assert out["token_logprobs"].shape == (2, L) and out["watch_logprobs"].shape == (2, L, 3)
        assert out["token_logprobs"].dtype == out["watch_logprobs"].dtype == torch.float32
        assert bool((out["token_logprobs"][:, 0] < 0).all()) and bool((out["watch_logprobs"][:, 0] < 0).all())
        assert model.generate(samples, output_scores=True, **kw)["watch_logprobs"].shape == (2, L, 0)
        # the stream: one-sample batches, so both paths encode and prefill the sample alone -- the same bits
        ones = [{k: (v[i:i + 1] if torch.is_tensor(v) else [v[i]]) for k, v in samples.items()} for i in range(2)]
        outs = list(model.generate_stream(iter(ones), slots=2, output_scores=True, watch_ids=[3, 5, 7], **kw))
        assert [o["index"] for o in outs] == [0, 1]
        for o, one in zip(outs, ones):
            ref = model.generate(one, output_scores=True, watch_ids=[3, 5, 7], **kw)
            n = o["token_ids"].shape[0]
            assert torch.equal(o["token_ids"], ref["token_ids"][0, :n])
            assert o["token_logprobs"].shape == (n,) and o["watch_logprobs"].shape == (n, 3)
            assert torch.equal(o["token_logprobs"], ref["token_logprobs"][0, :n])
            assert torch.equal(o["watch_logprobs"], ref["watch_logprobs"][0, :n])
        assert set(next(iter(model.generate_stream(iter(ones), slots=2, **kw)))) == {"index", "token_ids", "ve_anomaly_map"}
        with pytest.raises(NotImplementedError, match="output_scores"):
            model.generate(samples, output_scores=True, num_beams=2, **kw)
        with pytest.raises(NotImplementedError):
            model.generate_stream(iter(ones), slots=2, output_scores=True, num_beams=2, **kw)
        with pytest.raises(ValueError, match="watch_ids"):
            model.generate(samples, output_scores=True, watch_ids=list(range(9)), **kw)
    finally:
        model.train()


@pytest.mark.parametrize("slots", [0, 2])
def test_eval_entry_point_writes_the_llm_anomaly_score(fx, tmp_path, monkeypatch, slots):
    import eval_aqa
    seen, watch = [], []
    gen, stream = MyriadHIP.generate, MyriadHIP.generate_stream

    def spy_generate(self, samples, **kw):
        out = gen(self, samples, **kw)
        watch.append(kw["watch_ids"])
        seen.extend(out["watch_logprobs"][:, 0].clone())
        return out

    def spy_stream(self, batches, **kw):
        watch.append(kw["watch_ids"])
        for out in stream(self, batches, **kw):
            seen.append(out["watch_logprobs"][0].clone())
            yield out

    monkeypatch.setattr(MyriadHIP, "generate", spy_generate)
    monkeypatch.setattr(MyriadHIP, "generate_stream", spy_stream)
    path, records = eval_aqa.main(["--cfg-path", fx["eval_yaml"], "--dataset", "synthetic", "--bs", "2", "--limit", "2", "--slots",
                                   str(slots), "--llm-score", "--out", str(tmp_path / "res.jsonl")])
    rows = [json.loads(ln) for ln in open(path)]
    assert len(rows) == len(records) == len(seen) == 4
    assert set(rows[0]) == {"image_id", "image_path", "is_anomaly", "error", "output", "anomaly_score", "llm_anomaly_score"}
    for r, lp in zip(rows, seen):
        assert lp.shape == (2,)
        p_yes, p_no = (float(torch.exp(v.double())) for v in lp)
        want = p_yes / (p_yes + p_no)
        assert 0.0 <= float(r["llm_anomaly_score"]) <= 1.0
        assert abs(float(r["llm_anomaly_score"]) - want) <= 0.5e-4 + 1e-9, (r, want)     # str(round(x, 4))
    assert len({tuple(w) for w in watch}) == 1 and len(watch[0]) == 2 and watch[0][0] != watch[0][1]


def test_the_watch_ids_are_the_training_labels_first_tokens(model):
    import eval_aqa
    tok = model.llama_tokenizer
    yes, no = eval_aqa.llm_watch_ids(tok)
    assert yes == tok(D.ABNORMAL_DESCRIBE, add_special_tokens=False).input_ids[0]
    assert no == tok(D.NORMAL_DESCRIBE, add_special_tokens=False).input_ids[0] and yes != no
