"""The chat call's generate() arguments (conversation.py:144-168: do_sample=True, top_p=0.9, temperature=1.0, HF's top_k=50,
repetition_penalty) on the model built from the reference's on-disk files (the fixtures of tests/test_entrypoints_gpu.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd.myriad import StoppingCriteriaSub  # noqa: E402
from tests.test_entrypoints_gpu import DEV, _batch, fx, model  # noqa: E402,F401


def test_generate_takes_the_chat_arguments_with_device_sampling(model):
    tok = model.llama_tokenizer
    samples = _batch(2, train=False, seed=5)
    hashes = tok("###", add_special_tokens=False).input_ids
    kw = {"max_new_tokens": 12, "stopping_criteria": [StoppingCriteriaSub(stops=[torch.tensor(hashes).to(DEV)])], "do_sample": True,
          "top_p": 0.9, "temperature": 1.0, "min_length": 1}
    model.eval()
    prev = model.llama.device_sampling
    try:
        model.llama.device_sampling = False                 # the switch off: the earlier contract, a penalty is refused
        with pytest.raises(NotImplementedError):
            model.generate(samples, **dict(kw, repetition_penalty=1.3))
        model.llama.device_sampling = True
        a = model.generate(samples, generator=torch.Generator().manual_seed(3), **kw)["token_ids"]
        st = dict(model.last_generate_stats)
        assert a.shape[0] == 2 and st["steps"] == a.shape[1]
        assert st["device_sampled_rows"] > 0 and st["host_sampled_rows"] == 0
        b = model.generate(samples, generator=torch.Generator().manual_seed(3), **kw)["token_ids"]
        assert torch.equal(a, b)                            # reproducible through the generator's seed
        pen = model.generate(samples, generator=torch.Generator().manual_seed(3), **dict(kw, repetition_penalty=1.3))["token_ids"]
        assert pen.shape[0] == 2 and model.last_generate_stats["steps"] == pen.shape[1]
        g = model.generate(samples, **dict(kw, do_sample=False, repetition_penalty=1.3))["token_ids"]   # greedy with the penalty
        assert g.shape[0] == 2
        for bad in ({"num_beams": 2}, {"length_penalty": 2.0}, {"num_return_sequences": 2}):
            with pytest.raises(NotImplementedError):
                model.generate(samples, **dict(kw, **bad))
        for bad in ({"temperature": 0.0}, {"repetition_penalty": 0.0}):
            with pytest.raises(ValueError):
                model.generate(samples, **dict(kw, **bad))
    finally:
        model.llama.device_sampling = prev
        model.train()
