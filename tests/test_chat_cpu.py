"""Host side of the multi-turn chat (myriad_amd/chat.py, LlamaHIP's DecodeSession): the reference's prompt format against a
fixture written with the reference's own Conversation (tools/make_golden_chat.py), the longest-common-prefix rule over position
keys, the session's invalidation rules and key bookkeeping (on a stand-in model: no kernel runs), the truncation window and the
answer's post-processing."""
import json
import os

import pytest
import torch

from myriad_amd import chat as C
from myriad_amd.llama import DecodeSession, common_prefix, split_kv_rule

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chat_prompts.json")


def _styles():
    return {"single": C.CONV_VISION,
            "two": C.Conversation(system="A chat.", roles=("USER", "ASSISTANT"), messages=[], offset=0,
                                  sep_style=C.SeparatorStyle.TWO, sep=" ", sep2="</s>")}


@pytest.mark.parametrize("case", json.load(open(GOLDEN))["cases"], ids=lambda c: c["style"] + "-" + c["name"])
def test_prompts_match_the_reference_conversation(case):
    base = _styles()[case["style"]]
    conv = base.copy()
    prompts = []
    for st in case["steps"]:
        if st[0] == "img":
            conv.append_message(conv.roles[0], "<Img><ImageHere></Img>")
        elif st[0] == "ask":
            C.Chat.ask(None, st[1], conv)
        else:
            conv.append_message(conv.roles[1], None)
            prompts.append(conv.get_prompt())
            conv.messages[-1][1] = st[1]
        prompts.append(conv.get_prompt())
    assert prompts == case["prompts"]
    assert [list(m) for m in conv.messages] == case["messages"]
    assert conv.to_gradio_chatbot() == case["gradio"]
    d = {k: (list(v) if isinstance(v, tuple) else v) for k, v in conv.dict().items()}
    assert d == case["dict"]
    assert (conv.copy().dict() == conv.dict()) == case["copy_equal"]
    assert base.messages == []                                   # copies never share the template's history


def test_stop_words_are_the_references():
    assert [list(s) for s in C.STOP_WORDS] == json.load(open(GOLDEN))["stop_words"]
    assert [s.tolist() for s in C.Chat(None).stopping_criteria[0].stops] == [[835], [2277, 29937]]


def test_common_prefix_over_position_keys():
    t = lambda ids: [("t", i) for i in ids]
    img = lambda tag, n: [("i", tag, j) for j in range(n)]
    ctx1 = t([1, 5, 6]) + img("a", 4) + t([7, 8, 9])
    cached = ctx1 + t([40, 41, 42])                               # the generated ids the token step fed back
    # the answer re-tokenizes differently from the generated ids: reuse stops at the first differing id
    ctx2 = ctx1 + t([40, 43, 44]) + t([9, 9])
    assert common_prefix(ctx2, cached) == len(ctx1) + 1
    # an image inserted mid-history: nothing past the insertion point is reused
    ctx3 = t([1, 5, 6]) + img("b", 4) + img("a", 4) + t([7, 8, 9])
    assert common_prefix(ctx3, cached) == 3
    # the same image rows re-encoded to other values (another digest): not reused either
    assert common_prefix(t([1, 5, 6]) + img("a2", 4), cached) == 3
    assert common_prefix(ctx1, cached) == len(ctx1) and common_prefix([], cached) == 0


def test_truncation_window_and_postprocessing():
    assert C.truncation_begin(1500, 300, 2000) == 0
    assert C.truncation_begin(1700, 300, 2000) == 0
    assert C.truncation_begin(1701, 300, 2000) == 1
    assert C.truncation_begin(2500, 300, 2000) == 800
    assert C.postprocess_tokens([0, 1, 5, 6]) == [5, 6]
    assert C.postprocess_tokens([1, 0, 5]) == [0, 5]             # <s> then <unk>: only the <s> goes (the reference's order)
    assert C.postprocess_tokens([0, 0, 5]) == [0, 5]
    assert C.postprocess_tokens([7, 1]) == [7, 1] and C.postprocess_tokens([]) == []
    assert C.postprocess_text("There is a crack.###Human: next") == "There is a crack."
    assert C.postprocess_text("  Assistant: yes, at the top ### no") == "yes, at the top"
    assert C.postprocess_text("a Assistant: b Assistant: c") == "c"


def test_split_kv_rule():
    assert split_kv_rule(1, 32, 1024) and split_kv_rule(7, 32, 4096)
    assert not split_kv_rule(1, 32, 1023)                        # short contexts: the single-workgroup kernel is faster
    assert not split_kv_rule(8, 32, 2048)                        # 256 (row, head) workgroups fill the CUs already


class _FakeLlama:
    """What DecodeSession reads of LlamaHIP, on the CPU; _greedy_core returns scripted ids once the session has set its turn up."""

    def __init__(self):
        self.H, self.D, self.V, self.layers, self.dev = 2, 8, 50, [None], torch.device("cpu")
        self._packed, self.decode_fused, self.lora = None, True, None
        self.cos = torch.zeros((4096, 4))
        self.script = []

    def _prepare_decode_weights(self, rows):
        return {}

    def _greedy_core(self, emb, ws, past, weight_stats, max_new_tokens=90, **kw):
        self.last_past = past
        ids = self.script.pop(0)
        self.last_generate_stats = dict(steps=ids.shape[1], graph_replays=0)
        return ids


def test_session_reuse_invalidation_and_key_bookkeeping():
    L = _FakeLlama()
    s = DecodeSession(L, 100)
    t = lambda ids: [("t", i) for i in ids]
    emb = lambda n, B=1: torch.zeros((B, n, 8))
    k1 = t([1, 3, 4, 5])
    L.script.append(torch.tensor([[10, 11, 12]]))
    s.generate(emb(4), [k1], weights_version=0, max_new_tokens=5, eos_id=2)
    assert s.last_stats["reused_tokens"] == 0 and s.last_stats["full_reprefill_reason"] == "empty cache"
    assert s.keys == [k1 + t([10, 11])]                          # the last pick (12) was never fed back: no KV
    k2 = k1 + t([10, 11, 12, 6, 7])
    L.script.append(torch.tensor([[2, 2]]))
    s.generate(emb(len(k2)), [k2], weights_version=0, max_new_tokens=5, eos_id=2)
    assert s.last_stats["reused_tokens"] == 6 and s.last_stats["prefilled_tokens"] == 3
    assert s.last_stats["full_reprefill_reason"] is None and s.last_stats["split_kv"] is False
    # the whole context cached already: the last position is prefilled again (it gives the first logits)
    L.script.append(torch.tensor([[9]]))
    s.generate(emb(len(k2)), [k2], weights_version=0, max_new_tokens=5, eos_id=2)
    assert L.last_past == len(k2) - 1
    # weights changed, window moved, batch size changed, capacity exceeded: full prefill with a reason
    for kw, B, reason in ((dict(weights_version=1), 1, "weights changed"), (dict(weights_version=1, reset_reason="window"), 1, "window"),
                          (dict(weights_version=1), 2, "batch size")):
        L.script.append(torch.tensor([[9]] * B))
        s.generate(emb(len(k2), B), [k2] * B, max_new_tokens=5, eos_id=2, **kw)
        assert s.last_stats["reused_tokens"] == 0 and s.last_stats["full_reprefill_reason"] == reason
    L.script.append(torch.tensor([[9], [9]]))
    s.generate(emb(len(k2), 2), [k2] * 2, weights_version=1, max_new_tokens=200, eos_id=2)
    assert s.last_stats["full_reprefill_reason"] == "capacity" and s.bufs["T"] == 256
    # a row that finished early fed ids the host does not know: its keys past its EOS match nothing
    L.script.append(torch.tensor([[5, 6, 7, 8], [5, 2, 2, 2]]))
    s.generate(emb(len(k2), 2), [k2] * 2, weights_version=1, max_new_tokens=5, eos_id=2)
    assert s.keys[0] == k2 + t([5, 6, 7]) and s.keys[1] == k2 + t([5, 2]) + [("x",)]
    with pytest.raises(ValueError):                              # past the rotary table
        s.generate(emb(4000), [t([0] * 4000)], weights_version=1, max_new_tokens=200, eos_id=2)
