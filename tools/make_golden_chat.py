#!/usr/bin/env python3
"""Writes tests/golden/chat_prompts.json with the reference's own `Conversation` / `Chat.ask`
(minigpt4/conversation/conversation.py): multi-turn, multi-image histories, the prompt after every step, and the final
`to_gradio_chatbot()` / `dict()`.  Only this generator reads the reference; the tests read the JSON.

python tools/make_golden_chat.py --reference /path/to/reference/checkout [--out tests/golden/chat_prompts.json]

The module is loaded from its file with stand-ins for the imports it does not use here (the package registry, torchvision's
transforms), so no other part of the reference package is imported."""
import argparse
import importlib.util
import json
import os
import sys
import types

ap = argparse.ArgumentParser()
ap.add_argument("--reference", required=True, help="root of the reference checkout (holds minigpt4/)")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                              "chat_prompts.json"))
a = ap.parse_args()


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


import transformers  # noqa: E402,F401  (before the torchvision stand-in: transformers probes for the real package)
from transformers import AutoModelForCausalLM, AutoTokenizer, LlamaTokenizer, StoppingCriteria  # noqa: E402,F401

stub("minigpt4")
stub("minigpt4.common")
stub("minigpt4.common.registry", registry=object())
tv = stub("torchvision")
tv.transforms = stub("torchvision.transforms", transforms=types.SimpleNamespace(
    Compose=lambda *x, **k: None, Resize=lambda *x, **k: None, CenterCrop=lambda *x, **k: None,
    InterpolationMode=types.SimpleNamespace(BICUBIC=3)))
spec = importlib.util.spec_from_file_location("ref_conversation",
                                              os.path.join(a.reference, "minigpt4", "conversation", "conversation.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

IMG = "<Img><ImageHere></Img>"
# ("img",) = upload_img's message; ("ask", text) = Chat.ask; ("answer", text) = Chat.answer's two edits of the conversation
SCENARIOS = {
    "one_image_three_turns": [("img",), ("ask", "Is there a defect?"), ("answer", "Yes, there is a scratch."),
                              ("ask", "Where is it?"), ("answer", "At the upper left."), ("ask", "How large?"), ("answer", "")],
    "two_images_mid_history": [("img",), ("ask", "Is there a defect?"), ("answer", "No."), ("img",), ("img",),
                               ("ask", "And in these two?"), ("answer", "The second one has a crack.\nIt is small."),
                               ("ask", "Assistant: is that a trick?"), ("answer", "###")],
    "text_first_then_image": [("ask", "Hello"), ("answer", "Hi! Please upload an image."), ("img",), ("ask", "What is this?"),
                              ("answer", "A bottle ### with text after the stop")],
    "question_not_merged_after_answer": [("img",), ("answer", "Received it."), ("ask", "Now what?"), ("img",), ("ask", "Merged?")],
}
STYLES = {
    "single": ref.CONV_VISION,
    "two": ref.Conversation(system="A chat.", roles=("USER", "ASSISTANT"), messages=[], offset=0,
                            sep_style=ref.SeparatorStyle.TWO, sep=" ", sep2="</s>"),
}

out = {"stop_words": [[835], [2277, 29937]], "cases": []}
for style, base in STYLES.items():
    for name, steps in SCENARIOS.items():
        conv = base.copy()
        prompts = []
        for st in steps:
            if st[0] == "img":
                conv.append_message(conv.roles[0], IMG)
            elif st[0] == "ask":
                ref.Chat.ask(None, st[1], conv)
            else:
                conv.append_message(conv.roles[1], None)
                prompts.append(conv.get_prompt())               # what answer() feeds the model
                conv.messages[-1][1] = st[1]
            prompts.append(conv.get_prompt())
        cp = conv.copy()
        out["cases"].append(dict(style=style, name=name, steps=[list(s) for s in steps], prompts=prompts,
                                 messages=[list(m) for m in conv.messages], gradio=conv.to_gradio_chatbot(),
                                 dict={k: (list(v) if isinstance(v, tuple) else v) for k, v in conv.dict().items()},
                                 copy_equal=cp.dict() == conv.dict()))
with open(a.out, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
print("wrote", a.out, len(out["cases"]), "cases")
