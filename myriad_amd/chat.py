"""Multi-turn chat about images: the reference's `minigpt4/conversation/conversation.py` (`SeparatorStyle`, `Conversation`,
`CONV_VISION`, `StoppingCriteriaSub`, `Chat` with `upload_img` / `ask` / `answer`) on the HIP decode path, with the KV cache kept
across turns.

Kept from the reference: the prompt format (`Conversation.get_prompt`), `ask` merging a question into a trailing image message
(conversation.py:137-142), the context built as `get_context_emb` builds it (the prompt split on `<ImageHere>`, each segment
tokenized, BOS on the first segment only, image embeddings in between), the stop words (835; 2277 29937: '###' tokenizes two
ways), the truncation window `begin_idx = max(0, len + max_new_tokens - max_length)`, and the answer's post-processing (a leading
0 / 1 token stripped, the text cut at '###' and after the last 'Assistant:').

Changed, because the reference's `Chat` does not match its own model's signatures (`prepare_sample(..., do_one_class=...)`,
`encode_img(image, maps)` do not exist with those arguments): `upload_img` maps onto this project's model calls -- the anomaly maps
come from `extras` or the attached vision expert through `MyriadHIP._maps_for`, as `generate()` gets them, and the image tokens
from `encode_img(image, maps, stage=1)` (MiniGPT-4 arch: the image alone, stage 0).  Path and PIL inputs go through the GPU image
front-end (Resize(224, bicubic) + CenterCrop(224) + CLIP normalisation, what the reference's transform + processor do) unless a
`vis_processor` is given.  `answer` also takes `do_sample` and `generator` (the reference always samples), and returns
`(text, token_ids)` like the reference.

Reuse.  Each `Chat` owns a `myriad_amd.decode.DecodeSession`: turn n prefills only the part of the context past the longest common prefix
with what the cache holds (positions named by token ids and (image, row) keys), then decodes on the session's own buffers and
captured graph.  `Chat.last_stats` reports what a turn reused.  The session uses the split-KV decode attention kernel where it is
measured faster (decode_host.split_kv_rule).  `num_beams > 1` runs the model's beam search (LlamaHIP.beam_generate) on the full context
without reuse (deterministic: `do_sample` does not apply to it), and leaves the session's cache as it was.

Several conversations at once.  `ChatPool` serves up to `slots` conversations on the decode slots (decode.SlotDecoder.run_turns):
one captured token step for all of them, each conversation's KV cache kept in its own slot across turns, a turn's new rows
prefilled on top of the reused prefix -- several conversations per pass over the weights.  `answer_many` does per conversation
what `Chat.answer` does; both classes share the conversation side (`_ChatBase`).
"""
from __future__ import annotations

import dataclasses
import hashlib
import warnings
from enum import Enum, auto
from typing import Any, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .decode import DecodeSession
from .myriad import StoppingCriteriaSub

__all__ = ["SeparatorStyle", "Conversation", "CONV_VISION", "StoppingCriteriaSub", "Chat", "ChatPool", "truncation_begin",
           "postprocess_tokens", "postprocess_text"]

STOP_WORDS = ((835,), (2277, 29937))          # '###' can be encoded in two different ways (conversation.py:130-131)


class SeparatorStyle(Enum):
    """Different separator style."""
    SINGLE = auto()
    TWO = auto()


@dataclasses.dataclass
class Conversation:
    """A class that keeps all conversation history."""
    system: str
    roles: List[str]
    messages: List[List[str]]
    offset: int
    sep_style: SeparatorStyle = SeparatorStyle.SINGLE
    sep: str = "###"
    sep2: str = None

    skip_next: bool = False
    conv_id: Any = None

    def get_prompt(self):
        if self.sep_style == SeparatorStyle.SINGLE:
            ret = self.system + self.sep
            for role, message in self.messages:
                if message:
                    ret += role + ": " + message + self.sep
                else:
                    ret += role + ":"
            return ret
        if self.sep_style == SeparatorStyle.TWO:
            seps = [self.sep, self.sep2]
            ret = self.system + seps[0]
            for i, (role, message) in enumerate(self.messages):
                if message:
                    ret += role + ": " + message + seps[i % 2]
                else:
                    ret += role + ":"
            return ret
        raise ValueError(f"Invalid style: {self.sep_style}")

    def append_message(self, role, message):
        self.messages.append([role, message])

    def to_gradio_chatbot(self):
        ret = []
        for i, (role, msg) in enumerate(self.messages[self.offset:]):
            if i % 2 == 0:
                ret.append([msg, None])
            else:
                ret[-1][-1] = msg
        return ret

    def copy(self):
        return Conversation(system=self.system, roles=self.roles, messages=[[x, y] for x, y in self.messages], offset=self.offset,
                            sep_style=self.sep_style, sep=self.sep, sep2=self.sep2, conv_id=self.conv_id)

    def dict(self):
        return {"system": self.system, "roles": self.roles, "messages": self.messages, "offset": self.offset, "sep": self.sep,
                "sep2": self.sep2, "conv_id": self.conv_id}


CONV_VISION = Conversation(
    system="Give the following image: <Img>ImageContent</Img>. "
           "You will be able to see the image once I provide it to you. Please answer my questions.",
    roles=("Human", "Assistant"),
    messages=[],
    offset=2,
    sep_style=SeparatorStyle.SINGLE,
    sep="###",
)


def ask(text: str, conv: Conversation) -> None:
    """`Chat.ask`: a question right after an image message joins that message (conversation.py:137-142)."""
    if len(conv.messages) > 0 and conv.messages[-1][0] == conv.roles[0] and conv.messages[-1][1][-6:] == "</Img>":
        conv.messages[-1][1] = " ".join([conv.messages[-1][1], text])
    else:
        conv.append_message(conv.roles[0], text)


def truncation_begin(context_len: int, max_new_tokens: int, max_length: int) -> int:
    """The reference's window (conversation.py:150-156): the first context position the model still sees."""
    return max(0, context_len + max_new_tokens - max_length)


def postprocess_tokens(ids: Sequence[int]) -> List[int]:
    """A leading <unk> (0), then a leading <s> (1), is removed (conversation.py:170-173)."""
    out = [int(t) for t in ids]
    if out and out[0] == 0:
        out = out[1:]
    if out and out[0] == 1:
        out = out[1:]
    return out


def postprocess_text(text: str) -> str:
    """The decoded answer cut at the stop sign and after the last 'Assistant:' (conversation.py:175-176)."""
    return text.split("###")[0].split("Assistant:")[-1].strip()


class _ChatBase:
    """The conversation side shared by Chat and ChatPool: images in, the context's embeddings and position keys out."""

    def __init__(self, model, vis_processor=None, device="cuda:0"):
        self.device = torch.device(device)
        self.model = model
        self.vis_processor = vis_processor
        self.stopping_criteria = [StoppingCriteriaSub(stops=[torch.tensor(list(s)) for s in STOP_WORDS])]
        self._frontend = None
        self.last_stats = {}
        self.last_token_ids = None
        self._digests = {}

    # ------------------------------------------------------------------ conversation
    def ask(self, text, conv):
        ask(text, conv)

    def _image_tensor(self, image) -> torch.Tensor:
        if isinstance(image, torch.Tensor):
            if image.dim() == 3:
                image = image.unsqueeze(0)
            return image.to(self.device, torch.float32)
        from PIL import Image
        raw = Image.open(image).convert("RGB") if isinstance(image, str) else image
        if not isinstance(raw, Image.Image):
            raise TypeError(f"upload_img: a tensor, a path or a PIL image, got {type(image).__name__}")
        if self.vis_processor is not None:
            return self.vis_processor(raw).unsqueeze(0).to(self.device, torch.float32)
        if self._frontend is None:
            from .image_frontend import ImageFrontEndHIP
            self._frontend = ImageFrontEndHIP(self.device, size=224, mode="train")   # Resize(224) + CenterCrop(224) + normalise
        return self._frontend([np.asarray(raw.convert("RGB"), dtype=np.uint8)])

    @torch.no_grad()
    def upload_img(self, image, conv, img_list, **extras):
        """Encode one image and add it to the conversation.  `extras`: `anomaly_maps` / `oneshot_anomaly_maps` [1, 1, 224, 224], or
        `expert_text_feats` + `ref_images` for an attached vision expert (Myriad arch; the key generate() reads: oneshot maps when
        k_shot > 0).  Returns ("Received.", the anomaly map used or None)."""
        m = self.model
        m.finish_update()
        image = self._image_tensor(image)
        maps = None
        if m.arch == "myriad":
            key = "oneshot_anomaly_maps" if m.k_shot > 0 else "anomaly_maps"
            maps = m._maps_for(dict(extras), key, image)
            parts = m.encode_img(image, maps, 1, False)
        else:
            parts = m.encode_img(image, None, 0, False)
        emb = torch.cat([p.to(torch.float32) for p in parts], 1).contiguous()      # [1, n_img, D]: the rows _assemble places
        img_list.append(emb)
        conv.append_message(conv.roles[0], "<Img><ImageHere></Img>")
        return "Received.", maps

    def _image_key(self, emb: torch.Tensor):
        """A digest of the embedding's bytes: a re-encoded or replaced image never matches the rows cached for another one.  Kept
        per tensor (holding it, so its id is not reused) and version."""
        hit = self._digests.get(id(emb))
        if hit is not None and hit[0] is emb and hit[1] == emb._version:
            return hit[2]
        dig = hashlib.blake2b(emb.detach().float().cpu().numpy().tobytes(), digest_size=16).hexdigest()
        if len(self._digests) > 64:
            self._digests.clear()
        self._digests[id(emb)] = (emb, emb._version, dig)
        return dig

    def context_tokens(self, conv, img_list):
        """`get_context_emb`'s layout without the embeddings: a list of segments, token-id lists and image tensors in order."""
        tok = self.model.llama_tokenizer
        segs = conv.get_prompt().split("<ImageHere>")
        assert len(segs) == len(img_list) + 1, "Unmatched numbers of image placeholders and images."
        out = []
        for i, seg in enumerate(segs):
            out.append([int(t) for t in tok(seg, return_tensors="pt", add_special_tokens=i == 0).input_ids[0].tolist()])
            if i < len(img_list):
                out.append(img_list[i])
        return out

    def get_context_emb(self, conv, img_list):
        """Returns (embeddings [1, S, D] f32 on the device, one key per position)."""
        parts = self.context_tokens(conv, img_list)
        llama = self.model.llama
        S = sum(len(p) if isinstance(p, list) else p.shape[1] for p in parts)
        emb = torch.empty((1, S, llama.D), dtype=torch.float32, device=self.device)
        keys, ids, rows, col = [], [], [], 0
        for p in parts:
            if isinstance(p, list):
                ids += p
                rows += range(col, col + len(p))
                keys += [("t", t) for t in p]
                col += len(p)
            else:
                n = p.shape[1]
                ops.copy3d(p.to(self.device, torch.float32), emb[:, col:col + n])
                dig = self._image_key(p)
                keys += [("i", dig, j) for j in range(n)]
                col += n
        if ids:
            llama.embed_tokens_into(ops.h2d(torch.tensor(ids, dtype=torch.long), self.device), emb.view(S, llama.D),
                                    ops.h2d(torch.tensor(rows, dtype=torch.int32), self.device))
        return emb, keys

    def _turn_context(self, conv, img_list, max_new_tokens, max_length):
        """The start of an assistant turn (conversation.py:144-156): the assistant role appended, the context's embeddings and
        keys cut to the reference's window.  Returns (embs [1, S, D], keys [S], begin)."""
        conv.append_message(conv.roles[1], None)
        embs, keys = self.get_context_emb(conv, img_list)
        begin = truncation_begin(embs.shape[1], max_new_tokens, max_length)
        if begin > 0:
            warnings.warn("The number of tokens in current conversation exceeds the max length. "
                          "The model will not see the contexts outside the range.", RuntimeWarning, stacklevel=3)
        return embs[:, begin:].contiguous(), keys[begin:], begin

    def _finish_turn(self, conv, ids):
        """The end of one (conversation.py:170-177): post-processing, the answer written into the conversation."""
        out = postprocess_tokens(ids)
        text = postprocess_text(self.model.llama_tokenizer.decode(out, add_special_tokens=False))
        conv.messages[-1][1] = text
        return text, np.asarray(out, dtype=np.int64)


class Chat(_ChatBase):
    def __init__(self, model, vis_processor=None, device="cuda:0"):
        super().__init__(model, vis_processor, device)
        self.session: Optional[DecodeSession] = None

    # ------------------------------------------------------------------ answer
    @torch.no_grad()
    def answer(self, conv, img_list, max_new_tokens=300, num_beams=1, min_length=1, top_p=0.9, repetition_penalty=1.0,
               length_penalty=1, temperature=1.0, max_length=2000, do_sample=True, generator=None, draft=None, draft_k=4):
        """One assistant turn (conversation.py:144-178).  The context is truncated to the reference's window; the KV cache of the
        earlier turns is reused up to the first position whose token / image row differs.  `repetition_penalty` != 1 needs the
        device sampling switch, as in generate().  num_beams > 1: beam search on the full context, no reuse; with the beam sampling
        switch (MYRIAD_BEAM_SAMPLING=1 or model.llama.beam_sampling = True) it is the reference's own call -- beam-search
        multinomial sampling with do_sample, top_p, temperature, top_k = 50, repetition_penalty and generator
        (LlamaHIP.beam_generate) -- and last_stats gains num_beams, beam_sampled_steps and beam_host_steps; without it the
        beams are deterministic and a penalty is refused, as before.  `draft` / `draft_k`: draft-and-verify decoding of the turn
        (LlamaHIP.greedy_generate; the same ids in fewer token steps when the drafter guesses well), refused with beams and --
        unless model.llama.draft_sampling (MYRIAD_DRAFT_SAMPLING=1) is on -- with device sampling and `repetition_penalty` != 1;
        a turn on the split-KV view decodes with plain steps and last_stats["draft_off"] says "split_kv", unless
        model.llama.draft_split (MYRIAD_DRAFT_SPLIT=1) is on: then it drafts there too (mh_attn_decode_rope_split_draft)."""
        m = self.model
        m.finish_update()
        llama = m.llama
        llama.decode_lora_version = m.store.version                 # decode_merge_lora re-merges only when the LoRA weights moved
        rep = 1.0 if repetition_penalty is None else float(repetition_penalty)
        beam_sampling = bool(llama.beam_sampling and int(num_beams) > 1)
        if rep != 1.0 and not llama.device_sampling and not beam_sampling:
            raise NotImplementedError(f"answer(repetition_penalty={rep}) needs the device sampling switch "
                                      "(MYRIAD_DEVICE_SAMPLING=1 or model.llama.device_sampling = True)")
        embs, keys, begin = self._turn_context(conv, img_list, max_new_tokens, max_length)
        S = embs.shape[1]
        if int(num_beams) > 1:
            if draft is not None:
                raise NotImplementedError(f"answer(num_beams={num_beams}, draft=...): draft decoding is greedy decoding")
            if rep != 1.0 and not beam_sampling:
                raise NotImplementedError(f"answer(num_beams={num_beams}, repetition_penalty={rep}) is not implemented")
            sample_kw = {}
            if beam_sampling:
                sample_kw = dict(do_sample=bool(do_sample), top_p=float(top_p), temperature=float(temperature), top_k=50,
                                 repetition_penalty=rep, generator=generator)
            ids = llama.beam_generate(embs, int(num_beams), max_new_tokens=max_new_tokens, stop_ids=STOP_WORDS, eos_id=2,
                                      min_length=min_length, length_penalty=float(length_penalty), **sample_kw)
            st = llama.last_generate_stats
            self.last_stats = dict(context_tokens=S, reused_tokens=0, prefilled_tokens=S, steps=st["steps"],
                                   graph_captures=0 if self.session is None else self.session.graph_captures,
                                   graph_replays=st["graph_replays"], split_kv=False, full_reprefill_reason="num_beams")
            if beam_sampling:
                self.last_stats.update(num_beams=st["num_beams"], beam_sampled_steps=st.get("beam_sampled_steps", 0),
                                       beam_host_steps=st.get("beam_host_steps", 0))
        else:
            if self.session is None:
                self.session = DecodeSession(llama, max_length + max_new_tokens + 2 + (0 if draft is None else int(draft_k)))
            ids = self.session.generate(embs, [keys], weights_version=m.store.version,
                                        reset_reason="window" if begin > 0 else None, max_new_tokens=max_new_tokens,
                                        stop_ids=STOP_WORDS, eos_id=2, min_length=min_length, do_sample=bool(do_sample),
                                        top_p=float(top_p), temperature=float(temperature), generator=generator, top_k=50,
                                        repetition_penalty=rep, **({} if draft is None else dict(draft=draft, draft_k=draft_k)))
            self.last_stats = dict(self.session.last_stats)
        self.last_token_ids = ids                                    # [B, L] as decoded, before the post-processing
        return self._finish_turn(conv, ids[0].tolist())


class ChatPool(_ChatBase):
    """Several conversations at once on the decode slots: `slots` conversations share ONE captured token step (each weight is
    streamed once per step for all of them) and each keeps its KV cache in its own slot across turns, as a `Chat` keeps its
    session's.  The session id is the `Conversation` object; the pool holds it until `close(conv)` frees its slot, and a
    conversation beyond `slots` open ones is a ValueError.  `upload_img` / `ask` are Chat's.  No beam search (decode slots have
    none).  `split_kv` picks the step's attention kernel (SlotDecoder's argument): False, the default, is the single-workgroup
    rows kernel at every length; True the split-KV rows kernel, which a few long conversations want (a solo Chat switches to
    split-KV past ~1,024 keys); None chooses per answer_many call by decode_host.split_kv_rows_rule.  `last_stats[i]["split_kv"]`
    reports the choice."""

    def __init__(self, model, slots=8, capacity=2000 + 300 + 2, split_kv=False, device=None, vis_processor=None):
        super().__init__(model, vis_processor, model.llama.dev if device is None else device)
        self.decoder = model.llama.slot_decoder(int(slots), int(capacity), split_kv=split_kv)
        self.last_stats = []

    def close(self, conv) -> None:
        self.decoder.close(conv)

    @torch.no_grad()
    def answer_many(self, items, max_new_tokens=300, num_beams=1, min_length=1, top_p=0.9, repetition_penalty=1.0, temperature=1.0,
                    max_length=2000, do_sample=True, generator=None, seeds=None, prefill_batch=8, draft=None, draft_k=4):
        """One assistant turn for each (conv, img_list) of `items`, Chat.answer's per conversation (the assistant role, the
        context and its truncation window -- a moved window resets that session, reason "window" --, the post-processing, the
        answer written into conv.messages) through SlotDecoder.run_turns.  Returns [(text, ids)] in the items' order;
        `last_stats` is a list of per-conversation dicts with Chat.last_stats' keys where they apply.  `seeds`: with device
        sampling, the i-th item's random stream (else drawn from `generator`), so an answer does not depend on its neighbours.
        `draft` / `draft_k`: draft-and-verify decoding of the call's turns (SlotDecoder.run_turns(draft=), behind
        model.llama.slot_draft and model.llama.draft_split -- NotImplementedError without them): the same texts in fewer token
        steps where the drafter guesses well, and every `last_stats[i]` gains the call's draft counters (draft_k, draft_off,
        verify_steps, plain_steps, draft_proposed, draft_accepted)."""
        m = self.model
        if int(num_beams) > 1:
            raise NotImplementedError(f"answer_many(num_beams={num_beams}): decode slots have no beam search; use Chat.answer")
        m.finish_update()
        llama = m.llama
        llama.decode_lora_version = m.store.version
        rep = 1.0 if repetition_penalty is None else float(repetition_penalty)
        if rep != 1.0 and not llama.device_sampling:
            raise NotImplementedError(f"answer_many(repetition_penalty={rep}) needs the device sampling switch "
                                      "(MYRIAD_DEVICE_SAMPLING=1 or model.llama.device_sampling = True)")
        items = list(items)
        if len({id(c) for c, _ in items}) != len(items):             # refused before any conversation is touched
            raise ValueError("answer_many: at most one turn per conversation in one call")
        new = [c for c, _ in items if c not in self.decoder.sessions]
        if len(self.decoder.sessions) + len(new) > self.decoder.slots:
            raise ValueError(f"{len(self.decoder.sessions)} open conversations + {len(new)} new ones do not fit "
                             f"{self.decoder.slots} slots: close() some")
        turns = []
        for conv, img_list in items:
            embs, keys, begin = self._turn_context(conv, img_list, max_new_tokens, max_length)
            turns.append((conv, embs[0], keys, "window" if begin > 0 else None))
        kw = dict(seeds=seeds) if seeds is not None else {}
        if draft is not None:
            kw.update(draft=draft, draft_k=draft_k)
        got = list(self.decoder.run_turns(turns, weights_version=m.store.version, max_new_tokens=max_new_tokens,
                                          stop_ids=STOP_WORDS, eos_id=2, min_length=min_length, do_sample=bool(do_sample),
                                          top_p=float(top_p), temperature=float(temperature), generator=generator, top_k=50,
                                          repetition_penalty=rep, prefill_batch=int(prefill_batch), ordered=True, **kw))
        st = self.decoder.last_stats
        shared = {k: st[k] for k in ("steps", "graph_captures", "graph_replays")}
        if "draft_k" in st:                                          # a draft call: its counters, the same for every conversation
            shared.update({k: st[k] for k in ("draft_k", "draft_off", "verify_steps", "plain_steps", "draft_proposed", "draft_accepted")})
        self.last_stats = [dict(t, split_kv=st["split_kv"], **shared) for t in st["turns"]]
        self.last_token_ids = [ids for _, ids, _ in got]
        return [self._finish_turn(conv, ids.tolist()) for (conv, _), (_, ids, _) in zip(items, got)]
