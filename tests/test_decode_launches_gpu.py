"""The decode paths' launches and picks, pinned: every case below runs one decode path on a small model with myriad_amd._lib.load
replaced by a proxy that notes the name of every mh_* entry called, and compares the ordered name list and the generated ids with
tests/golden/decode_launches.json.  A change that means to leave the decode path's device work alone (moving its host code,
renaming, refolding a loop) passes this file unchanged.

The model is the peaked token-transition LLaMA of tests/golden_utils.decode_chain_weights() (two layers, D = 64): its picks do
not sit on ties.  MXFP4 needs K % 128 == 0, so that one case runs on the D = 128 model of tests/test_fp4_decode_gpu.py.  A step
that captures a graph makes its calls through Python once more and they are noted like eager ones; replays are not noted.

Re-recording (only for a change that MEANS to alter the launches or the picks; say so in its description): run

    MYRIAD_RECORD_DECODE_LAUNCHES=tests/golden/decode_launches.json python -m pytest tests/test_decode_launches_gpu.py

on the commit BEFORE the change to see that the file reproduces, then on the change: each case then rewrites its entry of the named
JSON file instead of comparing, and the diff of the JSON is the change of the launches.  The file holds a table of entry names and,
per case, the ids and the calls as indices into the table with repeats folded: [n, [...]] is n times the inner list."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from myriad_amd.llama import DecodeSession, LlamaHIP  # noqa: E402
from tests import chat_pool_case as C  # noqa: E402
from tests import golden_utils as gu  # noqa: E402

DEV = "cuda:0"
BF16 = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_launches.json")
RECORD = os.environ.get("MYRIAD_RECORD_DECODE_LAUNCHES")                   # a path: record into it instead of comparing


# ------------------------------------------------------------------ the recording
def fold(seq):
    """Run-length fold of a list: a stretch that is n >= 2 copies of one block becomes [n, fold(block)]."""
    out, i = [], 0
    while i < len(seq):
        best_len, best_n = 1, 1
        for n_blk in range(1, min(96, (len(seq) - i) // 2) + 1):
            n = 1
            while seq[i + n * n_blk:i + (n + 1) * n_blk] == seq[i:i + n_blk]:
                n += 1
            if n > 1 and n * n_blk > best_len * best_n:
                best_len, best_n = n_blk, n
        if best_n > 1:
            out.append([best_n, fold(seq[i:i + best_len])])
            i += best_len * best_n
        else:
            out.append(seq[i])
            i += 1
    return out


def unfold(folded):
    out = []
    for item in folded:
        if isinstance(item, list):
            out.extend(unfold(item[1]) * item[0])
        else:
            out.append(item)
    return out


class _Noting:
    """The loaded library with every mh_* entry wrapped: the call's name is noted, then the call is made."""

    def __init__(self, lib, calls):
        self._lib, self._calls, self._wrapped = lib, calls, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("mh_"):
            return fn
        w = self._wrapped.get(name)
        if w is None:
            def w(*args, _fn=fn, _name=name):
                self._calls.append(_name)
                return _fn(*args)
            self._wrapped[name] = w
        return w


@pytest.fixture
def noted(monkeypatch):
    lib = _lib.load()
    ops.ensure_workspace(DEV)                                        # once per process: not a call of any case
    calls = []
    proxy = _Noting(lib, calls)
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    return calls


def _check(case, calls, ids):
    torch.cuda.synchronize()
    calls = list(calls)
    assert calls and all(c.startswith("mh_") for c in calls)
    if RECORD:
        doc = json.load(open(RECORD)) if os.path.exists(RECORD) else dict(names=[], cases={})
        names = doc["names"]
        for c in calls:
            if c not in names:
                names.append(c)
        doc["cases"][case] = dict(ids=ids, calls=fold([names.index(c) for c in calls]))
        with open(RECORD, "w") as f:
            f.write("{\n\"names\": " + json.dumps(names) + ",\n\"cases\": {\n"
                    + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in sorted(doc["cases"].items()))
                    + "\n}}\n")
        return
    doc = json.load(open(GOLDEN))
    want = doc["cases"][case]
    want_calls = [doc["names"][i] for i in unfold(want["calls"])]
    first = next((i for i, (a, b) in enumerate(zip(calls, want_calls)) if a != b), min(len(calls), len(want_calls)))
    assert calls == want_calls, (case, "first difference at call", first, "got", calls[first:first + 6], "recorded",
                                 want_calls[first:first + 6], "lengths", len(calls), len(want_calls))
    assert ids == want["ids"], (case, ids, want["ids"])


# ------------------------------------------------------------------ models and inputs
@pytest.fixture(scope="module")
def chain_sd():
    return gu.decode_chain_weights()


def _chain_model(sd):
    return LlamaHIP(sd, gu.DECODE_CHAIN["heads"], DEV, need_backward=False)


def _with_lora(lm, r=8, seed=77):
    """The q/v LoRA of tests/test_lora_merge_gpu.py's _lora_model: bf16-valued masters in a ParamStore."""
    from myriad_amd.lora import LoraQV, lora_param_specs
    from myriad_amd.myriad import ParamStore
    gen = torch.Generator().manual_seed(seed)
    st = ParamStore(lora_param_specs(len(lm.layers), lm.D, r), DEV)
    for name, ishape, _ in st.specs:
        st.p[name].copy_((torch.randn(ishape, generator=gen) * (0.05 if "lora_A" in name else 0.1)).to(BF16).float())
    lm.attach_lora(LoraQV(len(lm.layers), lm.D, r, 16.0, 0.0, st.p, st.g, DEV))
    return lm


CHAIN_ROWS = ["row0", "row1", "row2", "row3", "stop835"]
GREEDY_KW = dict(max_new_tokens=5, stop_ids=((835,), (2277, 29937)), eos_id=2, min_length=1, use_graph=False)


def _rows(n):
    return gu.decode_chain_inputs([CHAIN_ROWS[i % len(CHAIN_ROWS)] for i in range(n)]).to(DEV)


# ------------------------------------------------------------------ greedy_generate, eager
GREEDY = {
    "rows1": (1, {}, False), "rows3": (3, {}, False), "rows17": (17, {}, False),
    "rows1_unfused": (1, dict(decode_fused=False), False), "rows1_unpacked": (1, dict(pack_decode=False), False),
    "rows1_fp8": (1, dict(decode_fp8=True), False),
    "rows2_lora_bordered": (2, {}, True), "rows2_lora_merged": (2, dict(decode_merge_lora=True), True),
}


@pytest.mark.parametrize("case", sorted(GREEDY))
def test_greedy_generate(case, chain_sd, noted):
    rows, switches, lora = GREEDY[case]
    lm = _chain_model(chain_sd)
    for k, v in switches.items():
        assert hasattr(lm, k)
        setattr(lm, k, v)
    if lora:
        _with_lora(lm)
    x = _rows(rows)
    del noted[:]                                                     # building the model and the inputs is not the decode path
    ids = lm.greedy_generate(x, **GREEDY_KW)
    _check("greedy_" + case, noted, ids.tolist())


def test_greedy_generate_fp4(noted):
    from tests.test_fp4_decode_gpu import _tiny
    emb, sd, heads = _tiny()
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    lm.decode_fp4 = True
    x = emb[:1].to(DEV)
    del noted[:]
    ids = lm.greedy_generate(x, max_new_tokens=5, stop_ids=(), eos_id=-5, min_length=0, use_graph=False)
    _check("greedy_rows1_fp4", noted, ids.tolist())


def test_beam_generate(chain_sd, noted):
    lm = _chain_model(chain_sd)
    x = _rows(1)
    del noted[:]
    ids = lm.beam_generate(x, num_beams=2, max_new_tokens=5, stop_ids=((835,),), eos_id=2, min_length=1, use_graph=False)
    _check("beam2", noted, ids.tolist())


# ------------------------------------------------------------------ DecodeSession
@pytest.mark.parametrize("split", [False, True])
def test_decode_session_two_turns(split, chain_sd, noted):
    """The second turn's context is the first one's, the ids it generated and new rows: all but its new rows are reused."""
    lm = _chain_model(chain_sd)
    emb_w = chain_sd["llama_model.model.embed_tokens.weight"]
    sess = DecodeSession(lm, C.CAPACITY, split=split)
    kw = dict(max_new_tokens=C.MAX_NEW, stop_ids=C.STOPS, eos_id=C.EOS, min_length=1)
    ctx, keys = C.first_turn("a", emb_w)
    del noted[:]
    ids1 = sess.generate(ctx[None].to(DEV), [keys], weights_version=0, **kw)[0].tolist()
    ctx, keys = C.next_turn("a", 1, ctx, keys, ids1, emb_w[ids1].to(BF16).float(), emb_w)
    ids2 = sess.generate(ctx[None].to(DEV), [keys], weights_version=0, **kw)[0].tolist()
    assert sess.last_stats["reused_tokens"] > 0 and sess.last_stats["split_kv"] is split
    _check("session_split" if split else "session", noted, [ids1, ids2])


# ------------------------------------------------------------------ SlotDecoder.run
def _slot_requests(sd):
    """The seven requests of tests/test_decode_slots_gpu.py's ragged test; its stops are request 3's second token (835) and
    request 0's fifth (105)."""
    starts = ["row0", "row1", "row2", "row3", "stop835", "row1", "row3"]
    lengths = [5, 23, 9, 14, 7, 18, 11]
    g = torch.Generator().manual_seed(77)
    emb_w = sd["llama_model.model.embed_tokens.weight"]
    reqs = []
    for name, n in zip(starts, lengths):
        x = torch.randn(n, gu.DECODE_CHAIN["D"], generator=g) * 0.3
        x[-1] = emb_w[gu.DECODE_CHAINS[name][0]]
        reqs.append(x)
    return reqs


SLOT_KW = dict(max_new_tokens=12, stop_ids=((835,), (105,)), eos_id=2, min_length=1)
SAMPLED = dict(do_sample=True, temperature=0.8, top_p=0.9, top_k=50)
SLOTS = {                                                            # slots, decoder arguments, device_sampling, run arguments
    "plain": (3, {}, False, {}),
    "prefill_batch2": (3, {}, False, dict(prefill_batch=2)),
    "min_length2_rows_tail": (3, {}, True, dict(min_length=2)),
    "device_sampled_seeds": (3, {}, True, dict(SAMPLED, seeds=[11, 12, 13, 14, 15, 16, 17])),
    "split_kv": (3, dict(split_kv=True), False, {}),
    "plain_24_slots": (24, {}, False, {}),
}


@pytest.mark.parametrize("case", sorted(SLOTS))
def test_slot_decoder_run(case, chain_sd, noted):
    slots, dec_kw, device_sampling, run_kw = SLOTS[case]
    lm = _chain_model(chain_sd)
    lm.device_sampling = device_sampling
    reqs = _slot_requests(chain_sd)
    dec = lm.slot_decoder(slots, 64, **dec_kw)
    del noted[:]
    got = {i: ids.tolist() for i, ids, _ in dec.run(reqs, **dict(SLOT_KW, **run_kw))}
    assert sorted(got) == list(range(7)) and len({len(v) for v in got.values()}) >= 3
    _check("slots_" + case, noted, [got[i] for i in range(7)])


# ------------------------------------------------------------------ SlotDecoder.run_turns
@pytest.mark.parametrize("prefill_batch", [1, 2])
def test_slot_decoder_run_turns(prefill_batch, chain_sd, noted):
    """Two conversations, two calls each; the second call's turns reuse what their slots hold."""
    lm = _chain_model(chain_sd)
    emb_w = chain_sd["llama_model.model.embed_tokens.weight"]
    dec = lm.slot_decoder(2, C.CAPACITY)
    kw = dict(max_new_tokens=C.MAX_NEW, stop_ids=C.STOPS, eos_id=C.EOS, min_length=1, prefill_batch=prefill_batch)
    state = {s: C.first_turn(s, emb_w) for s in "ab"}
    del noted[:]
    out = []
    for k in range(2):
        got = {s: ids.tolist() for s, ids, _ in dec.run_turns([(s, state[s][0], state[s][1]) for s in "ab"], weights_version=0, **kw)}
        out.append([got["a"], got["b"]])
        if k == 0:
            state = {s: C.next_turn(s, 1, state[s][0], state[s][1], got[s], emb_w[got[s]].to(BF16).float(), emb_w) for s in "ab"}
    assert all(t["reused_tokens"] > 0 for t in dec.last_stats["turns"])
    _check("turns_prefill_batch%d" % prefill_batch, noted, out)
