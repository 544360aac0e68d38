"""Multi-turn chat (myriad_amd/chat.py) on the HIP decode path: the split-KV decode attention kernel against an fp64 reference and
the single-workgroup kernel's cache row, and the chat session (KV cache reused across turns) against from-scratch decoding on the
model built from the reference's on-disk files (the fixtures of tests/test_entrypoints_gpu.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import ops  # noqa: E402
from myriad_amd.chat import CONV_VISION, STOP_WORDS, Chat  # noqa: E402
from myriad_amd.llama import DecodeSession  # noqa: E402
from oracle import myriad_ref as R  # noqa: E402
from tests import fp8_ref as F  # noqa: E402
from tests.test_entrypoints_gpu import DEV, _batch, fx, model  # noqa: E402,F401

BF16 = torch.bfloat16


# ------------------------------------------------------------------ kernel
def _tables(T, D):
    fr = torch.arange(T).float()[:, None] * (1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D)))[None]
    return fr.cos().contiguous(), fr.sin().contiguous()


def _rotate(x, c, s):
    """rotate-half in fp32 of a bf16 [.., D] head, rounded to bf16 once (modeling_llama.py:109-123)."""
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h].float(), x[..., h:].float()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(BF16)


def _reference(qkv, cache_after, pos, kv_len, cos, sin, H, D, scale):
    """fp64 attention of the rotated (bf16-rounded) query over the first kv_len[b] rows of the cache after the append."""
    B, W = qkv.shape[0], H * D
    out = torch.zeros((B, W), dtype=torch.float64)
    for b in range(B):
        p = int(pos[b])
        q = _rotate(qkv[b, :W].view(H, D), cos[p], sin[p]).double()
        n = int(kv_len[b])
        k = cache_after[b, :n, :W].view(n, H, D).double()
        v = cache_after[b, :n, W:].view(n, H, D).double()
        s = torch.einsum("hd,nhd->hn", q, k) * scale
        out[b] = torch.einsum("hn,nhd->hd", torch.softmax(s, -1), v).reshape(W)
    return out


@pytest.mark.parametrize("H,D", [(2, 16), (32, 128)])
@pytest.mark.parametrize("chunk", [128, 256, 512])
def test_split_decode_attention_matches_fp64_and_the_single_workgroup_row(H, D, chunk):
    """Ragged kv_len: below one chunk, exactly a multiple of the chunk, crossing chunks; the new row at pos_dev[0] inside every
    row's range, or past one row's kv_len (written, not attended)."""
    torch.manual_seed(H * 7 + chunk)
    W, T = H * D, 2048
    cos, sin = _tables(T, D)
    for kv_len, prow in (([chunk // 2, chunk, 2 * chunk + 37], chunk // 2 - 1), ([3 * chunk + 5], 3 * chunk + 4),
                         ([chunk, 40], chunk - 1)):
        B = len(kv_len)
        kvl = torch.tensor(kv_len, dtype=torch.int32)
        pos = torch.tensor([min(n, T) - 1 for n in kv_len], dtype=torch.int32)
        qkv = (torch.randn(B, 3 * W) * 0.7).to(BF16)
        cache0 = (torch.randn(B, T, 2 * W) * 0.7).to(BF16)
        scale = 1.0 / D ** 0.5
        d = lambda t: t.to(DEV)
        args = (d(pos), d(torch.tensor([prow], dtype=torch.int32)), d(kvl), d(cos), d(sin), H, D, scale)
        part = ops.attn_decode_split_ws(B, H, T, DEV, chunk=chunk)
        runs = []
        for _ in range(2):
            c, q = d(cache0), d(qkv)
            o = ops.attn_decode_rope_split(q, c, args[0], args[1], args[2], *args[3:], part, chunk=chunk)
            torch.cuda.synchronize()
            assert torch.equal(q.cpu(), qkv)                            # q is rotated in registers, qkv is left alone
            runs.append((o.cpu(), c.cpu()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])      # run to run: the same bits
        o, c = runs[0]
        c_single, q_single = d(cache0), d(qkv)
        o_single = ops.attn_decode_rope(q_single, c_single, *args)
        c_single = c_single.cpu()
        assert torch.equal(c[:, prow], c_single[:, prow])              # the appended row: mh_attn_decode_rope's bits
        untouched = torch.ones(T, dtype=torch.bool)
        untouched[prow] = False
        assert torch.equal(c[:, untouched], cache0[:, untouched])       # every other row, past kv_len too (canaries)
        ref = _reference(qkv, c, pos, kvl, cos, sin, H, D, scale)
        err = (o.double() - ref).abs()
        # bf16 output: half an ulp (2^-9 relative) of the value, plus fp32 accumulation over <= 1.1k keys
        bound = ref.abs() * 2.0 ** -8 + 1e-4
        assert bool((err <= bound).all()), (kv_len, float((err - bound).max()))
        assert float((o.double() - o_single.cpu().double()).abs().max()) <= float((ref.abs() * 2.0 ** -7 + 2e-4).max())


def test_split_decode_attention_replays_from_a_graph_as_the_context_grows():
    torch.manual_seed(3)
    B, H, D, T = 1, 32, 128, 1024
    W = H * D
    cos, sin = (t.to(DEV) for t in _tables(T, D))
    cache = (torch.randn(B, T, 2 * W, device=DEV) * 0.7).to(BF16)
    qkv = (torch.randn(B, 3 * W, device=DEV) * 0.7).to(BF16)
    pos = torch.zeros((B,), dtype=torch.int32, device=DEV)
    kvl = torch.zeros((B,), dtype=torch.int32, device=DEV)
    part = ops.attn_decode_split_ws(B, H, T, DEV)
    out = torch.empty((B, W), dtype=BF16, device=DEV)
    step = lambda c, o: ops.attn_decode_rope_split(qkv, c, pos, pos, kvl, cos, sin, H, D, 0.088, part, out=o)
    pos.fill_(9)
    kvl.fill_(10)
    step(cache, out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(cache, out)
    for n in (11, 200, 256, 257, 700, 1024):
        pos.fill_(n - 1)
        kvl.fill_(n)
        before = cache.clone()
        g.replay()
        eager_c = before.clone()
        eager_o = step(eager_c, None)
        torch.cuda.synchronize()
        assert torch.equal(out, eager_o), n
        assert torch.equal(cache, eager_c), n


# ------------------------------------------------------------------ chat session
def _img(samples, i):
    return samples["image"][i:i + 1], dict(anomaly_maps=samples["anomaly_maps"][i:i + 1])


def _context(chat, conv, img_list, max_new, max_length=2000):
    c = conv.copy()
    c.append_message(c.roles[1], None)
    emb, _ = chat.get_context_emb(c, img_list)
    begin = max(0, emb.shape[1] + max_new - max_length)
    return emb[:, begin:].contiguous()


def _turn(chat, conv, img_list, q, max_new=12, **kw):
    chat.ask(q, conv)
    emb = _context(chat, conv, img_list, max_new, kw.get("max_length", 2000))
    text, toks = chat.answer(conv, img_list, max_new_tokens=max_new, do_sample=kw.pop("do_sample", False), **kw)
    return emb, chat.last_token_ids[0].cpu(), dict(chat.last_stats)


def _compare_scratch(model, fx, emb, ids, max_new):
    """ids equal from-scratch greedy_generate's up to the oracle's first two-ulp near tie; returns the steps compared."""
    ref_ids, _ = model.llama.greedy_generate(emb, max_new_tokens=max_new, stop_ids=STOP_WORDS, eos_id=2, min_length=1,
                                             return_margins=True)
    with torch.no_grad():
        o_ids, o_mar, o_sc = R.greedy_generate(fx["sd"], emb.cpu(), 32, max_new_tokens=max_new, stop_ids=STOP_WORDS, eos_id=2,
                                               min_length=1, return_margins=True, return_scales=True)
    first = min(F.two_ulp_horizon(o_mar, o_sc), ids.shape[0], ref_ids.shape[1])
    assert torch.equal(ids[:first], ref_ids[0, :first].cpu()), (first, ids, ref_ids)
    return first


@pytest.mark.parametrize("split", [None, True])
def test_three_turn_chat_reuses_the_cache_and_matches_from_scratch(model, fx, split):
    """split=None: the session's rule (contexts of a few hundred keys: the single-workgroup kernel); True: the split-KV kernel."""
    model.eval()
    try:
        samples = _batch(3, train=False, seed=5)
        chat, conv, imgs = Chat(model, device=DEV), CONV_VISION.copy(), []
        if split:
            chat.session = DecodeSession(model.llama, 2000 + 12 + 2, split=True)
        im, ex = _img(samples, 0)
        assert chat.upload_img(im, conv, imgs, **ex)[0] == "Received."
        checked = 0
        for t, q in enumerate(["Is there a defect?", "Where is it?", "Compare the two new images."]):
            if t == 2:
                for i in (1, 2):
                    im, ex = _img(samples, i)
                    chat.upload_img(im, conv, imgs, **ex)
            emb, ids, st = _turn(chat, conv, imgs, q)
            assert st["context_tokens"] == emb.shape[1]
            assert st["prefilled_tokens"] == st["context_tokens"] - st["reused_tokens"]
            if t == 0:
                assert st["reused_tokens"] == 0 and st["full_reprefill_reason"] == "empty cache"
            else:
                assert st["reused_tokens"] > 0 and st["full_reprefill_reason"] is None, st
            assert st["split_kv"] is bool(split)
            assert conv.messages[-1][0] == "Assistant" and isinstance(conv.messages[-1][1], str)
            checked += _compare_scratch(model, fx, emb, ids, 12)
        assert checked > 0
        assert chat.last_stats["graph_captures"] == 1 and chat.session.graph_captures == 1
        assert chat.last_stats["graph_replays"] > 0
    finally:
        model.train()


def test_other_generate_calls_leave_the_session_alone(model):
    model.eval()
    try:
        samples = _batch(3, train=False, seed=8)
        outs = []
        for interfere in (False, True):
            chat, conv, imgs = Chat(model, device=DEV), CONV_VISION.copy(), []
            im, ex = _img(samples, 0)
            chat.upload_img(im, conv, imgs, **ex)
            _turn(chat, conv, imgs, "Is there a defect?")
            if interfere:
                for n in (2, 3):                                       # other batch sizes: the _decode_ws LRU churns
                    model.generate(_batch(n, train=False, seed=n), max_new_tokens=6)
            _, ids, st = _turn(chat, conv, imgs, "Where is it?")
            assert st["reused_tokens"] > 0
            outs.append(ids)
        assert torch.equal(outs[0], outs[1])
    finally:
        model.train()


def test_training_step_and_window_invalidate_the_cache(model, fx):
    samples = _batch(3, train=False, seed=9)
    model.eval()
    chat, conv, imgs = Chat(model, device=DEV), CONV_VISION.copy(), []
    im, ex = _img(samples, 0)
    chat.upload_img(im, conv, imgs, **ex)
    _turn(chat, conv, imgs, "Is there a defect?")
    model.train()
    model.train_step(_batch(2, train=True, seed=4), lr=1e-4)
    model.finish_update()
    model.eval()
    try:
        emb, ids, st = _turn(chat, conv, imgs, "Where is it?")
        assert st["reused_tokens"] == 0 and st["full_reprefill_reason"] == "weights changed", st
        _turn(chat, conv, imgs, "Anything else?")
        assert chat.last_stats["reused_tokens"] > 0
        # past max_length: the reference's window is prefilled alone, from position 0
        chat.ask("And now?", conv)
        full = _context(chat, conv, imgs, 12).shape[1]
        max_length = full + 12 - 8                                     # begin_idx = 8
        emb = _context(chat, conv, imgs, 12, max_length)
        with pytest.warns(RuntimeWarning):
            chat.answer(conv, imgs, max_new_tokens=12, do_sample=False, max_length=max_length)
        st, ids = chat.last_stats, chat.last_token_ids[0].cpu()
        assert st["full_reprefill_reason"] == "window" and st["reused_tokens"] == 0
        assert st["context_tokens"] == emb.shape[1] == full - 8
        _compare_scratch(model, fx, emb, ids, 12)
    finally:
        model.train()


@pytest.mark.parametrize("device_sampling", [False, True])
def test_sampled_turns_are_reproducible(model, device_sampling):
    samples = _batch(2, train=False, seed=11)
    model.eval()
    prev = model.llama.device_sampling
    model.llama.device_sampling = device_sampling
    try:
        runs = []
        for _ in range(2):
            chat, conv, imgs = Chat(model, device=DEV), CONV_VISION.copy(), []
            im, ex = _img(samples, 0)
            chat.upload_img(im, conv, imgs, **ex)
            g = torch.Generator().manual_seed(21)
            got = []
            for q in ("Is there a defect?", "Where is it?"):
                chat.ask(q, conv)
                text, toks = chat.answer(conv, imgs, max_new_tokens=10, do_sample=True, top_p=0.9, temperature=1.0, generator=g)
                assert isinstance(toks, np.ndarray)
                got.append(chat.last_token_ids[0].cpu())
            assert chat.last_stats["reused_tokens"] > 0
            runs.append(got)
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        st = model.llama.last_generate_stats
        if device_sampling:
            assert st["device_sampled_rows"] > 0 and st["host_sampled_rows"] == 0
    finally:
        model.llama.device_sampling = prev
        model.train()
