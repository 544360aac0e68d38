"""The q/v LoRA merged into the decode token step's weights (LlamaHIP.decode_merge_lora) on the MI355X: the merge kernel against
float64 and the stated fp32 rule, its packed copies against gemv_pack / gemv_pack_fp8 of its row-major output, and the merged
token step (bf16 and fp8) against the reference loop of tests/lora_merge_ref.py (exact LoRA in the prefill, merged weights in
every later step), training in between, switch flips, chat sessions and beams."""
import numpy as np
import pytest
import torch

from myriad_amd import _lib, ops
from myriad_amd.llama import DecodeSession, LlamaHIP
from myriad_amd.lora import PEFT_PREFIX, LoraQV, lora_param_specs, merged_qv_names
from tests import fp8_ref as F
from tests import golden_utils as gu
from tests import lora_merge_ref as LM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32


def _case(D, r, seed, b_std=0.05, zero_b=False):
    """W [3D, D] as the frozen columns of a bordered [3D, D + 64] buffer (ld = D + 64), fp32 masters; CPU and device copies."""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(3 * D, D, generator=g) * 0.02).to(BF16)
    a = ((torch.rand(2 * r, D, generator=g) * 2 - 1) / D ** 0.5).contiguous()
    bq, bv = torch.randn(D, r, generator=g) * b_std, torch.randn(D, r, generator=g) * b_std
    if zero_b:
        bq.zero_(), bv.zero_()
    ext = torch.zeros(3 * D, D + 64, dtype=BF16, device=DEV)
    ext[:, :D].copy_(w)
    ext[:, D:].fill_(1.0)                                          # the border must not be read
    dev = (ext[:, :D], a.to(DEV), bq.to(DEV), bv.to(DEV))
    return dev, (w, a, bq, bv)


# ------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("D,r", [(4096, 8), (4096, 16), (64, 8), (64, 16), (192, 8), (320, 16)])
def test_merge_kernel_against_float64_and_the_stated_rule(D, r):
    dev, (w, a, bq, bv) = _case(D, r, seed=D * 3 + r)
    s = 16.0 / r
    m = ops.lora_merge(*dev, s).cpu()
    assert m.shape == (3 * D, D) and m.dtype == BF16
    # bit for bit the rule as stated (fp32, j in order, no FMA), restated in torch
    assert torch.equal(m.view(torch.int16), LM.merge_rows(w, a, bq, bv, s).view(torch.int16))
    assert torch.equal(m[D:2 * D].view(torch.int16), w[D:2 * D].view(torch.int16))          # k rows: W bit for bit
    exact_all, bound_all = LM.merge_float64(w.float(), a, bq, bv, s), LM.fp32_sum_bound(a, bq, bv, s, D)
    for rows in (slice(0, D), slice(2 * D, 3 * D)):
        exact = exact_all[rows]
        dist = LM.ulp_distance(m[rows], exact)
        # one bf16 ulp of the float64 value; where W and s B A nearly cancel, the fp32 rounding of the rank-r sum may add more
        slack = bound_all[rows] / F.bf16_ulp(exact)
        assert bool(((dist <= 1.0) | (dist <= 0.5 + slack)).all()), float(dist.max())
        assert float((dist > 1.0).double().mean()) < 1e-5
        assert float((m[rows].float() != w[rows].float()).float().mean()) > 0.5                 # the merge moved the rows


@pytest.mark.parametrize("D,r", [(4096, 8), (192, 16)])
def test_zero_b_gives_w_bit_for_bit(D, r):
    dev, (w, _, _, _) = _case(D, r, seed=1, zero_b=True)
    m = ops.lora_merge(*dev, 2.0).cpu()
    assert torch.equal(m.view(torch.int16), w.view(torch.int16))


def test_merge_refuses_bad_arguments():
    D, r = 192, 8
    (wd, ad, bqd, bvd), _ = _case(D, r, seed=2)
    lib = _lib.load()
    out = torch.empty(3 * D, D, dtype=BF16, device=DEV)
    ok = (wd.data_ptr(), wd.stride(0), ad.data_ptr(), bqd.data_ptr(), bvd.data_ptr(), D, r, 2.0, out.data_ptr(), D, ops._s())
    assert lib.mh_lora_merge(*ok) == 0
    bad = {5: 100, 6: 12}                                           # D % 64 != 0, r not 8 / 16
    for i, v in bad.items():
        args = list(ok)
        args[i] = v
        assert lib.mh_lora_merge(*args) == -1, (i, v)
    for i, v in ((1, D - 8), (1, D + 4), (9, D - 8), (9, D + 2), (0, wd.data_ptr() + 2), (2, ad.data_ptr() + 4),
                 (8, out.data_ptr() + 2), (3, bqd.data_ptr() + 2), (3, None), (5, 0), (5, -64)):
        args = list(ok)
        args[i] = v
        assert lib.mh_lora_merge(*args) == -1, (i, v)
    pk = torch.empty(lib.mh_gemv_pack_elems(3 * D, D), dtype=BF16, device=DEV)
    assert lib.mh_lora_merge_pack(wd.data_ptr(), wd.stride(0), ad.data_ptr(), bqd.data_ptr(), bvd.data_ptr(), D, 4, 2.0,
                                  pk.data_ptr(), ops._s()) == -1
    q = torch.empty(lib.mh_gemv_pack_fp8_elems(3 * D, D), dtype=torch.uint8, device=DEV)
    sc = torch.empty(3 * D, dtype=F32, device=DEV)
    base = (wd.data_ptr(), wd.stride(0), ad.data_ptr(), bqd.data_ptr(), bvd.data_ptr(), D, r, 2.0, q.data_ptr())
    assert lib.mh_lora_merge_pack_fp8(*base, None, ops._s()) == -1
    assert lib.mh_lora_merge_pack_fp8(*base, sc.data_ptr() + 2, ops._s()) == -1
    assert lib.mh_lora_merge_pack_fp8(*base, sc.data_ptr(), ops._s()) == 0
    with pytest.raises(_lib.MyriadHipError):
        ops.lora_merge(wd[:, :64], ad, bqd, bvd, 2.0)               # not [3D, D]
    with pytest.raises(_lib.MyriadHipError):
        ops.lora_merge(wd, ad.t().contiguous().t(), bqd, bvd, 2.0)   # A not row-contiguous
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- packs
@pytest.mark.parametrize("D,r", [(4096, 8), (4096, 16), (2880, 16), (64, 8), (192, 16), (320, 8)])
def test_packs_equal_gemv_pack_of_the_merged_rows(D, r):
    """(2880: 540 blocks of 16 rows -> 4 waves, 45 steps padded to 48; 64 / 192 / 320: 8 waves, zero steps past K)"""
    dev, _ = _case(D, r, seed=D + 11 * r)
    s = 16.0 / r
    m = ops.lora_merge(*dev, s)
    pb, ref = ops.lora_merge_pack(*dev, s), ops.gemv_pack(m)
    assert torch.equal(pb.data.view(torch.int16), ref.data.view(torch.int16))
    p8, ref8 = ops.lora_merge_pack_fp8(*dev, s), ops.gemv_pack_fp8(m)
    assert torch.equal(p8.data, ref8.data)
    assert torch.equal(p8.scales.view(torch.int32), ref8.scales.view(torch.int32))
    # out= re-use overwrites every byte
    pb.data.fill_(7.0)
    p8.data.fill_(0x7F)
    p8.scales.fill_(-1.0)
    assert ops.lora_merge_pack(*dev, s, out=pb) is pb and ops.lora_merge_pack_fp8(*dev, s, out=p8) is p8
    assert torch.equal(pb.data.view(torch.int16), ref.data.view(torch.int16))
    assert torch.equal(p8.data, ref8.data) and torch.equal(p8.scales.view(torch.int32), ref8.scales.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------- model
def _tiny():
    g = np.load(__file__.rsplit("/", 1)[0] + "/golden/llama_tiny.npz")
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in g.items()}
    D, layers, heads, inter, V, seed = [int(x) for x in g["meta"]]
    sd = {k: (v.to(BF16).float() if v.is_floating_point() and v.dim() == 2 else v)
          for k, v in gu.llama_weights(D, layers, inter, V, seed=seed, std=0.2).items()}
    return g, sd, heads, D, layers


def _lora_model(r=8, zero_b=False, seed=77):
    """The flat llama_tiny fixture with LoRA r on q/v (bf16-valued masters, as test_fp8_decode_gpu's LoRA case); returns the
    fixture, the oracle state dict with the LoRA keys, the model and its ParamStore."""
    from myriad_amd.myriad import ParamStore
    g, sd, heads, D, layers = _tiny()
    gen = torch.Generator().manual_seed(seed)
    st = ParamStore(lora_param_specs(layers, D, r), DEV)
    osd = dict(sd)
    for name, ishape, _ in st.specs:
        t = (torch.randn(ishape, generator=gen) * (0.05 if "lora_A" in name else 0.1)).to(BF16).float()
        if zero_b and "lora_B" in name:
            t.zero_()
        st.p[name].copy_(t)
        osd[name.replace(PEFT_PREFIX, "llama_model.model.layers.")] = t
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    lm.attach_lora(LoraQV(layers, D, r, 16.0, 0.0, st.p, st.g, DEV))
    return g, osd, heads, lm, st


def _expected_bytes(lm, kind, merged):
    L = _lib.load()
    total = 2 * L.mh_gemv_pack_elems(*lm.lm_head.shape)
    for layer in lm.layers:
        for k in ("wqkv_ext", "wo", "wgu", "wd"):
            N, K = layer[k].shape
            if k == "wqkv_ext" and merged:
                K -= 64
            fp8 = kind == "fp8" and (k != "wqkv_ext" or merged)
            total += (L.mh_gemv_pack_fp8_elems(N, K) + 4 * N) if fp8 else 2 * L.mh_gemv_pack_elems(N, K)
    return total


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_flat_logit_merged_decode_ids_equal_the_merged_reference(kind):
    g, osd, heads, lm, _ = _lora_model()
    D, layers = lm.D, len(lm.layers)
    lm.decode_fp8 = kind == "fp8"
    lm.decode_merge_lora = True
    lora = dict(r=8, alpha=16.0, dropout_mask=None)
    sd_step = LM.merged_step_state_dict(osd, layers, 2.0)
    if kind == "fp8":
        sd_step = F.fp8_state_dict(sd_step)                          # q/k/v (merged), o, gate, up, down: fp8 round trips
    emb = g["emb"]
    checked, longest = 0, 0
    for row in range(emb.shape[0]):
        for s0 in (5, 7, 9):
            e = emb[row:row + 1, :s0]
            with torch.no_grad():
                ids_ref, _, margins, scales = F.greedy_decode(osd, sd_step, e, heads, 40, lora=lora)
            ids = lm.greedy_generate(e.to(DEV), max_new_tokens=40, stop_ids=())
            st = lm.last_generate_stats
            assert st["decode_weights"] == kind and st["lora_merged"] is True
            first = F.two_ulp_horizon(margins, scales)
            assert ids.shape[1] >= first, (row, s0, ids.shape, first)
            assert torch.equal(ids[:, :first].cpu(), ids_ref[:, :first]), (row, s0, first, ids[:, :first + 1], ids_ref[:, :first + 1])
            checked += first
            longest = max(longest, first)
    # the reference's margins admit 24 steps (8 on the longest run) for bf16 and 49 (16) for fp8; floors so the test cannot pass
    # on a handful
    floor = {"bf16": (20, 6), "fp8": (40, 12)}[kind]
    assert checked >= floor[0] and longest >= floor[1], (checked, longest)
    P = lm._packed["layers"]
    for i in range(layers):
        assert (P[i]["wqkv"].N, P[i]["wqkv"].K) == (3 * D, D)        # the merged [3D, D] copy, not the bordered [3D, D + 64] one
        assert isinstance(P[i]["wqkv"], ops.PackedFp8Weight if kind == "fp8" else ops.PackedWeight)
    # the bytes tell a merged fp8 step from one that stayed bordered (bf16 qkv); at D = 64 the bf16 copies of [3D, 64] and
    # [3D, 128] pad to the same 8 steps, so there the [3D, D] shape above is what tells them apart
    assert st["decode_weight_bytes"] == _expected_bytes(lm, kind, merged=True)
    if kind == "fp8":
        assert st["decode_weight_bytes"] < _expected_bytes(lm, kind, merged=False)
    assert st["lora_merges"] == 9                                    # a bare LlamaHIP without a version re-merges at every call


def test_off_is_the_bordered_path_and_on_without_lora_or_with_zero_b_changes_nothing():
    g, osd, heads, lm, _ = _lora_model()
    x = g["emb"][:2, :9].to(DEV)
    kw = dict(max_new_tokens=24, stop_ids=())
    ref = lm.greedy_generate(x, **kw)                                # default: off
    st_ref = dict(lm.last_generate_stats)
    assert lm.decode_merge_lora is False and st_ref["lora_merged"] is False and st_ref["lora_merges"] == 0
    assert st_ref["decode_weight_bytes"] == _expected_bytes(lm, "bf16", merged=False)
    lm.decode_merge_lora = True
    lm.greedy_generate(x, **kw)
    lm.decode_merge_lora = False
    again = lm.greedy_generate(x, **kw)
    assert torch.equal(again, ref) and lm.last_generate_stats["decode_weight_bytes"] == st_ref["decode_weight_bytes"]
    # no LoRA attached: the switch changes nothing
    _, sd, heads2, _, _ = _tiny()
    plain, plain_on = LlamaHIP(sd, heads2, DEV, need_backward=False), LlamaHIP(sd, heads2, DEV, need_backward=False)
    plain_on.decode_merge_lora = True
    a, b = plain.greedy_generate(x, **kw), plain_on.greedy_generate(x, **kw)
    assert torch.equal(a, b)
    assert plain_on.last_generate_stats["lora_merged"] is False and plain_on.last_generate_stats["lora_merges"] == 0
    assert plain_on.last_generate_stats["decode_weight_bytes"] == plain.last_generate_stats["decode_weight_bytes"]
    # B = 0 (PEFT init): the merged copy is W, and the ids are the bordered path's exactly
    _, _, _, lz, _ = _lora_model(zero_b=True)
    bordered = lz.greedy_generate(x, **kw)
    lz.decode_merge_lora = True
    merged = lz.greedy_generate(x, **kw)
    assert lz.last_generate_stats["lora_merged"] is True
    assert torch.equal(merged, bordered), (merged, bordered)


def test_switch_flips_share_no_graph_or_workspace():
    g, _, _, lm, st = _lora_model()
    x = g["emb"][:2, :9].to(DEV)
    kw = dict(max_new_tokens=24, stop_ids=())
    seq = [(True, False), (True, True), (False, False), (False, True), (True, False)]     # (merge, fp8)
    got = []
    for merge, fp8 in seq:
        lm.decode_merge_lora, lm.decode_fp8 = merge, fp8
        got.append(lm.greedy_generate(x, **kw))
        s = lm.last_generate_stats
        assert s["lora_merged"] is merge and s["decode_weights"] == ("fp8" if fp8 else "bf16") and s["graph_replays"] > 0
    for (merge, fp8), ids in zip(seq, got):
        fresh = LlamaHIP(*_tiny()[1:3], DEV, need_backward=False)
        fresh.attach_lora(LoraQV(len(fresh.layers), fresh.D, 8, 16.0, 0.0, st.p, st.g, DEV))
        fresh.decode_merge_lora, fresh.decode_fp8 = merge, fp8
        assert torch.equal(ids, fresh.greedy_generate(x, **kw)), (merge, fp8)


def test_chat_session_resets_when_the_merge_switch_flips():
    g, _, _, lm, st = _lora_model()
    emb = g["emb"][:1].to(DEV)
    keys = lambda n: [[("x", p) for p in range(n)]]
    kw = dict(max_new_tokens=10, stop_ids=(), eos_id=2, min_length=1)
    sess = DecodeSession(lm, 64)
    lm.decode_merge_lora = True
    lm.decode_lora_version = 0
    sess.generate(emb[:, :6], keys(6), weights_version=0, **kw)
    sess.generate(emb[:, :8], keys(8), weights_version=0, **kw)
    assert sess.last_stats["reused_tokens"] > 0 and lm.last_generate_stats["lora_merges"] == 1      # same version: no re-merge
    for merge in (False, True):
        lm.decode_merge_lora = merge
        ids = sess.generate(emb[:, :10], keys(10), weights_version=0, **kw)
        assert sess.last_stats["reused_tokens"] == 0, sess.last_stats
        assert sess.last_stats["full_reprefill_reason"] == "decode weights changed", sess.last_stats
        fresh = LlamaHIP(*_tiny()[1:3], DEV, need_backward=False)
        fresh.attach_lora(LoraQV(len(fresh.layers), fresh.D, 8, 16.0, 0.0, st.p, st.g, DEV))
        fresh.decode_merge_lora = merge
        assert torch.equal(ids, fresh.greedy_generate(emb[:, :10], **kw)), merge
    # merged weights that change under the same caller version: the re-merge alone resets the cache
    lm.decode_lora_version = None
    sess.generate(emb[:, :11], keys(11), weights_version=0, **kw)
    assert sess.last_stats["full_reprefill_reason"] == "decode weights changed"


def test_beams_run_on_the_merged_fp8_step():
    g, _, _, lm, _ = _lora_model()
    lm.decode_fp8 = lm.decode_merge_lora = True
    x = g["emb"][:, :7].to(DEV)                                      # 3 items x 4 beams = 12 rows
    kw = dict(max_new_tokens=10, stop_ids=(), eos_id=2, min_length=1, length_penalty=1.0, early_stopping=False,
              num_return_sequences=2, return_scores=True)
    ids, scores = lm.beam_generate(x, 4, **kw)
    st = lm.last_generate_stats
    assert st["lora_merged"] is True and st["decode_weights"] == "fp8" and st["graph_replays"] > 0
    assert st["decode_weight_bytes"] == _expected_bytes(lm, "fp8", merged=True)
    ids2, scores2 = lm.beam_generate(x, 4, **kw)
    assert torch.equal(ids, ids2) and torch.equal(torch.as_tensor(scores), torch.as_tensor(scores2))
    lm.beam_generate(g["emb"][:, :7].repeat(2, 1, 1).to(DEV), 3, **kw)    # 18 rows: the bordered GEMM path
    assert lm.last_generate_stats["lora_merged"] is False


def test_training_step_triggers_one_re_merge():
    from tests import dp_common
    model, cfg = dp_common.build_model(DEV)
    model.llama.decode_merge_lora = True
    smp = dp_common.batch(0, 0, 1024, DEV)                         # build_model's vocabulary
    gen = dict(max_new_tokens=4, stop_ids=((-1,),), min_length=0, eos_token_id=-5)
    model.eval()
    model.generate(smp, **gen)
    n0 = model.last_generate_stats["lora_merges"]
    assert model.last_generate_stats["lora_merged"] is True and n0 == 1
    model.generate(smp, **gen)
    assert model.last_generate_stats["lora_merges"] == n0                      # unchanged weights: no re-merge
    names = model.lora.names(0)
    b0 = model.store.p[names[2]].clone()
    model.train()
    model.train_step(smp, lr=1e-3)
    model.finish_update()
    model.eval()
    assert not torch.equal(b0, model.store.p[names[2]])                        # the step moved B_q
    model.generate(smp, **gen)
    assert model.last_generate_stats["lora_merges"] == n0 + 1
    for i, L in enumerate(model.llama.layers):
        fresh = model.lora.merge_layer(i, L, "bf16")
        assert torch.equal(model.llama._packed["layers"][i]["wqkv"].data.view(torch.int16), fresh.data.view(torch.int16))
    model.generate(smp, **gen)
    assert model.last_generate_stats["lora_merges"] == n0 + 1
    # the merge_and_unload view: the kernel's row-major merge under the reference names
    msd = model.merged_lora_state_dict()
    D = model.llama.D
    assert list(msd) == [n for i in range(len(model.llama.layers)) for n in merged_qv_names(i)]
    rows = model.lora.merge_layer(0, model.llama.layers[0], "rows")
    assert torch.equal(msd[merged_qv_names(0)[0]], rows[:D]) and torch.equal(msd[merged_qv_names(0)[1]], rows[2 * D:])
    model.train()
