"""LlamaHIP.score_continuations on the tiny golden LLaMA, with and without LoRA attached: every token's log-prob bit for bit
against the existing cache-writing path (_prefill_packed with `pasts` on cloned caches + mh_token_scores_rows), independent of
the candidates' order and neighbours, inside tests/token_scores_ref.py's bound of the float64 log-softmax of its logits row,
against the oracle's loss on prompt + candidate, and on the peaked chain fixture, where the greedy continuation must rank first."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import ops  # noqa: E402
from myriad_amd.llama import LlamaHIP  # noqa: E402
from oracle import myriad_ref as R  # noqa: E402
from tests import golden_utils as gu  # noqa: E402
from tests import token_scores_ref as T  # noqa: E402
from tests.test_sampling_gpu import _tiny  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
# candidate lengths per prompt: 1 (no segment), 2 and at least 5.  The scoring pass packs 0 + 1 + 5 + 0 + 1 + 4 = 11 rows: its
# frame pads to 64 rows like the reference's, and its lm-head launch (11 rows) is the <= 16-row weight-streaming kernel the
# reference's one-row launch is, whose rows do not depend on each other
CAND_LENS = [(1, 2, 6), (1, 2, 5)]


def _cands(V, seed):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randint(3, V, (n,), generator=g) for n in lens] for lens in CAND_LENS]


def _attach_lora(lm, sd, meta, r=8, seed=77):
    """r = 8 LoRA on q / v of the tiny golden LLaMA (the recipe of tests/test_fp8_decode_gpu.py's LoRA test); returns the oracle's
    state dict with the LoRA weights under the reference's names."""
    from myriad_amd.lora import PEFT_PREFIX, LoraQV, lora_param_specs
    from myriad_amd.myriad import ParamStore
    D, layers = meta[0], meta[1]
    gen = torch.Generator().manual_seed(seed)
    st = ParamStore(lora_param_specs(layers, D, r), DEV)
    osd = dict(sd)
    for name, ishape, _ in st.specs:
        t = (torch.randn(ishape, generator=gen) * (0.05 if "lora_A" in name else 0.1)).to(torch.bfloat16).float()
        st.p[name].copy_(t)
        osd[name.replace(PEFT_PREFIX, "llama_model.model.layers.")] = t
    lm.attach_lora(LoraQV(layers, D, r, 16.0, 0.0, st.p, st.g, DEV))
    return osd


@pytest.fixture(scope="module", params=["plain", "lora"])
def case(request):
    gd, sd, heads = _tiny()
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    prompts, lora = [gd["emb"][0, :7], gd["emb"][1, :5]], None
    if request.param == "lora":
        sd, lora = _attach_lora(lm, sd, [int(x) for x in gd["meta"]]), dict(r=8, alpha=16.0, dropout_mask=None)
        prompts = [gd["emb"][0, :7], gd["emb"][2, :9]]
    prompts = [p.to(DEV).contiguous() for p in prompts]
    cands = _cands(lm.V, 31)
    lm._decode_ws.clear()
    out, rows = lm.score_continuations(prompts, cands, return_logits=True)
    stats = dict(lm.last_score_stats)
    (ws,) = lm._decode_ws.values()                                       # the caches the call took
    return dict(name=request.param, lm=lm, sd=sd, heads=heads, lora=lora, prompts=prompts, cands=cands, out=out, rows=rows,
                stats=stats, caches=ws["caches"])


def _embed(lm, ids):
    x = torch.zeros((len(ids), lm.D), dtype=F32, device=DEV)
    lm.embed_tokens_into(ids.to(DEV), x)
    return x


def _score(lm, logits, ids):
    """ops.token_scores_rows on [R, V] f32 logits at ids: the picks' log-probs [R] on the CPU."""
    out = torch.empty((ops.SCORE_ROWS, logits.shape[0]), dtype=F32, device=DEV)
    watch = torch.full((ops.SCORE_WATCH_MAX,), -1, dtype=torch.int32, device=DEV)
    ops.token_scores_rows(logits, torch.as_tensor(ids, dtype=torch.long).to(DEV), watch, out)
    return out[1].cpu()


def _past_chunk_logits(lm, p, new, slot, caches, row):
    """_prefill_packed([p + new], [slot], caches, pasts=[S]) restated launch for launch from the parent's pieces (_decode_layers,
    ops.attn_prefill_ragged_past, _last_rows_logits), returning the logits of NEW row `row` where _prefill_packed gathers the last
    one; the test pins the restatement to _prefill_packed bit for bit at row = the last."""
    S, n = int(p.shape[0]), int(new.shape[0])
    x = torch.zeros((ops.round_up(n, 64), lm.D), dtype=F32, device=DEV)
    x[:n].copy_(new)
    pos = torch.zeros((x.shape[0],), dtype=torch.int32)
    pos[:n] = torch.arange(S, S + n, dtype=torch.int32)
    seg_host = torch.tensor([(0, n, slot, S)], dtype=torch.int32)
    pos_dev, seg_dev, scale = pos.to(DEV), seg_host.to(DEV), 1.0 / math.sqrt(lm.hd)

    def attention(li, qkv):
        return ops.attn_prefill_ragged_past(qkv, pos_dev, seg_dev, seg_host, caches[li], lm.cos, lm.sin, lm.H, lm.hd, scale)

    h = lm._decode_layers(x, lm._gemm_lin, attention, lm.lora)
    return lm._last_rows_logits(ops.gather_rows_f32(h, torch.tensor([row], dtype=torch.int32, device=DEV)))


def test_returns_f32_token_logprobs_per_candidate_and_the_stats(case):
    assert len(case["out"]) == 2
    for cs, got in zip(case["cands"], case["out"]):
        assert len(got) == len(cs)
        for c, lp in zip(cs, got):
            assert lp.shape == c.shape and lp.dtype == F32 and lp.device.type == "cpu" and bool((lp < 0).all())
    assert case["stats"] == dict(passes=2, packed_rows=sum(int(p.shape[0]) for p in case["prompts"]) + 11, segments=4, prompts=2,
                                 candidates=6)


def test_every_token_equals_the_cache_writing_path_bit_for_bit(case):
    """Token 0: mh_token_scores_rows on the packed prompt prefill's logits.  Token j >= 1: the parent's packed prefill with
    `pasts` of prompt + cand[:j] on top of the prompt's cached rows (cloned: that path writes them), its last row's logits scored
    by the same kernel.  The scoring pass wrote no cache row: the caches equal a prompt prefill's into zeros, whole.

    One token per candidate of three or more tokens needs another chunk of the same path.  The parent gives a chunk of ONE new row
    the decode kernel's arithmetic (mh_attn_fwd's rule for Sq == 1, which mh_attn_prefill_ragged_past repeats) and a longer chunk
    the tile kernel's, so its own logits after t_0 differ between the chunk cand[:1] and the first row of any longer chunk
    (measured here: 147 ulp of the log-prob at candidate (0, 2)) -- and the candidate's segment t_0 .. t_{n-2} IS a longer chunk,
    whose bits the kernel test pins to that entry's.  For j = 1 of such a candidate the reference is therefore the chunk
    cand[:2] of the same cache-writing path, first new row (_past_chunk_logits, pinned to _prefill_packed below); every other
    token, j = 1 of the two-token candidates included, is compared with _prefill_packed's own return as stated above."""
    lm, prompts, cands = case["lm"], case["prompts"], case["cands"]
    fresh = [torch.zeros_like(c) for c in case["caches"]]
    logits0 = lm._prefill_packed(prompts, [0, 1], fresh)
    for mine, ref in zip(case["caches"], fresh):
        assert torch.equal(mine.view(torch.int16), ref.view(torch.int16))
    compared = 0
    for i, (p, cs) in enumerate(zip(prompts, cands)):
        S = int(p.shape[0])
        for c, ids in enumerate(cs):
            want = [_score(lm, logits0[i:i + 1], ids[:1])[0]]
            for j in range(1, len(ids)):
                clone = [t.clone() for t in fresh]
                if j == 1 and len(ids) >= 3:                             # the segment's first row is a tile-kernel row
                    logits = _past_chunk_logits(lm, p, _embed(lm, ids[:2]), i, clone, 0)
                else:
                    logits = lm._prefill_packed([torch.cat([p, _embed(lm, ids[:j])])], [i], clone, pasts=[S])
                    if j == len(ids) - 1:                                # the restatement is the parent's path, bit for bit
                        again = _past_chunk_logits(lm, p, _embed(lm, ids[:j]), i, [t.clone() for t in fresh], j - 1)
                        assert torch.equal(again.view(torch.int32), logits.view(torch.int32))
                want.append(_score(lm, logits, ids[j:j + 1])[0])
            want = torch.stack(want)
            assert torch.equal(case["out"][i][c].view(torch.int32), want.view(torch.int32)), (case["name"], i, c, case["out"][i][c],
                                                                                              want)
            compared += len(ids)
    assert compared == sum(sum(lens) for lens in CAND_LENS)


def test_a_candidates_logprobs_do_not_depend_on_order_duplicates_or_neighbours(case):
    lm, prompts, cands, out = case["lm"], case["prompts"], case["cands"], case["out"]

    def same(a, b):
        return torch.equal(a.view(torch.int32), b.view(torch.int32))

    rev = lm.score_continuations(prompts[::-1], [cs[::-1] for cs in cands[::-1]])
    for i in range(2):
        for c in range(3):
            assert same(rev[1 - i][2 - c], out[i][c]), ("reversed", i, c)
    # a duplicate beside it, with 11 and 9 packed rows: the frame still pads to 64 rows and the lm-head launch stays the
    # <= 16-row kernel (a GEMM's plan is the one thing that depends on the row count, _prefill_packed's docstring)
    (a, b) = cands
    dup = lm.score_continuations(prompts, [[a[2], a[2]], [b[1], b[0]]])
    assert same(dup[0][0], out[0][2]) and same(dup[0][1], out[0][2]) and same(dup[1][0], out[1][1]) and same(dup[1][1], out[1][0])
    dup = lm.score_continuations(prompts, [[a[0], a[1]], [b[2], b[2]]])
    assert same(dup[1][0], out[1][2]) and same(dup[1][1], out[1][2]) and same(dup[0][0], out[0][0]) and same(dup[0][1], out[0][1])
    alone = lm.score_continuations(prompts, [[cs[2]] for cs in cands])                         # neighbours removed
    for i in range(2):
        assert same(alone[i][0], out[i][2])
    assert lm.last_score_stats["segments"] == 2 and lm.last_score_stats["passes"] == 2


def test_every_logprob_is_within_the_bound_of_the_float64_log_softmax_of_its_row(case):
    worst = 0.0
    for cs, got, rows in zip(case["cands"], case["out"], case["rows"]):
        for ids, lp, x in zip(cs, got, rows):
            assert x.shape == (len(ids), case["lm"].V) and x.dtype == F32
            for j, t in enumerate(ids.tolist()):
                row = x[j].numpy()
                E = T.bound(T.row_X(row), row.shape[0])
                _, ref = T.ref64(row, [t])
                assert T.within([float(lp[j])], ref, E), (case["name"], t, float(lp[j]), ref, E)
                worst = max(worst, abs(float(lp[j]) - float(ref[0])) / E)
    print(f"{case['name']}: worst |log-prob - float64| / bound {worst:.3f}")


def test_mean_negative_logprob_is_the_oracles_loss_on_prompt_plus_candidate(case):
    """2e-3 relative: the project's loss tolerance (header of tests/test_model_gpu.py).  Precondition: every token's probability
    is inside the oracle's clamp [1e-7, 1 - 1e-7] by a factor of 10, so the clamp does not enter."""
    sd, ew = case["sd"], case["sd"]["llama_model.model.embed_tokens.weight"]
    for i, (p, cs) in enumerate(zip(case["prompts"], case["cands"])):
        S = int(p.shape[0])
        for c, ids in enumerate(cs):
            lp = case["out"][i][c].double()
            pr = torch.exp(lp)
            assert bool((pr >= 1e-6).all()) and bool((pr <= 1 - 1e-6).all()), (i, c, pr)
            x = torch.cat([p.cpu().float(), ew[ids].float()])[None]
            labels = torch.cat([torch.full((S,), -100, dtype=torch.long), ids])[None]
            with torch.no_grad():
                loss, _ = R.llama_causal_lm(sd, x, torch.ones(1, x.shape[1], dtype=torch.long), labels, case["heads"],
                                            lora=case["lora"])
            got = -float(lp.sum()) / len(ids)
            rel = abs(got - float(loss)) / abs(float(loss))
            print(f"{case['name']} prompt {i} candidate {c} (n = {len(ids)}): -mean log-prob {got:.6f}  oracle {float(loss):.6f}  "
                  f"rel {rel:.2e}")
            assert rel < 2e-3, (case["name"], i, c, got, float(loss))


# ------------------------------------------------------------------------------------------------ the peaked chain fixture
def test_the_greedy_continuation_ranks_first_on_the_peaked_chain_and_decoding_is_undisturbed():
    c = gu.DECODE_CHAIN
    lm = LlamaHIP(gu.decode_chain_weights(), c["heads"], DEV, need_backward=False)
    emb = gu.decode_chain_inputs(["row1"]).to(DEV)
    kw = dict(max_new_tokens=12, stop_ids=(), min_length=1)
    before, sc = lm.greedy_generate(emb, return_scores=True, **kw)
    plain = lm.greedy_generate(emb, **kw)
    greedy = before[0]
    assert greedy.tolist() == gu.DECODE_CHAINS["row1"][1:13] and torch.equal(plain, before)
    # the precondition that makes `best` a theorem: a candidate that leaves the greedy ids at token j has, up to there, the
    # greedy prefix, so its log-likelihood is at most log(1 - p_j); the greedy one's is sum_j log p_j
    lp = sc["token_logprobs"][0].double()
    assert float(lp.sum()) > float(torch.log1p(-torch.exp(lp)).max())
    cands = [greedy]
    for j in (0, 5, 11):
        other = greedy.clone()
        other[j] = 7000 + j
        cands.append(other)
    out = lm.score_continuations([emb[0]], [cands])
    sums = torch.stack([t.double().sum() for t in out[0]])
    assert int(sums.argmax()) == 0 and float(sums[0]) > float(sums[1:].max())
    assert lm.last_score_stats == dict(passes=2, packed_rows=6 + 4 * 11, segments=4, prompts=1, candidates=4)
    # shared-prefix candidates agree with their common part: tokens before the change have the greedy candidate's bits
    assert torch.equal(out[0][3][:11].view(torch.int32), out[0][0][:11].view(torch.int32))
    after = lm.greedy_generate(emb, **kw)
    assert torch.equal(after, plain)


def test_refusals_reach_the_caller_before_any_launch():
    gd, sd, heads = _tiny()
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    p = gd["emb"][0, :7].to(DEV)
    for bad in ([[]], [[torch.tensor([], dtype=torch.long)]], [[torch.tensor([lm.V])]],
                [[torch.arange(3, 3 + lm.cos.shape[0]) % lm.V]]):
        with pytest.raises(ValueError):
            lm.score_continuations([p], bad)
    assert not lm._decode_ws                                             # refused by the plan: nothing was allocated or launched
