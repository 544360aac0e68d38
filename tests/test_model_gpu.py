"""GPU parity of the assembled HIP sub-models and the full Myriad/MiniGPT4 step against (a) the committed golden
vectors produced by the reference's own modules and (b) the CPU oracle on the same seeded inputs.

Tolerances (stated, bf16 operands / fp32 accumulation, vs an fp32 reference):
  activations / logits : 2e-2 of the tensor's max-abs   loss : 2e-3 relative   gradients : 5e-2 of max-abs
Greedy token ids: exact equality wherever the oracle's top-1/top-2 logit margin exceeds 0.05."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd.eva_vit import EvaViTHIP  # noqa: E402
from myriad_amd.llama import LlamaHIP  # noqa: E402
from myriad_amd.myriad import MiniGPT4HIP, MyriadHIP  # noqa: E402
from myriad_amd.networks import from_reference_layout  # noqa: E402
from myriad_amd.qformer import QFormerHIP  # noqa: E402
from myriad_amd import _lib as L, ops  # noqa: E402
from oracle import myriad_ref as R  # noqa: E402
from tests import golden_utils as gu  # noqa: E402

DEV = "cuda:0"
G = os.path.join(os.path.dirname(__file__), "golden")


def load(name):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(G, name + ".npz")).items()}


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def cos_sim(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


def bf16_round(sd):
    """The HIP path holds frozen weights in bf16; give the oracle the same (bf16-representable) values so the
    comparison isolates arithmetic, not weight quantisation."""
    return {k: (v.to(torch.bfloat16).float() if v.is_floating_point() and v.numel() > 4096 else v) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------ ViT
def test_vit_tiny_vs_golden():
    g = load("vit_tiny")
    D, depth, heads, hidden, img, seed = [int(x) for x in g["meta"]]
    sd = gu.vit_weights(D, depth, heads, hidden, 14, 17, seed=seed)
    vit = EvaViTHIP(sd, heads, DEV)
    y = vit.forward(g["image"].to(DEV))
    assert relerr(y, g["out"]) < 2e-2


def test_vit_fullwidth_vs_golden():
    g = load("vit_fullwidth")
    D, depth, heads, hidden, img, seed = [int(x) for x in g["meta"]]
    sd = gu.vit_weights(D, depth, heads, hidden, 14, 257, seed=seed)
    x = torch.randn(1, 3, img, img, generator=torch.Generator().manual_seed(int(g["image_seed"][0])))
    y = EvaViTHIP(sd, heads, DEV).forward(x.to(DEV))
    assert relerr(y[:, ::8, ::4], g["out_sub"]) < 2e-2


# ------------------------------------------------------------------------------------------------ Q-Former
def test_qformer_fullwidth_fwd_bwd_vs_golden():
    g = load("qformer_fullwidth")
    D, layers, heads, inter, enc_w, seed = [int(x) for x in g["meta"]]
    sd = gu.qformer_weights(D, layers, inter, enc_w, seed=seed)
    gen = torch.Generator().manual_seed(int(g["seed"][1]))
    q = torch.randn(1, 81, D, generator=gen)
    e = torch.randn(1, 257, enc_w, generator=gen)
    ct = torch.randn(1, 81, D, generator=gen)
    qf = QFormerHIP(sd, heads, DEV)
    y = qf.forward(q.to(DEV), e.to(DEV).to(torch.bfloat16))
    assert relerr(y[:, :, ::4], g["out_sub"]) < 2e-2
    dq, de = qf.backward(ct.to(DEV))
    assert relerr(dq[:, :, ::4], g["dquery_sub"]) < 5e-2
    assert relerr(de[:, ::4, ::8], g["denc_sub"]) < 5e-2


# ------------------------------------------------------------------------------------------------ LLaMA
@pytest.mark.parametrize("sampled", [False, True])
def test_decode_chain_every_generated_id_equals_the_reference(sampled):
    """KV-cache decode (prefill, eager step, hipGraph replay, packed weight copies) on the peaked-logit fixture generated
    by the reference's own LLaMA (tests/golden/decode_chain.npz): >= 30 tokens, the eval script's stop ids ([835] and the
    two-token [2277, 29937] on row 0), the min_length EOS ban, a row that finishes early and is padded.  EVERY id must be
    equal, at batch 4 and batch 1; with the eval script's `do_sample=True, top_p=0.01, temperature=1.0`
    (evaluation_aqa_dataset.py:289-301) the kernel-reported p_max proves each step was the arg-max."""
    g = load("decode_chain")
    c = gu.DECODE_CHAIN
    sd = gu.decode_chain_weights()
    lm = LlamaHIP(sd, c["heads"], DEV, need_backward=False)
    kw = dict(do_sample=True, top_p=0.01, temperature=1.0) if sampled else {}
    for name, rows in (("b4", ["row0", "row1", "row2", "row3"]), ("b1", ["row0"]), ("stop835", ["stop835"])):
        ids = lm.greedy_generate(gu.decode_chain_inputs(rows).to(DEV), max_new_tokens=90, min_length=1, **kw)
        assert torch.equal(ids, g[name + "_ids"]), (name, ids, g[name + "_ids"])
        st = lm.last_generate_stats
        assert st["steps"] == ids.shape[1] and st["sampled_rows"] == 0
        if sampled:
            assert st["min_pmax"] >= 0.01


def test_top_p_sampling_falls_back_to_a_real_draw_on_flat_logits():
    """p_max < top_p: HF's warper keeps several tokens and the reference draws among them -- the decode loop must not
    silently take the arg-max.  Tiny random-weight model: logits are flat (p_max ~ 1/V)."""
    gd = load("llama_tiny")
    D, layers, heads, inter, V, seed = [int(x) for x in gd["meta"]]
    lm = LlamaHIP(gu.llama_weights(D, layers, inter, V, seed=seed, std=0.02), heads, DEV, need_backward=False)
    emb = gd["emb"][:2, :7].to(DEV)
    gen = torch.Generator().manual_seed(5)
    a = lm.greedy_generate(emb, max_new_tokens=6, stop_ids=(), do_sample=True, top_p=0.9, generator=gen)
    st = dict(lm.last_generate_stats)
    assert st["sampled_rows"] > 0 and st["min_pmax"] < 0.9
    b = lm.greedy_generate(emb, max_new_tokens=6, stop_ids=(), do_sample=True, top_p=0.9, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a, b)                                                    # reproducible through the generator
    greedy = lm.greedy_generate(emb, max_new_tokens=6, stop_ids=())
    assert lm.last_generate_stats["sampled_rows"] == 0 and greedy.shape == a.shape
    # HF's TopKLogitsWarper runs before top-p (default top_k = 50): with top_k = 1 every host draw can only return the arg-max
    k1 = lm.greedy_generate(emb, max_new_tokens=6, stop_ids=(), do_sample=True, top_p=0.9, top_k=1, generator=torch.Generator().manual_seed(7))
    assert lm.last_generate_stats["sampled_rows"] > 0 and torch.equal(k1, greedy)


def test_llama_fullwidth_loss_and_input_grad_vs_golden():
    g = load("llama_fullwidth")
    D, layers, heads, inter, V, seed = [int(x) for x in g["meta"]]
    sd = gu.llama_weights(D, layers, inter, V, seed=seed)
    gen = torch.Generator().manual_seed(int(g["seed"][1]))
    emb = torch.randn(2, 24, D, generator=gen) * 0.02
    lm = LlamaHIP(sd, heads, DEV)
    loss = lm.forward_loss(emb.to(DEV), g["mask"], g["labels"])
    assert abs(loss.item() - g["loss"].item()) < 2e-3 * abs(g["loss"].item())
    demb = lm.backward()
    assert relerr(demb[:, :, ::16], g["demb_sub"]) < 5e-2


def test_llama_tiny_ragged_loss_grad_and_greedy_ids():
    g = load("llama_tiny")
    D, layers, heads, inter, V, seed = [int(x) for x in g["meta"]]
    sd = bf16_round(gu.llama_weights(D, layers, inter, V, seed=seed, std=0.2))
    lm = LlamaHIP(sd, heads, DEV)
    emb = g["emb"]
    loss_ref, _ = R.llama_causal_lm(sd, emb.clone().requires_grad_(True), g["mask"], g["labels"], heads)
    loss = lm.forward_loss(emb.to(DEV), g["mask"], g["labels"])
    assert abs(loss.item() - loss_ref.item()) < 5e-3 * abs(loss_ref.item())
    assert abs(loss.item() - g["loss"].item()) < 3e-2 * abs(g["loss"].item())   # golden used unrounded weights
    e2 = emb.clone().requires_grad_(True)
    R.llama_causal_lm(sd, e2, g["mask"], g["labels"], heads)[0].backward()
    demb = lm.backward()
    # Why this bound is 9e-2 and not the 5e-2 the full-width model is held to (below): at width 64 with std-0.2 weights every
    # layer multiplies the bf16 rounding error of the gradient by ~2.5 (measured, tools/tiny_llama_depth_error.py: the same
    # weights truncated to ONE layer give 2.9e-2 of max-abs / 1.7e-2 Frobenius, the two layers of this fixture 7.5e-2 / 4.1e-2;
    # deterministic).  So the one-layer model is asserted at 4e-2 -- inside the 5e-2 class -- and the two-layer one at 9e-2 =
    # one more factor of 2.5 on 2.9e-2 plus margin; the Frobenius error stays under 5e-2 at both depths.
    assert relerr(demb, e2.grad) < 9e-2
    assert ((demb.cpu() - e2.grad).norm() / e2.grad.norm()).item() < 5e-2
    sd1 = {n: t for n, t in sd.items() if ".layers." not in n or int(n.split(".layers.")[1].split(".")[0]) < 1}
    lm1 = LlamaHIP(sd1, heads, DEV)
    e1 = emb.clone().requires_grad_(True)
    R.llama_causal_lm(sd1, e1, g["mask"], g["labels"], heads)[0].backward()
    lm1.forward_loss(emb.to(DEV), g["mask"], g["labels"])
    d1 = lm1.backward()
    assert relerr(d1, e1.grad) < 4e-2
    assert ((d1.cpu() - e1.grad).norm() / e1.grad.norm()).item() < 2.5e-2
    # greedy decode with KV cache: ids equal to the oracle's wherever its margin is healthy
    with torch.no_grad():
        ids_ref, margins = R.greedy_generate(sd, emb[:2, :7], heads, max_new_tokens=12, stop_ids=((7,),),
                                             return_margins=True)
    ids, mar = lm.greedy_generate(emb[:2, :7].to(DEV), max_new_tokens=12, stop_ids=((7,),), return_margins=True)
    n = min(ids.shape[1], ids_ref.shape[1])
    # compare up to (and including) the first step whose oracle margin is small; after a legitimate tie-flip
    # the sequences diverge by construction
    for t in range(n):
        if float(margins[:, t].min()) < 0.05:
            break
        assert torch.equal(ids[:, t], ids_ref[:, t]), (t, ids, ids_ref)
    else:
        assert ids.shape == ids_ref.shape


# ------------------------------------------------------------------------------------------------ full models
def _composite_sd(seeds):
    sd = {}
    sd.update(gu.vit_weights(1408, 1, 16, int(1408 * 4.3637), 14, 257, seed=seeds[0]))
    sd.update(gu.qformer_weights(768, 2, 3072, 1408, seed=seeds[1]))
    sd.update(gu.llama_weights(4096, 1, 11008, 1000, seed=seeds[2]))
    sd.update(gu.adapter_weights(seed=seeds[3]))
    sd.update(gu.glue_weights(seed=seeds[4]))
    return sd


@pytest.fixture(scope="module")
def composite():
    g = load("composite_fullwidth")
    seeds = [int(x) for x in g["seed"]]
    sd = _composite_sd(seeds)
    batch = gu.synthetic_batch(2, 1000, seed=seeds[5], pad_tail=1)
    return g, sd, batch


def _samples(batch):
    image, maps, before, after, tgt, tmask = batch
    return dict(image=image, anomaly_maps=maps, oneshot_anomaly_maps=maps, before_ids=before, after_ids=after,
                target_ids=tgt, target_mask=tmask)


@pytest.mark.parametrize("arch,stage", [("mini_gpt4", 0), ("myriad", 0), ("myriad", 1), ("myriad", 2)])
def test_composite_step_vs_golden(composite, arch, stage):
    g, sd, batch = composite
    cls = MiniGPT4HIP if arch == "mini_gpt4" else MyriadHIP
    model = cls(sd, dict(fixed_stage=stage, fixed_taskstage=0), device=DEV)
    out = model(_samples(batch))
    key = f"{arch}_s{stage}"
    loss = out["loss"]
    assert abs(loss.item() - g[key + "_loss"].item()) < 3e-3 * abs(g[key + "_loss"].item()), (loss.item(), g[key + "_loss"])
    loss.backward()     # autograd bridge -> explicit HIP backward
    grads = {n: p.grad for n, p in model.named_parameters()}
    if arch == "mini_gpt4":
        assert set(grads) == {"llama_proj.weight", "llama_proj.bias"}
        assert float(grads["llama_proj.weight"].abs().max()) > 0
        return
    assert relerr(grads["expert_adaptor.conv1.weight"], g[key + "_dA"]) < 5e-2
    assert relerr(grads["expert_adaptor.conv2.weight"][::16], g[key + "_dB_sub"]) < 5e-2

    def ref_layout(name, t):
        return t if t.dim() != 2 or "meta_net" not in name else None

    if stage in (1, 2):
        w15 = grads["VEInstructor.meta_net.15.weight"]                     # [768, (ky, kx, ci)]: element by element on a sub-sample
        assert relerr(w15.reshape(w15.shape[0], -1)[::8, ::8], g[key + "_instr_dw15_sub"]) < 5e-2
        assert abs(w15.norm().item() - g[key + "_instr_dw15_norm"].item()) < 5e-2 * g[key + "_instr_dw15_norm"].item()
        # the first stem layers are NOT compared with this fp32-forward golden here: they are held to the reference's own
        # measured bf16 gap (test_stem_gradients_vs_the_fp32_reference_are_bounded_by_its_own_bf16_gap) and to 5e-2 of the
        # bf16-forward reference (test_ve_net_grads_vs_the_reference_run_with_bf16_forward_rounding); the former
        # cosine >= 0.9 / norm +-25 % gate is gone
        assert bool(torch.isfinite(grads["VEInstructor.meta_net.0.weight"]).all())
        assert float(grads["VEInstructor.meta_net.0.weight"].abs().max()) > 0
    else:
        # unused at this prompt stage: no gradient for torch's optimiser (autograd leaves None in the reference), zeros in the flat
        # buffer that the data-parallel exchange sums
        assert grads["VEInstructor.meta_net.15.weight"] is None
        assert float(model.store.g["VEInstructor.meta_net.15.weight"].abs().max()) == 0
    if stage in (0, 1):
        w15 = grads["VETokenizer.meta_net.15.weight"]                      # [4096, (ky, kx, ci)] = 105 M weights
        assert relerr(w15.reshape(w15.shape[0], -1)[::64, ::100], g[key + "_tok_dw15_sub"]) < 5e-2
        assert abs(w15.norm().item() - g[key + "_tok_dw15_norm"].item()) < 5e-2 * g[key + "_tok_dw15_norm"].item()
        assert bool(torch.isfinite(grads["VETokenizer.meta_net.0.weight"]).all())
        assert float(grads["VETokenizer.meta_net.0.weight"].abs().max()) > 0
        assert relerr(grads["VETokenizer.base_prompts"][:, ::64], g[key + "_tok_dbase_sub"]) < 5e-2
    else:
        assert grads["VETokenizer.meta_net.15.weight"] is None
        assert float(model.store.g["VETokenizer.meta_net.15.weight"].abs().max()) == 0


def test_networks_vs_golden():
    g = load("networks_full")
    sd = gu.adapter_weights(seed=int(g["seed"][0]))
    # minimal host: only the adapters are exercised here
    from myriad_amd.myriad import ParamStore
    from myriad_amd.networks import LoraAdaptor, VENet, ve_param_specs
    specs = [("expert_adaptor.conv1.weight", (4, 1408), (4, 1408)), ("expert_adaptor.conv2.weight", (1408, 4), (1408, 4))]
    specs += ve_param_specs("VETokenizer.", 4096, 5) + [("VETokenizer.base_prompts", (9, 4096), (9, 4096))]
    specs += ve_param_specs("VEInstructor.", 768, 1)
    st = ParamStore(specs, DEV)
    for name, ishape, _ in st.specs:
        st.p[name].copy_(from_reference_layout(sd[name].to(DEV), ishape))
    gen = torch.Generator().manual_seed(int(g["seed"][1]))
    x = torch.randn(2, 257, 1408, generator=gen)
    maps = torch.rand(2, 1, 224, 224, generator=gen)
    ct_a = torch.randn(2, 257, 1408, generator=gen)
    ct_i = torch.randn(2, 49, 768, generator=gen)
    ct_t = torch.randn(2, 18, 4096, generator=gen)
    ad = LoraAdaptor(st.p, st.g)
    ins = VENet("VEInstructor.", 1, 768, st.p, st.g, DEV)
    tok = VENet("VETokenizer.", 5, 4096, st.p, st.g, DEV)
    ya = ad.forward(x.view(-1, 1408).to(DEV)).view(2, 257, 1408)
    yi = ins.forward(maps.to(DEV))
    yt = tok.forward(maps.to(DEV))
    assert relerr(ya[:, ::16, ::8], g["adaptor_out_sub"]) < 1e-4
    assert relerr(yi, g["instr_out"]) < 2e-2
    assert relerr(yt[:, :, ::8], g["tok_out_sub"][:, 9:]) < 2e-2
    ad.backward(ct_a.view(-1, 1408).to(DEV))
    ins.backward(ct_i.to(DEV))
    tok.backward(ct_t[:, 9:].contiguous().to(DEV))
    assert relerr(st.g["expert_adaptor.conv1.weight"], g["dA"]) < 1e-3
    assert relerr(st.g["expert_adaptor.conv2.weight"], g["dB"]) < 1e-3
    for nm, pre in (("instr", "VEInstructor."), ("tok", "VETokenizer.")):
        for idx in (0, 3, 6, 9, 12, 15):
            w = st.g[pre + f"meta_net.{idx}.weight"]
            want_norm = g[f"{nm}_dw{idx}_norm"].item()
            if idx in (0, 3):
                # the first two stem layers against an fp32 forward are bounded by the reference's own bf16 gap, measured on
                # matching inputs: test_stem_gradients_vs_the_fp32_reference_are_bounded_by_its_own_bf16_gap (this golden has
                # no bf16-forward twin); against the bf16-forward reference they are held to 5e-2 like every other layer
                continue
            assert abs(w.norm().item() - want_norm) < 5e-2 * want_norm, (nm, idx, w.norm().item(), want_norm)
            # the bias gradients are sums over every position behind the ReLU / arg-max gates and move by 8-14 % of max-abs between
            # an fp32 and a bf16 forward (measured, round 6); they are held to 5e-2 -- every layer, weights and biases -- against
            # the reference run with the bf16 forward rounding (test_ve_net_grads_vs_reference_bf16_forward_golden), not here


class _TwoIdenticalRanks:
    """Stand-in for myriad_amd.runner.DataParallel with world 2 whose peer holds the same gradient: the async
    all-reduce(sum) returns 2*g at wait() time."""
    world = 2
    mode = "allreduce"

    def start(self, flat, n_grad=None):
        self.flat = flat

    def wait(self):
        self.flat.mul_(2.0)

    def allreduce(self, flat, n_grad=None):
        flat.mul_(2.0)


def test_overlapped_update_equals_synchronous_update(composite):
    """Delaying all-reduce + AdamW of step t behind the ViT forward of step t+1 must not change the trajectory."""
    g, sd, batch = composite
    smp = _samples(batch)
    runs = []
    for overlap in (False, True):
        model = MyriadHIP(sd, dict(fixed_stage=1, fixed_taskstage=0), device=DEV)
        dp = _TwoIdenticalRanks()
        losses = [float(model.train_step(smp, lr=1e-3, dp=dp, overlap=overlap)) for _ in range(3)]
        model.finish_update()
        runs.append((losses, model.store.flat_p.clone()))
    assert runs[0][0] == pytest.approx(runs[1][0], rel=1e-6)
    assert relerr(runs[1][1], runs[0][1]) < 1e-6
    assert runs[0][0][2] < runs[0][0][0]


class _TwoIdenticalRanksSegmented(_TwoIdenticalRanks):
    """The same stand-in with runner.DataParallel's segment interface: records WHEN each piece of the buffer is started (what
    the launch thread had queued by then and on which stream) and doubles the pieces at wait() time."""

    def __init__(self, log):
        self.log, self._segs, self._total, self._started, self._parts = log, None, None, set(), []

    def set_segments(self, total, cuts):
        pts = [0] + sorted(c for c in cuts if 0 < c < total) + [total]
        self._segs, self._total = [(a, b) for a, b in zip(pts[:-1], pts[1:]) if b > a], total

    def segments(self, total):
        return self._segs if self._segs is not None else [(0, total)]

    def start_part(self, flat, n_grad, k):
        lo, hi = self.segments(n_grad)[k]
        ev = torch.cuda.Event()
        ev.record()                                   # ordered behind what the CALLING stream has queued: the collective's producer event
        self.log.append(("part", k, (lo, hi), torch.cuda.current_stream().cuda_stream, ev))
        self._started.add(k)
        self._parts.append((flat, lo, hi, ev))

    def start(self, flat, n_grad=None):
        self.log.append(("rest", sorted(self._started)))
        for k, (lo, hi) in enumerate(self.segments(n_grad)):
            if k not in self._started:
                self._parts.append((flat, lo, hi, None))
        self._parts.append((flat, n_grad, flat.numel(), None))   # the use flags
        self._started = set()

    def wait(self):
        for flat, lo, hi, ev in self._parts:
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)
            flat[lo:hi].mul_(2.0)
        self._parts = []


def test_tokenizer_segment_exchange_starts_inside_the_backward_before_the_qformer(composite):
    """VERDICT r5 item 2 (runner_base.py:94-98: DDP overlaps its bucketed all-reduce with the backward).  With a segment-aware
    exchange object train_step cuts the gradient buffer at the map tokenizer's conv-head weights (>= 90 % of the trainable bytes,
    cut points multiples of 32 elements so that 2 / 4 / 8-rank reduce-scatters tile every segment) and starts THAT segment from
    inside the backward: after the tokenizer's own backward, on the stream that ran it (the leaf stream), BEFORE the first launch
    of the Q-Former backward -- the rest (+ the use flags) follows when the whole backward is queued.  At a prompt stage that skips
    the tokenizer the segment's zeros still travel at the same point (every rank issues the same collectives).  The trajectory is
    the synchronous one."""
    g, sd, batch = composite
    smp = _samples(batch)
    runs = []
    for segmented in (False, True):
        log = []
        model = MyriadHIP(sd, dict(fixed_stage=1, fixed_taskstage=0), device=DEV)
        dp = _TwoIdenticalRanksSegmented(log) if segmented else _TwoIdenticalRanks()
        orig_qb, orig_tb = model.qformer.backward, model.ve_tok.backward
        model.qformer.backward = lambda *a, **k: (log.append(("qformer.backward",)), orig_qb(*a, **k))[1]
        model.ve_tok.backward = lambda *a, **k: (log.append(("ve_tok.backward", torch.cuda.current_stream().cuda_stream)), orig_tb(*a, **k))[1]
        losses = []
        for i, stage in enumerate((1, 2, 1)):                       # step 1: stage 2 = the tokenizer is unused on this rank
            model.fixed_stage = stage
            losses.append(float(model.train_step(smp, lr=1e-3, dp=dp, overlap=segmented)))
        model.finish_update()
        runs.append((losses, model.store.flat_p.clone(), log))
    assert runs[0][0] == pytest.approx(runs[1][0], rel=1e-6)
    assert relerr(runs[1][1], runs[0][1]) < 1e-6
    log = runs[1][2]
    names = [e[0] for e in log]
    assert names == ["ve_tok.backward", "part", "qformer.backward", "rest",          # stage 1
                     "part", "qformer.backward", "rest",                             # stage 2: no tokenizer backward, same collectives
                     "ve_tok.backward", "part", "qformer.backward", "rest"], names
    st = model.store
    a, b = st.module_range("VETokenizer", True)
    for e in log:
        if e[0] == "part":
            lo, hi = e[2]
            assert e[1] == 1 and a <= lo < hi <= b and lo % 32 == 0 and hi % 32 == 0 and st.total % 32 == 0
            assert hi - lo >= 0.9 * st.n_params()
        if e[0] == "rest":
            assert e[1] == [1]
    # issued on the stream that ran the tokenizer's backward (its gradient is complete THERE, not yet on the main stream)
    assert log[1][3] == log[0][1] and log[1][3] != torch.cuda.current_stream().cuda_stream


def test_flat_logit_decode_ids_equal_up_to_the_first_two_ulp_near_tie():
    """VERDICT r3 item 8b.  A FLAT fixture (random std-0.2 weights, V = 320: top-1 probability ~ 1 %) is where greedy ids are
    fragile, so the gate is stated in the arithmetic's own unit: ids must be equal at every step before the first one whose
    ORACLE top-1 / top-2 margin is below two bf16 ulps of that step's logit scale (2 * 2^-7 * max|logit|; a bf16 lm_head
    operand cannot resolve less), per prompt, single-row batches so one prompt's near-tie does not end another's comparison.
    Nine prompts (3 rows x 3 prefix lengths, 40 new tokens): the oracle's margins admit 65 comparable steps in total (13 on the
    longest run) -- asserted, so the test cannot pass on `checked >= 1`."""
    g = load("llama_tiny")
    D, layers, heads, inter, V, seed = [int(x) for x in g["meta"]]
    sd = bf16_round(gu.llama_weights(D, layers, inter, V, seed=seed, std=0.2))
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    emb = g["emb"]
    checked, longest = 0, 0
    for r in range(emb.shape[0]):
        for s0 in (5, 7, 9):
            with torch.no_grad():
                ids_ref, margins, scales = R.greedy_generate(sd, emb[r:r + 1, :s0], heads, max_new_tokens=40, stop_ids=(), return_scales=True)
            ids = lm.greedy_generate(emb[r:r + 1, :s0].to(DEV), max_new_tokens=40, stop_ids=())
            near = (margins < 2.0 * 2.0 ** -7 * scales).any(0)
            first = int(near.nonzero()[0]) if bool(near.any()) else ids_ref.shape[1]
            assert ids.shape[1] >= first, (r, s0, ids.shape, first)
            assert torch.equal(ids[:, :first].cpu(), ids_ref[:, :first]), (r, s0, first, ids[:, :first + 1], ids_ref[:, :first + 1], margins[:, :first + 1])
            checked += first
            longest = max(longest, first)
    assert checked >= 60 and longest >= 12, (checked, longest)


def test_myriad_generate_output_schema_and_determinism(composite):
    """`Myriad.generate` on the flat random-weight composite model: the output dict the evaluation script reads
    (evaluation_aqa_dataset.py:339-387: token ids, the text field, the anomaly map handed through), its shapes, and the same ids
    from a second call (KV-cache workspace and captured graph reused).  WHICH ids come out is pinned elsewhere, with no margin
    gate: every id of the full pipeline on the peaked fixture (test_myriad_generate_every_id_equals_the_reference_pipeline,
    below) and every id up to the first two-ulp near-tie on flat logits (test_flat_logit_decode_ids_equal_up_to_...).  (Until
    round 5 this test compared ids with the oracle while its top-2 margin stayed >= 0.1 and passed on one compared step.)"""
    g, sd, batch = composite
    image, maps, before, after, tgt, tmask = batch
    model = MyriadHIP(sd, dict(need_backward=False), device=DEV)
    model.eval()
    smp = dict(image=image, anomaly_maps=maps, before_ids=before, after_ids=after)
    out = model.generate(smp, max_new_tokens=10, stop_ids=((5,),), min_length=1)
    ids = out["token_ids"]
    assert out["ve_anomaly_maps"].shape == maps.shape
    assert ids.dim() == 2 and ids.shape[0] == image.shape[0] and 1 <= ids.shape[1] <= 10 and ids.dtype == torch.long
    assert int(ids.min()) >= 0 and int(ids.max()) < sd["llama_model.lm_head.weight"].shape[0]
    again = model.generate(smp, max_new_tokens=10, stop_ids=((5,),), min_length=1)["token_ids"]
    assert torch.equal(ids, again)
    # the first id of the sequence is the arg-max of the prefill's last logits: compare it with the oracle's when the oracle
    # itself is decided by more than two bf16 ulps of its logit scale (else either id is a correct bf16 answer)
    with torch.no_grad():
        img = R.encode_img(sd, image, maps, 1, "myriad")
        ew = sd["llama_model.model.embed_tokens.weight"]
        wrapped = torch.cat([ew[before], img, ew[after]], 1)
        ids_ref, margins = R.greedy_generate(sd, wrapped, 32, max_new_tokens=1, stop_ids=((5,),), return_margins=True)
    for b in range(ids.shape[0]):
        if float(margins[b, 0]) >= 0.1:
            assert int(ids[b, 0]) == int(ids_ref[b, 0]), (b, ids, ids_ref, margins)


@pytest.mark.parametrize("sampled", [False, True])
def test_myriad_generate_every_id_equals_the_reference_pipeline(sampled):
    """The FULL `Myriad.generate` (myriad.py:433-454: ViT -> adaptor -> ln_vision -> Q-Former with the VEInstructor queries
    -> llama_proj + VETokenizer tokens -> prompt_wrap without BOS -> prefill -> KV-cache decode) on the peaked pipeline
    fixture made by the reference's own modules (tests/golden/pipeline_chain.npz, tools/make_golden.py:case_pipeline_chain).
    The four rows share one prompt: the FIRST generated id of each row is decided by its image alone.  EVERY id must be
    equal -- no margin gate -- at batch 4 (row-0 stop rule on [2277, 29937] after 33 tokens, a row finishing early on EOS,
    a row emitting 835 without stopping), at batch 1, and for row 3 alone (where [835] does stop the call)."""
    g = load("pipeline_chain")
    sd = gu.pipeline_chain_weights(g["probe"])
    image, maps, before, after = gu.pipeline_chain_batch()
    model = MyriadHIP(sd, dict(need_backward=False), device=DEV)
    model.eval()
    kw = dict(do_sample=True, top_p=0.01, temperature=1.0) if sampled else {}
    stops = ((835,), (2277, 29937))
    for name, sel in (("b4", [0, 1, 2, 3]), ("b1", [0]), ("b1r3", [3])):
        smp = dict(image=image[sel], anomaly_maps=maps[sel], before_ids=before[sel], after_ids=after[sel])
        out = model.generate(smp, max_new_tokens=90, stop_ids=stops, min_length=1, **kw)
        ids = out["token_ids"].cpu()
        assert torch.equal(ids, g[name + "_ids"]), (name, ids, g[name + "_ids"])
        st = model.last_generate_stats
        assert st["steps"] == ids.shape[1] and st["sampled_rows"] == 0
        if sampled:
            assert st["min_pmax"] >= 0.5
    assert g["b4_ids"][:, 0].tolist() == [100, 200, 300, 400]           # one first id per image


def test_train_step_moves_parameters_like_adamw(composite):
    g, sd, batch = composite
    model = MyriadHIP(sd, dict(fixed_stage=1, fixed_taskstage=0), device=DEV)
    p0 = model.store.flat_p.clone()
    loss0 = model.train_step(_samples(batch), lr=1e-3)
    gflat = model.store.flat_g.clone()
    # AdamW first step: p1 = p0*(1-lr*wd) - lr*sign-ish(g) ; check against the oracle formula on the flat buffer
    a = model.store.n_wd
    p_ref = p0.cpu().clone()
    m, v = torch.zeros_like(p_ref), torch.zeros_like(p_ref)
    R.adamw_step(p_ref[:a], gflat.cpu()[:a], m[:a], v[:a], 1, 1e-3, 0.05)
    R.adamw_step(p_ref[a:], gflat.cpu()[a:], m[a:], v[a:], 1, 1e-3, 0.0)
    assert relerr(model.store.flat_p, p_ref) < 1e-5
    # ... and elementwise: float64 torch.optim.AdamW on the two groups, within the budgets of tests/adamw_ref.py
    from tests.adamw_ref import AdamWRef
    ref = AdamWRef([p0[:a], p0[a:]], [0.05, 0.0])
    ref.step([gflat[:a], gflat[a:]], 1e-3)
    st = model.store
    ref.check(0, st.flat_p[:a], st.flat_m[:a], st.flat_v[:a], "decay group")
    ref.check(1, st.flat_p[a:], st.flat_m[a:], st.flat_v[a:], "no-decay group")
    loss1 = model.train_step(_samples(batch), lr=1e-3)
    assert float(loss1) < float(loss0)      # same batch, one AdamW step => loss goes down


@pytest.mark.parametrize("accum,beta2", [(1, 0.999), (2, 0.999), (1, 0.98)])
def test_training_trajectory_replays_on_float64_torch_adamw(accum, beta2):
    """The default train_step path (the map tokenizer's AdamW early on the leaf stream, the rest at the tail, look-ahead ViT) of
    the reduced-depth full-width LoRA model, replayed on the optimiser the reference builds: float64 torch.optim.AdamW, one
    parameter per module range of the flat buffer in the reference's two groups, fed after every update the gradients and use
    flags the step left in flat_g_comm (.grad None for a module no call of the window used) and that update's lr.
    VEInstructor is unused in the first two steps (its first update is its own step 1 at a later global step), VETokenizer in a
    later one; with accum_grad_iters = 2 the window's summed buffer is replayed at the due calls only.  p, m and v within the
    budgets of tests/adamw_ref.py, per-module step counts equal torch's, the padding tail stays zero.  After every step the LoRA
    borders of W_ext and W_ext^T hold, in every border group, bf16 of the B_q / B_v that step's forward read; the k rows' border
    stays zero and the frozen block keeps its bits."""
    from myriad_amd.lora import BORDER
    from tests import dp_common as C
    from tests.adamw_ref import AdamWRef
    dev = torch.device(DEV)
    model, cfg = C.build_model(dev)
    model.lora.base_seed = 11
    st, lora, layers = model.store, model.lora, model.llama.layers
    for name, _, rshape in st.specs:
        o, n = st.offsets[name]
        assert [d for _, a, b, d in st.ranges if a <= o and o + n <= b] == [R.uses_weight_decay(name, len(rshape))], name
    stages = [0, 0, 1, 2, 1, 0] if accum == 1 else [0, 0, 0, 1, 2, 2, 1, 0]
    lrs = [1e-3, 7e-4, 1.2e-3, 5e-4, 9e-4, 3e-4, 8e-4, 6e-4][:len(stages)]
    batches = [C.batch(0, i, cfg["vocab"], dev) for i in range(len(stages))]
    torch.cuda.synchronize()
    ref = AdamWRef([st.flat_p[a:b] for _, a, b, _ in st.ranges], [0.05 if d else 0.0 for _, _, _, d in st.ranges], beta2)
    D, r = lora.D, lora.r
    W = D
    frozen = [(L["wqkv_ext"][:, :D].clone(), L["wqkvT_ext"][:D].clone()) for L in layers]
    for i, stage in enumerate(stages):
        torch.cuda.synchronize()
        b_read = [(lora.P[lora.names(li)[2]].clone(), lora.P[lora.names(li)[3]].clone()) for li in range(len(layers))]
        model.fixed_stage = stage
        model.train_step(batches[i], lrs[i], 0.05, next_samples=batches[i + 1] if i + 1 < len(stages) else None,
                         accum_grad_iters=accum, beta2=beta2)
        torch.cuda.synchronize()
        for li, L in enumerate(layers):
            bq, bv = (t.view(W, r).to(torch.bfloat16) for t in b_read[li])
            want = torch.zeros(3 * W, BORDER, dtype=torch.bfloat16, device=dev)
            for grp in range(BORDER // (2 * r)):
                want[:W, grp * 2 * r:grp * 2 * r + r] = bq
                want[2 * W:, grp * 2 * r + r:(grp + 1) * 2 * r] = bv
            assert torch.equal(L["wqkv_ext"][:, D:], want), (i, li)
            assert torch.equal(L["wqkvT_ext"][D:], want.T), (i, li)
            assert torch.equal(L["wqkv_ext"][:, :D], frozen[li][0]) and torch.equal(L["wqkvT_ext"][:D], frozen[li][1]), (i, li)
        if (i + 1) % accum:
            continue
        gc = st.flat_g_comm.clone()
        used = gc[st.total:st.total + len(st.modules)].cpu()
        ref.step([gc[a:b] if float(used[mi]) > 0 else None for mi, a, b, _ in st.ranges], lrs[i])
        for k, (mi, a, b, _) in enumerate(st.ranges):
            ref.check(k, st.flat_p[a:b], st.flat_m[a:b], st.flat_v[a:b], f"call {i} {st.modules[mi]}")
        assert st.module_steps() == {st.modules[mi]: ref.steps(k) for k, (mi, _, _, _) in enumerate(st.ranges)}, i
        for t in (st.flat_p, st.flat_m, st.flat_v):
            assert int(torch.count_nonzero(t[st.n_used:])) == 0
    n_upd = len(stages) // accum
    want_steps = {"expert_adaptor": n_upd, "lora": n_upd, "VEInstructor": n_upd - (3 if accum == 1 else 1),
                  "VETokenizer": n_upd - 1}
    assert st.module_steps() == want_steps


def _store_state(st):
    return [t.clone() for t in (st.flat_p, st.flat_m, st.flat_v, st.steps_dev)]


def _store_load(st, state):
    for t, s0 in zip((st.flat_p, st.flat_m, st.flat_v, st.steps_dev), state):
        t.copy_(s0)


@pytest.mark.parametrize("gscale,beta2", [(1.0, 0.999), (0.5, 0.98)])
def test_param_store_splits_of_one_update_give_the_one_shot_bits(gscale, beta2):
    """ParamStore bookkeeping.  One update of a store holding all four module kinds (odd-sized tensors: padding inside the ranges;
    VEInstructor unused; counters at different steps) done as adamw_pieces + adamw_step(exclude=...), as adamw_module +
    adamw_step(skip=...), and as per-rank `shard` lists (each rank from the same state: its own counters) gives the bits of the
    one-shot adamw_step -- cut points inside a module range, on range boundaries, spanning two modules, empty pieces, and a
    piece over the padding tail, which never changes.  The one-shot update itself is float64 torch.optim.AdamW with the
    reference's grouping (oracle.uses_weight_decay per parameter, tests/adamw_ref.py budgets), and every range's decay flag is
    that grouping."""
    from myriad_amd.lora import lora_param_specs
    from myriad_amd.myriad import ParamStore, module_of
    from myriad_amd.networks import ve_param_specs
    from tests.adamw_ref import AdamWRef
    specs = ([("expert_adaptor.conv1.weight", (4, 37), (4, 37)), ("expert_adaptor.conv2.weight", (37, 4), (37, 4))]
             + ve_param_specs("VETokenizer.", 8, 5) + [("VETokenizer.base_prompts", (9, 33), (9, 33))]
             + ve_param_specs("VEInstructor.", 12, 1) + lora_param_specs(2, 36, 3))
    st = ParamStore(specs, DEV)
    for name, _, rshape in st.specs:
        o, n = st.offsets[name]
        dec = [d for _, a, b, d in st.ranges if a <= o and o + n <= b]
        assert dec == [R.uses_weight_decay(name, len(rshape))], name
    gen = torch.Generator(device=DEV).manual_seed(5)
    st.flat_p.copy_(torch.randn(st.total, generator=gen, device=DEV))
    st.flat_m.copy_(torch.randn(st.total, generator=gen, device=DEV) * 0.1)
    st.flat_v.copy_(torch.rand(st.total, generator=gen, device=DEV) * 0.01)
    st.flat_g.copy_(torch.randn(st.total, generator=gen, device=DEV))
    flags = {"expert_adaptor": 2.0, "VETokenizer": 1.0, "VEInstructor": 0.0, "lora": 2.0}
    st.used.copy_(torch.tensor([flags[m] for m in st.modules], device=DEV))
    st.set_module_steps({"expert_adaptor": 3, "VETokenizer": 0, "VEInstructor": 2, "lora": 7})
    assert st.n_used < st.total                                   # a padding tail exists: it must never change
    s0 = _store_state(st)
    lr = 7e-4
    st.adamw_step(lr, 0.05, beta2=beta2, grad_scale=gscale)
    s1 = _store_state(st)
    torch.cuda.synchronize()
    assert all(torch.equal(a[st.n_used:], b[st.n_used:]) for a, b in zip(s0[:3], s1[:3]))

    # the one-shot update is torch's, per parameter, with the reference's weight-decay grouping
    names = [n for n, _, _ in st.specs]
    sl = lambda t, n: t[st.offsets[n][0]:st.offsets[n][0] + st.offsets[n][1]]
    ref = AdamWRef([sl(s0[0], n) for n in names],
                   [0.05 if R.uses_weight_decay(n, len(r)) else 0.0 for n, _, r in st.specs], beta2)
    before = {"expert_adaptor": 3, "VETokenizer": 0, "VEInstructor": 2, "lora": 7}
    for i, n in enumerate(names):                                # the moments the store holds, at each module's step count
        ref.seed_state(i, before[module_of(n)], sl(s0[1], n), sl(s0[2], n))
    ref.step([sl(st.flat_g, n) * gscale if flags[module_of(n)] > 0 else None for n in names], lr)
    for i, n in enumerate(names):
        ref.check(i, sl(s1[0], n), sl(s1[1], n), sl(s1[2], n), n)
    assert st.module_steps() == {m: before[m] + (flags[m] > 0) for m in st.modules}

    def same(what):
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(zip(_store_state(st), s1)):
            assert torch.equal(a, b), (what, ("p", "m", "v", "steps")[k])

    rg = {st.modules[mi] + ("" if d else "/nd"): (a, b) for mi, a, b, d in st.ranges}
    ta, tb = rg["VETokenizer"]
    ea, eb = rg["expert_adaptor"]
    inside = (ta + 40, ta + 1000)                                 # inside one module range
    whole = rg["lora"]                                            # exactly one range
    span = (eb - 8, ta + 16)                                      # across the boundary of two modules
    tail = (st.n_used // 4 * 4, st.total)                         # over the padding tail
    for pieces in ([inside], [whole], [span], [(ta + 4, ta + 4)], [tail],
                   [span, (ta + 200, ta + 200), inside, whole, rg["VEInstructor/nd"], tail]):
        _store_load(st, s0)
        st.adamw_pieces(pieces, lr, 0.05, beta2=beta2, grad_scale=gscale)
        st.adamw_step(lr, 0.05, beta2=beta2, grad_scale=gscale, exclude=pieces)
        same(pieces)
    if gscale == 1.0:                                             # adamw_module: the single-process early update (no scale)
        for m in st.modules:
            _store_load(st, s0)
            st.adamw_module(m, lr, 0.05, beta2=beta2)
            st.adamw_step(lr, 0.05, beta2=beta2, skip={m})
            same(m)
    for world in (2, 4):                                          # rs_ag: every rank updates its own slices, from the same state
        cut = ta + 32 * 8
        segs = [(0, cut), (cut, st.total)]
        per_rank = []
        for r in range(world):
            mine = []
            for lo, hi in segs:
                per = -(-(hi - lo) // world)
                per = (per + 3) // 4 * 4
                a = min(lo + r * per, hi)
                mine.append((a, min(a + per, hi)))
            per_rank.append(mine)
        _store_load(st, s0)
        for mine in per_rank:
            st.steps_dev.copy_(s0[3])
            st.adamw_step(lr, 0.05, beta2=beta2, grad_scale=gscale, shard=mine)
        same(("shards", world))
        assert not st.moments_complete
    _store_load(st, s0)
    st.adamw_step(lr, 0.05, beta2=beta2, grad_scale=gscale, shard=(0, st.total))
    same("one shard tuple")


def test_ve_net_grads_vs_reference_bf16_forward_golden():
    """Every conv gradient of both VE nets, first stem layers included, within 5e-2 of a committed golden made by the
    REFERENCE's modules (networks.py:95-197) with their forward rounded to bf16 where the HIP path stores bf16
    (tools/make_golden.py case_networks_bf16): same gates on both sides, so the cancelling sums compare tightly."""
    from myriad_amd.myriad import ParamStore
    from myriad_amd.networks import VENet, ve_param_specs
    g = load("networks_bf16fwd")
    sd = gu.adapter_weights(seed=int(g["seed"][0]))
    gen = torch.Generator().manual_seed(int(g["seed"][1]))
    maps = torch.rand(2, 1, 224, 224, generator=gen).to(DEV)
    ct_i = torch.randn(2, 49, 768, generator=gen).to(DEV)
    ct_t = torch.randn(2, 18, 4096, generator=gen).to(DEV)
    for nm, pre, k_last, dim, ct in (("instr", "VEInstructor.", 1, 768, ct_i), ("tok", "VETokenizer.", 5, 4096, ct_t[:, 9:].contiguous())):
        st = ParamStore(ve_param_specs(pre, dim, k_last), DEV)
        for name, ishape, _ in st.specs:
            st.p[name].copy_(from_reference_layout(sd[name].to(DEV), ishape))
        net = VENet(pre, k_last, dim, st.p, st.g, DEV)
        out = net.forward(maps)
        want_out = g["instr_out"] if nm == "instr" else g["tok_out_sub"]
        assert relerr(out if nm == "instr" else out[:, :, ::8], want_out) < 2e-3, nm
        net.backward(ct)
        for idx in (0, 3, 6, 9, 12, 15):
            w = st.g[pre + f"meta_net.{idx}.weight"]
            want = torch.as_tensor(g[f"{nm}_dw{idx}"])
            if want.numel() != w.numel():
                w = w[:: max(1, w.shape[0] // 16), :: max(1, w.shape[1] // 64)]
            e_w = relerr(w, want)
            e_b = relerr(st.g[pre + f"meta_net.{idx}.bias"], g[f"{nm}_db{idx}"])
            e_n = abs(st.g[pre + f"meta_net.{idx}.weight"].norm().item() / g[f"{nm}_dw{idx}_norm"].item() - 1.0)
            print(f"{nm} conv{idx}: dW {e_w:.3e} db {e_b:.3e} |dW| {e_n:.3e}")
            assert e_w <= 5e-2 and e_b <= 5e-2 and e_n <= 5e-2, (nm, idx, e_w, e_b, e_n)


def test_stem_gradients_vs_the_fp32_reference_are_bounded_by_its_own_bf16_gap():
    """VERDICT r3 item 8a.  Against the reference's plain fp32 forward the first two stem layers' gradients cannot be tight:
    they are cancelling sums over ~1e5 positions behind five ReLU / arg-max layers, and a bf16 forward takes a few gates
    differently.  The golden now measures that on the REFERENCE alone (tools/make_golden.py case_networks_bf16, same modules,
    inputs and cotangents run twice): 0.02-1.7 % of the gates flip (per layer) and the reference's own stem gradients move by 7-33 %
    (relative L2; `*_gap{idx}`, `*_gate_flip_frac`).  The HIP path is within 5e-2 of the bf16-forward reference
    (test_ve_net_grads_vs_the_reference_run_with_bf16_forward_rounding), so against the fp32 reference it must satisfy the
    triangle bound  |g_hip - g_fp32| <= gap + 5e-2; measured: it sits within 0.01 of the gap itself, asserted at gap + 2e-2 -- this replaces the former cosine >= 0.9 / norm +-25 % check."""
    from myriad_amd.myriad import ParamStore
    from myriad_amd.networks import VENet, ve_param_specs
    g = load("networks_bf16fwd")
    sd = gu.adapter_weights(seed=int(g["seed"][0]))
    gen = torch.Generator().manual_seed(int(g["seed"][1]))
    maps = torch.rand(2, 1, 224, 224, generator=gen).to(DEV)
    ct_i = torch.randn(2, 49, 768, generator=gen).to(DEV)
    ct_t = torch.randn(2, 18, 4096, generator=gen).to(DEV)
    for nm, pre, k_last, dim, ct in (("instr", "VEInstructor.", 1, 768, ct_i), ("tok", "VETokenizer.", 5, 4096, ct_t[:, 9:].contiguous())):
        flips = g[f"{nm}_gate_flip_frac"]
        assert 0 < flips.max() < 0.03, flips                     # 0.02 % (first ReLU) .. 1.7 % (last arg-max) of the gates: what the gap is made of
        st = ParamStore(ve_param_specs(pre, dim, k_last), DEV)
        for name, ishape, _ in st.specs:
            st.p[name].copy_(from_reference_layout(sd[name].to(DEV), ishape))
        net = VENet(pre, k_last, dim, st.p, st.g, DEV)
        net.forward(maps)
        net.backward(ct)
        for idx in (0, 3):
            gap_w, gap_b = (float(v) for v in g[f"{nm}_gap{idx}"])
            w = st.g[pre + f"meta_net.{idx}.weight"].float().cpu()
            b = st.g[pre + f"meta_net.{idx}.bias"].float().cpu()
            w32, b32 = torch.as_tensor(g[f"{nm}_dw{idx}_fp32"]), torch.as_tensor(g[f"{nm}_db{idx}_fp32"])
            e_w = float((w.reshape(w32.shape) - w32).norm() / w32.norm())
            e_b = float((b[:b32.numel()] - b32).norm() / b32.norm())
            print(f"{nm} conv{idx}: vs fp32 reference dW {e_w:.3f} (reference's own bf16 gap {gap_w:.3f})  db {e_b:.3f} ({gap_b:.3f})")
            assert e_w <= gap_w + 2e-2 and e_b <= gap_b + 2e-2, (nm, idx, e_w, gap_w, e_b, gap_b)     # measured excess <= 0.010


def test_ve_net_grads_vs_bf16_forward_emulation():
    """Separates arithmetic error from forward-discontinuity sensitivity: an fp32 torch model whose FORWARD rounds
    activations/weights to bf16 at the same points as the HIP path (straight-through in backward) must agree with
    the HIP gradients tightly, including the first stem layer."""
    import torch.nn.functional as F
    from myriad_amd.myriad import ParamStore
    from myriad_amd.networks import VENet, ve_param_specs

    def ste(x):   # bf16 rounding, identity gradient
        return x + (x.to(torch.bfloat16).float() - x).detach()

    sd = gu.adapter_weights(seed=77, with_tokenizer=False)
    specs = ve_param_specs("VEInstructor.", 768, 1)
    st = ParamStore(specs, DEV)
    for name, ishape, _ in st.specs:
        st.p[name].copy_(from_reference_layout(sd[name].to(DEV), ishape))
    gen = torch.Generator().manual_seed(5)
    maps = torch.rand(2, 1, 224, 224, generator=gen).to(DEV)
    ct = torch.randn(2, 49, 768, generator=gen).to(DEV)
    net = VENet("VEInstructor.", 1, 768, st.p, st.g, DEV)
    out = net.forward(maps)
    net.backward(ct)
    prm = {k: v.to(DEV).clone().requires_grad_(True) for k, v in sd.items() if k.startswith("VEInstructor.")}
    x = ste(maps)
    for idx in (0, 3, 6, 9, 12):
        y = F.conv2d(x, ste(prm[f"VEInstructor.meta_net.{idx}.weight"]), ste(prm[f"VEInstructor.meta_net.{idx}.bias"]), padding=1)
        x = ste(F.max_pool2d(F.relu(y), 2))
    y = F.conv2d(x, ste(prm["VEInstructor.meta_net.15.weight"]), prm["VEInstructor.meta_net.15.bias"])
    ref = y.reshape(2, 768, 49).transpose(-2, -1)
    assert relerr(out, ref) < 2e-3
    (ref * ct).sum().backward()
    for idx, (ci, co) in zip((0, 3, 6, 9, 12), [(1, 4), (4, 16), (16, 64), (64, 256), (256, 1024)]):
        want = prm[f"VEInstructor.meta_net.{idx}.weight"].grad.permute(0, 2, 3, 1).reshape(co, 9 * ci)
        got = st.g[f"VEInstructor.meta_net.{idx}.weight"]
        assert cos_sim(got, want) > 0.995 and relerr(got, want) < 6e-2, (idx, cos_sim(got, want), relerr(got, want))
        assert relerr(st.g[f"VEInstructor.meta_net.{idx}.bias"], prm[f"VEInstructor.meta_net.{idx}.bias"].grad) < 6e-2, idx


# ------------------------------------------------------------------------------------------------ PEFT LoRA (a-14)
def test_lora_backward_fused_with_the_qkv_dgrad_is_bit_identical():
    """mh_gemm_lora_dx (split-K slabs summed inside the LoRA dx kernel, border kept for the weight gradients) against the
    two-call form gemm(out f32) + mh_lora_dx + mh_lora_wgrad: same dxn, same dA / dB, bit for bit, at the training shape."""
    from myriad_amd.lora import BORDER, LoraQV, lora_param_specs
    from myriad_amd.myriad import ParamStore
    ops.ensure_workspace(torch.device(DEV))
    D, r, M = 4096, 8, 1184
    assert ops.gemm_plan(M, D + BORDER, 3 * D)[1] > 1          # the policy splits K here: the slab path is what runs
    gen = torch.Generator().manual_seed(77)
    outs = []
    for fused in (False, True):
        st = ParamStore(lora_param_specs(1, D, r), DEV)
        g2 = torch.Generator().manual_seed(78)
        for name, ishape, _ in st.specs:
            st.p[name].copy_(torch.randn(ishape, generator=g2) * 0.05)
        lora = LoraQV(1, D, r, 16.0, 0.05, st.p, st.g, DEV)
        gen.manual_seed(79)
        dqkv = (torch.randn(M, 3 * D, generator=gen) * 0.02).to(DEV).to(torch.bfloat16)
        wT = (torch.randn(D + BORDER, 3 * D, generator=gen) * 0.02).to(DEV).to(torch.bfloat16)
        x_ext = (torch.randn(M, D + BORDER, generator=gen) * 0.5).to(DEV).to(torch.bfloat16)
        seed = 123456789
        if fused:
            dxn = lora.backward_from_dqkv(0, dqkv, wT, x_ext, 0.05, seed)
        else:
            dx_ext = ops.gemm(dqkv, wT, out_dtype=torch.float32)
            dxn = lora.backward(0, dx_ext, dqkv, x_ext, 0.05, seed)
        torch.cuda.synchronize()
        outs.append((dxn.clone(), st.flat_g.clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1]) and float(outs[0][1].abs().sum()) > 0


@pytest.mark.parametrize("M", [1, 2, 3])
def test_decode_norm_and_lora_down_in_one_launch_are_bit_identical(M):
    """mh_rmsnorm_lora_down (LoraQV.norm_border): the RMSNorm of <= 2 residual rows and their LoRA border in one launch -- every
    workgroup rebuilds the rows in rmsnorm_fwd_kernel's order -- against mh_rmsnorm_fwd + mh_lora_down: same x_ext, bit for bit;
    three rows are refused (the caller runs the two launches)."""
    from myriad_amd.lora import BORDER, LoraQV, lora_param_specs
    from myriad_amd.myriad import ParamStore
    D, r = 4096, 8
    st = ParamStore(lora_param_specs(1, D, r), DEV)
    g2 = torch.Generator().manual_seed(91)
    for name, ishape, _ in st.specs:
        st.p[name].copy_(torch.randn(ishape, generator=g2) * 0.05)
    lora = LoraQV(1, D, r, 16.0, 0.05, st.p, st.g, DEV)
    h = (torch.randn(M, D, generator=g2) * 1.3).to(DEV)
    w = (1 + 0.1 * torch.randn(D, generator=g2)).to(DEV)
    want = torch.zeros(M, D + BORDER, dtype=torch.bfloat16, device=DEV)
    ops.rmsnorm_fwd(h, w, 1e-6, out=want[:, :D])
    lora.forward_border(0, want, training=False)
    got = torch.full((M, D + BORDER), 7.0, dtype=torch.bfloat16, device=DEV)
    ok = lora.norm_border(0, h, w, 1e-6, got)
    torch.cuda.synchronize()
    if M > 2:
        assert not ok and float((got - 7.0).abs().max()) == 0
        return
    assert ok and torch.equal(got, want) and float(want[:, D:].float().abs().sum()) > 0


@pytest.mark.parametrize("M,p", [(1184, 0.05), (1184, 0.0), (148, 0.05), (37, 0.05), (5, 0.05)])
def test_lora_weight_gradients_as_mfma_products(M, p):
    """mh_lora_wgrad's MFMA kernel (option lora_wgrad_mfma, the default at r = 8) against the thread-per-column kernel it replaces
    and against float64 sums over the regenerated keep masks.  The MFMA form rounds nothing but the per-row scalars, and those to
    a bf16 head + bf16 remainder (~2^-16): the two kernels agree to 2e-5 of the gradient's scale, both to 1e-4 of float64's."""
    from myriad_amd import _lib as L
    from myriad_amd.lora import BORDER, V_TAG, LoraQV, lora_param_specs
    from myriad_amd.myriad import ParamStore
    D, r, s = 4096, 8, 2.0
    gen = torch.Generator().manual_seed(177)
    dqkv = (torch.randn(M, 3 * D, generator=gen) * 0.02).to(DEV).to(torch.bfloat16)
    x_ext = (torch.randn(M, D + BORDER, generator=gen) * 0.5).to(DEV).to(torch.bfloat16)
    dx_ext = (torch.randn(M, D + BORDER, generator=gen) * 0.1).to(DEV)
    seed = 987654321
    outs = {}
    for mfma in (0, 1):
        L.load().mh_set_option(b"lora_wgrad_mfma", mfma)
        try:
            st = ParamStore(lora_param_specs(1, D, r), DEV)
            lora = LoraQV(1, D, r, 16.0, 0.05, st.p, st.g, DEV)
            assert lora.s == s
            st.flat_g.zero_()
            lora._wgrad(0, (dx_ext, dx_ext.data_ptr(), dx_ext.stride(0)), dqkv, x_ext, p, seed)
            torch.cuda.synchronize()
            outs[mfma] = [st.g[n].double().clone() for n in lora.names(0)]
        finally:
            L.load().mh_set_option(b"lora_wgrad_mfma", 1)
    x = x_ext[:, :D].double()
    if p > 0:
        ones = torch.ones(M, D, dtype=torch.bfloat16, device=DEV)
        kq = (ops.dropout_bf16(ones, p, seed) != 0).double() / (1 - p)
        kv = (ops.dropout_bf16(ones, p, seed ^ V_TAG) != 0).double() / (1 - p)
    else:
        kq = kv = torch.ones(M, D, dtype=torch.float64, device=DEV)
    sg = s * dx_ext[:, D:D + 2 * r].double()                                  # [M, 2r]
    st_ = x_ext[:, D:].double().reshape(M, BORDER // (2 * r), 2 * r).sum(1)   # the border's groups add up to s * t
    want = [sg[:, :r].T @ (x * kq), sg[:, r:].T @ (x * kv),
            dqkv[:, :D].double().T @ st_[:, :r], dqkv[:, 2 * D:].double().T @ st_[:, r:]]
    for a, b, w in zip(outs[0], outs[1], want):
        scale = float(w.abs().max())
        assert scale > 0
        assert float((a - b).abs().max()) <= 2e-5 * scale
        assert float((b - w).abs().max()) <= 1e-4 * scale and float((a - w).abs().max()) <= 1e-4 * scale


@pytest.mark.parametrize("M,K,p", [(1184, 12288, 0.05), (1184, 12288, 0.0), (148, 12288, 0.05), (37, 12288, 0.05)])
def test_lora_dx_and_the_input_norm_backward_in_one_kernel_are_bit_identical(M, K, p):
    """mh_gemm_lora_rmsnorm_bwd (LoRA dx correction + the input RMSNorm's backward as ONE kernel that also sums the dgrad's
    split-K slabs: csrc/lora.hip lora_dx_rmsnorm_bwd_kernel) against the same call with option lora_norm_fused = 0 (lora_dx ->
    [M, D] f32 -> rmsnorm_bwd) and against the three separate calls: same dh (f32 and bf16), same dA / dB, bit for bit --
    at the training shape (split K, bf16 slabs), at batch 1 and at 37 rows (fp32 slabs, up to 15 of them; a ragged last row
    group, M % 4 != 0), with and without dropout."""
    from myriad_amd.lora import BORDER, LoraQV, lora_param_specs
    from myriad_amd.myriad import ParamStore
    ops.ensure_workspace(torch.device(DEV))
    D, r = 4096, 8
    lib = L.load()
    gen = torch.Generator().manual_seed(177)
    outs = []
    for mode in ("fused", "unfused_option", "three_calls"):
        st = ParamStore(lora_param_specs(1, D, r), DEV)
        g2 = torch.Generator().manual_seed(178)
        for name, ishape, _ in st.specs:
            st.p[name].copy_(torch.randn(ishape, generator=g2) * 0.05)
        lora = LoraQV(1, D, r, 16.0, p, st.p, st.g, DEV)
        gen.manual_seed(179)
        dqkv = (torch.randn(M, K, generator=gen) * 0.02).to(DEV).to(torch.bfloat16)
        wT = (torch.randn(D + BORDER, K, generator=gen) * 0.02).to(DEV).to(torch.bfloat16)
        x_ext = (torch.randn(M, D + BORDER, generator=gen) * 0.5).to(DEV).to(torch.bfloat16)
        h_in = torch.randn(M, D, generator=gen).to(DEV)
        w = (1.0 + 0.1 * torch.randn(D, generator=gen)).to(DEV)
        dres = torch.randn(M, D, generator=gen).to(DEV)
        seed = 123456789
        prev = lib.mh_set_option(b"lora_norm_fused", 0 if mode == "unfused_option" else 1)
        try:
            if mode == "three_calls":
                dxn = lora.backward_from_dqkv(0, dqkv, wT, x_ext, p, seed)
                dh, dhb = ops.rmsnorm_bwd(dxn, h_in, w, 1e-6, dres=dres, want_bf16=True)
            else:
                dh, dhb = lora.backward_from_dqkv_norm(0, dqkv, wT, x_ext, p, seed, h_in, w, 1e-6, dres)
        finally:
            lib.mh_set_option(b"lora_norm_fused", prev)
        torch.cuda.synchronize()
        outs.append((dh.clone(), dhb.clone(), st.flat_g.clone()))
    for o in outs[1:]:
        assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1])
        assert torch.equal(outs[0][2], o[2])
    assert float(outs[0][2].abs().sum()) > 0 and bool(torch.isfinite(outs[0][0]).all())


@pytest.mark.parametrize("dropout", [0.0, 0.05])
def test_llama_lora_qv_vs_oracle(dropout):
    """q/v LoRA as a K-border of the qkv GEMM vs the oracle's restated peft formula (parity unpinned by the
    reference: peft is un-vendored).  With dropout the oracle is fed the HIP path's own keep-masks (one per wrapped
    Linear, as peft's per-module nn.Dropout draws them: the v mask is the q mask's hash under lora.V_TAG)."""
    from myriad_amd.lora import LoraQV, PEFT_PREFIX, lora_param_specs
    from myriad_amd.myriad import ParamStore
    D, layers, heads, inter, V, r = 4096, 1, 32, 11008, 1000, 8
    sd = gu.llama_weights(D, layers, inter, V, seed=611)
    gen = torch.Generator().manual_seed(612)
    lora_sd = {}
    for name, ishape, _ in lora_param_specs(layers, D, r):
        lora_sd[name] = torch.randn(ishape, generator=gen) * (0.02 if "lora_A" in name else 0.05)
    emb = torch.randn(2, 24, D, generator=gen) * 0.02
    mask = torch.ones(2, 24, dtype=torch.long)
    mask[1, -4:] = 0
    labels = torch.randint(3, V, (2, 24), generator=gen)
    labels[:, :10] = -100
    labels[mask == 0] = -100
    st = ParamStore(lora_param_specs(layers, D, r), DEV)
    for n in lora_sd:
        st.p[n].copy_(lora_sd[n])
    lm = LlamaHIP(sd, heads, DEV)
    lora = LoraQV(layers, D, r, 16.0, dropout, st.p, st.g, DEV)
    lm.attach_lora(lora)
    lora.step_seed = 3
    loss = lm.forward_loss(emb.to(DEV), mask, labels)
    demb = lm.backward()
    # oracle with the same parameters under its own key convention
    osd = dict(sd)
    for n, t in lora_sd.items():
        osd[n.replace(PEFT_PREFIX, "llama_model.model.layers.")] = t.clone().requires_grad_(True)
    dmask = None
    if dropout > 0:
        seed = (3 * 1315423911 + 0 * 2654435761 + 12345) & 0x7FFFFFFFFFFFFFFF
        ones = torch.ones(48, D, dtype=torch.bfloat16, device=DEV)
        from myriad_amd.lora import V_TAG
        dmask = {"q_proj": ops.dropout_bf16(ones, dropout, seed).float().cpu().view(2, 24, D),      # keep/(1-p) factors
                 "v_proj": ops.dropout_bf16(ones, dropout, seed ^ V_TAG).float().cpu().view(2, 24, D)}
        assert 0.90 < float((dmask["q_proj"] > 0).float().mean()) < 0.99
        both = float(((dmask["q_proj"] > 0) & (dmask["v_proj"] > 0)).float().mean())
        assert abs(both - (1 - dropout) ** 2) < 5e-3                # independent draws, not one shared mask
    e = emb.clone().requires_grad_(True)
    loss_ref, _ = R.llama_causal_lm(osd, e, mask, labels, heads, lora=dict(r=r, alpha=16.0, dropout_mask=dmask))
    loss_ref.backward()
    assert abs(loss.item() - loss_ref.item()) < 3e-3 * abs(loss_ref.item())
    assert relerr(demb, e.grad) < 5e-2
    for n in lora_sd:
        want = osd[n.replace(PEFT_PREFIX, "llama_model.model.layers.")].grad
        assert relerr(st.g[n], want) < 6e-2, n


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_lora_qv_known_answer_hand_computed(p):
    """a-14 pinned independently of the oracle: peft's form  y = W x + (alpha/r) B A drop(x)  on q_proj / v_proj through the
    library's own path (lora_down -> bordered qkv GEMM; bordered dgrad GEMM -> lora_dx / lora_wgrad) on small integer
    operands, so every expected value is exact.  Row 0 / columns 0..3 of q_proj embed the case worked by hand in
    tests/test_oracle_golden.py (LORA_KAT, literals); the rest is checked against plain numpy int64 sums written out here.
    p = 0.5 (factor 2, exact): the keep mask is the library's counter-based one, read back through mh_dropout_bf16."""
    from myriad_amd.lora import BORDER, V_TAG, LoraQV, lora_param_specs
    from myriad_amd.myriad import ParamStore
    from tests.test_oracle_golden import LORA_KAT as k
    D, r, M, s = 128, 8, 4, 2
    rng = np.random.default_rng(5)

    def sparse(shape, lo, hi, dens):
        return rng.integers(lo, hi + 1, shape) * (rng.random(shape) < dens)

    x = sparse((M, D), -2, 2, 0.25)
    W = sparse((3 * D, D), -1, 1, 0.2)
    Aq, Av = sparse((r, D), -1, 1, 0.2), sparse((r, D), -1, 1, 0.2)
    Bq, Bv = sparse((D, r), -1, 1, 0.3), sparse((D, r), -1, 1, 0.3)
    dqkv = sparse((M, 3 * D), -1, 1, 0.2)
    # the hand-worked 4 x 4, rank-2 case in row 0 of the batch, rows 0..3 of q_proj
    x[:, :4] = 0; dqkv[:, :4] = 0                                  # rows 1.. stay out of the literal 4 x 4 gradients
    x[0] = 0; x[0, :4] = k["x"]
    W[:4] = 0; W[:4, :4] = k["W"]
    Aq[:, :4] = 0; Aq[:2, :4] = k["A"]
    Bq[:4] = 0; Bq[:4, :2] = k["B"]
    dqkv[0] = 0; dqkv[0, :4] = k["dy"]
    st = ParamStore(lora_param_specs(1, D, r), DEV)
    lora = LoraQV(1, D, r, 16.0, p, st.p, st.g, DEV)
    nAq, nAv, nBq, nBv = lora.names(0)
    for n, a in ((nAq, Aq), (nAv, Av), (nBq, Bq), (nBv, Bv)):
        st.p[n].copy_(torch.from_numpy(a).float())
    layer = dict(wqkv=torch.from_numpy(W).to(DEV, torch.bfloat16), wqkvT=torch.from_numpy(W.T.copy()).to(DEV, torch.bfloat16))
    lora.extend_weights(layer)
    lora.refresh([layer])
    lora.step_seed = 9
    x_ext = lora.x_ext(0, M)
    x_ext[:, :D].copy_(torch.from_numpy(x).to(DEV, torch.bfloat16))
    p_eff, seed = lora.forward_border(0, x_ext, training=True)
    assert p_eff == p
    qkv = ops.gemm(x_ext, layer["wqkv_ext"], out_dtype=torch.float32).cpu().numpy()
    if p > 0:
        ones = torch.ones(M, D, dtype=torch.bfloat16, device=DEV)
        mq = ops.dropout_bf16(ones, p, seed).float().cpu().numpy().astype(np.int64)
        mv = ops.dropout_bf16(ones, p, seed ^ V_TAG).float().cpu().numpy().astype(np.int64)
        assert set(np.unique(mq)) == {0, 2} and set(np.unique(mv)) == {0, 2} and (mq != mv).any()
    else:
        mq = mv = np.ones((M, D), np.int64)
    tq, tv = (x * mq) @ Aq.T, (x * mv) @ Av.T                       # [M, r] int64
    assert np.abs(s * tq).max() <= 256 and np.abs(s * tv).max() <= 256      # the border holds s*t in bf16: exact
    want = x @ W.T
    want[:, :D] += s * tq @ Bq.T
    want[:, 2 * D:] += s * tv @ Bv.T
    assert np.array_equal(qkv, want.astype(np.float32))
    if p == 0:
        assert qkv[0, :4].tolist() == k["y"]                        # the literal, hand-computed answer
    # ---- backward
    st.flat_g.zero_()
    dq_t = torch.from_numpy(dqkv).to(DEV, torch.bfloat16)
    dxn = lora.backward_from_dqkv(0, dq_t, layer["wqkvT_ext"], x_ext, p_eff, seed, defer_wgrad=False).cpu().numpy()
    torch.cuda.synchronize()
    dq, dv = dqkv[:, :D], dqkv[:, 2 * D:]
    gq, gv = dq @ Bq, dv @ Bv                                       # [M, r]
    want_dx = dqkv @ W + s * mq * (gq @ Aq) + s * mv * (gv @ Av)
    assert np.array_equal(dxn, want_dx.astype(np.float32))
    assert np.array_equal(st.g[nAq].cpu().numpy(), (s * gq.T @ (x * mq)).astype(np.float32))
    assert np.array_equal(st.g[nAv].cpu().numpy(), (s * gv.T @ (x * mv)).astype(np.float32))
    assert np.array_equal(st.g[nBq].cpu().numpy(), (s * dq.T @ tq).astype(np.float32))
    assert np.array_equal(st.g[nBv].cpu().numpy(), (s * dv.T @ tv).astype(np.float32))
    if p == 0:
        assert dxn[0, :4].tolist() == k["dx"]
        assert st.g[nAq][:2, :4].cpu().tolist() == k["dA"] and st.g[nBq][:4, :2].cpu().tolist() == k["dB"]
