"""The model backwards on the MI355X, probed one token row at a time (tests/backward_probes.py): EvaViTHIP.forward_train /
backward, QFormerHIP.forward / backward(wgrads=True) and LlamaHIP.forward_loss / backward with q/v LoRA, against autograd through
the oracle.  The gates are the project's own (rel < 6e-2 and cos > 0.998; LLaMA: max-abs 5e-2 / 6e-2, loss 3e-3); what is new
is where they are applied -- to gradients that consist of a single row's contribution, and to every row of the input gradients.
Each comparison prints its rel / cos before it is asserted."""
import pytest
import torch

from myriad_amd import ops
from tests import backward_probes as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _gate(tag, got, want, sibling=None):
    """Every tensor of `want` against `got` at the project's gate; `sibling(name)` names the tensor whose norm measures a part
    whose exact gradient is zero.  Returns the largest rel."""
    bad, worst = [], 0.0
    for n, w in want.items():
        sib = sibling(n) if sibling is not None else None
        if sib is not None:
            rel, cos = P.rel_cos(got[n], w, scale=want[sib].double().norm())
            ok = rel < P.REL
        else:
            rel, cos = P.rel_cos(got[n], w)
            ok = rel < P.REL and cos > P.COS
        print(f"{tag} {n}: rel {rel:.3e} cos {cos:.6f}" + (" (exact zero, vs " + sib + ")" if sib else ""))
        worst = max(worst, rel)
        if not ok:
            bad.append((n, rel, cos))
    print(f"{tag}: largest rel {worst:.3e}")
    assert not bad, (tag, bad)
    return worst


def _gate_rows(tag, got, want):
    rel, cos = P.row_rel_cos(got, want)
    i = int(rel.argmax())
    print(f"{tag}: {rel.numel()} rows, largest rel {float(rel[i]):.3e} at row {i}, smallest cos {float(cos.min()):.6f}")
    assert bool((rel < P.REL).all()) and bool((cos > P.COS).all()), (tag, i, float(rel[i]), float(cos.min()))


# ------------------------------------------------------------------------------------------------ ViT
def _vit(depth):
    from myriad_amd.eva_vit import EvaViTHIP
    ops.ensure_workspace(DEV)
    return EvaViTHIP({k: t.to(DEV) for k, t in P.vit_weights(depth).items()}, P.VIT_HEADS, DEV)


@pytest.fixture(scope="module")
def vit1():
    return _vit(1)


def _vit_backward(ve, image, dout, **kw):
    ve.forward_train(image.to(DEV), **kw)
    grads = ve.backward(dout.to(DEV))
    torch.cuda.synchronize()
    return grads


VIT_COT = [(B, b, t) for B in P.VIT_BATCHES for b in P.vit_samples(B) for t in P.VIT_COT_TOKENS]
VIT_IN = [(B, b, p) for B in P.VIT_BATCHES for b in P.vit_samples(B) for p in P.VIT_PATCHES]


@pytest.mark.parametrize("B,b,t", VIT_COT)
def test_vit_backward_of_a_one_row_cotangent(vit1, B, b, t):
    dout = P.vit_row_cot(B, b, t)
    grads = _vit_backward(vit1, P.vit_image(B), dout)
    ref = P.vit_ref(1, B).grads(dout)
    assert set(grads) == set(ref)
    (gl, gr), (wl, wr) = P.vit_split(grads, 0), P.vit_split(ref, 0)
    tag = f"vit B={B} sample={b} token={t}"
    _gate(tag + " localised", gl, wl)
    _gate(tag + " ordinary", gr, wr)


@pytest.mark.parametrize("B,b,p", VIT_IN)
def test_vit_backward_of_a_one_patch_image(vit1, B, b, p):
    image, dout = P.vit_patch_image(B, b, p), P.vit_dense_cot(B)
    grads = _vit_backward(vit1, image, dout)
    n = "visual_encoder.patch_embed.proj.weight"
    ref = P.VitRef(P.vit_weights(1), image, samples=[b]).grads(dout)       # the other samples' patches are zero: they add nothing
    _gate(f"vit B={B} sample={b} patch={p} localised", {n: grads[n]}, {n: ref[n]})


@pytest.mark.parametrize("B", P.VIT_BATCHES)
def test_vit_pos_embed_gradient_row_by_row(vit1, B):
    dout = P.vit_dense_cot(B)
    grads = _vit_backward(vit1, P.vit_image(B), dout)
    ref = P.vit_ref(1, B).grads(dout)
    n = "visual_encoder.pos_embed"
    _gate_rows(f"vit B={B} pos_embed rows", grads[n][0], ref[n][0])
    _gate(f"vit B={B} cls_token", {"visual_encoder.cls_token": grads["visual_encoder.cls_token"]},
          {"visual_encoder.cls_token": ref["visual_encoder.cls_token"]})
    # cls_token's gradient is row 0's share of pos_embed's
    assert torch.equal(grads["visual_encoder.cls_token"].view(-1), grads[n][0, 0])


def test_vit_checkpoint_replay_of_a_one_row_cotangent():
    """Depth 2 with checkpoint=True: the backward replays each block's forward from its saved input.  The probe in the last
    sample's last row localises block 1's parts; block 0's are ordinary."""
    B = 2
    ve = _vit(2)
    dout = P.vit_row_cot(B, B - 1, 256)
    grads = _vit_backward(ve, P.vit_image(B), dout, checkpoint=True)
    ref = P.vit_ref(2, B, only_last=True).grads(dout)
    assert set(grads) == set(ref)
    (gl, gr), (wl, wr) = P.vit_split(grads, 1), P.vit_split(ref, 1)
    _gate("vit depth 2 checkpoint localised", gl, wl)
    _gate("vit depth 2 checkpoint ordinary", gr, wr)


# ------------------------------------------------------------------------------------------------ Q-Former
@pytest.fixture(scope="module")
def qformers():
    from myriad_amd.myriad import ParamStore
    from myriad_amd.qformer import QFormerHIP, qformer_param_specs
    ops.ensure_workspace(DEV)
    out = {}
    for L, _ in P.QF_MODULES:
        sd = P.qf_weights(L)
        st = ParamStore(qformer_param_specs(sd), DEV)
        for n in st.p:
            st.p[n].copy_(sd[n])
        qf = QFormerHIP(sd, P.QF_HEADS, DEV)
        qf.bind_trainable(st)
        out[L] = (qf, st)
    return out


def _qf_backward(qformers, L, q, enc, dout):
    """Every gradient the backward writes, under the reference's names; the store's gradient buffer starts as NaN."""
    qf, st = qformers[L]
    st.flat_g.fill_(float("nan"))
    qf.forward(q.to(DEV), enc.to(DEV))
    dq, denc = qf.backward(dout.to(DEV), wgrads=True, want_denc=True)
    torch.cuda.synchronize()
    got = {n: g.clone() for n, g in st.g.items() if n != "query_tokens"}       # query_tokens' gradient is the model's to write
    got.update(d_query_embeds=dq, d_enc=denc)
    return got


QF_COT = [(L, B, b, q) for L, Bs in P.QF_MODULES for B in Bs for b in P.vit_samples(B) for q in P.QF_QUERIES]
QF_ENC = [(L, B, b, r) for L, Bs in P.QF_MODULES for B in Bs for b in P.vit_samples(B) for r in P.QF_ENC_ROWS]


def _qf_gates(tag, got, ref, local):
    assert set(got) == set(ref)
    _gate(tag + " localised", got, {n: ref[n] for n in local})
    _gate(tag + " ordinary", got, {n: g for n, g in ref.items() if n not in local}, sibling=P.qf_zero_sibling)


@pytest.mark.parametrize("L,B,b,q", QF_COT)
def test_qformer_backward_of_a_one_query_cotangent(qformers, L, B, b, q):
    qe, enc, _ = P.qf_inputs(B)
    dout = P.qf_row_cot(B, b, q)
    got = _qf_backward(qformers, L, qe, enc, dout)
    _qf_gates(f"qformer layers={L} B={B} sample={b} query={q}", got, P.qf_ref(L, B).grads(dout), P.qf_local_names(L))


@pytest.mark.parametrize("L,B,b,r", QF_ENC)
def test_qformer_backward_of_a_one_row_encoder_input(qformers, L, B, b, r):
    qe, _, dout = P.qf_inputs(B)
    enc = P.qf_row_enc(B, b, r)
    got = _qf_backward(qformers, L, qe, enc, dout)
    ref = P.QfRef(P.qf_weights(L), qe, enc).grads(dout)
    _qf_gates(f"qformer layers={L} B={B} sample={b} encoder row={r}", got, ref, P.qf_enc_local_names(L))


@pytest.mark.parametrize("L,B", [(L, B) for L, Bs in P.QF_MODULES for B in Bs])
def test_qformer_input_gradients_row_by_row(qformers, L, B):
    qe, enc, dout = P.qf_inputs(B)
    got = _qf_backward(qformers, L, qe, enc, dout)
    ref = P.qf_ref(L, B).grads(dout)
    _gate_rows(f"qformer layers={L} B={B} d_enc rows", got["d_enc"].reshape(-1, P.QF_ENC), ref["d_enc"].reshape(-1, P.QF_ENC))
    _gate_rows(f"qformer layers={L} B={B} d_query_embeds rows", got["d_query_embeds"].reshape(-1, P.QF_D),
               ref["d_query_embeds"].reshape(-1, P.QF_D))


# ------------------------------------------------------------------------------------------------ LLaMA + q/v LoRA
@pytest.fixture(scope="module", params=[0.0, 0.05], ids=["p=0", "p=0.05"])
def llama(request):
    """The two LoRA dropout settings of test_llama_lora_qv_vs_oracle.  With dropout the oracle is fed the HIP path's own
    keep-masks, read back through ops.dropout_bf16 as that test reads them (one per wrapped Linear)."""
    from myriad_amd.llama import LlamaHIP
    from myriad_amd.lora import V_TAG, LoraQV, lora_param_specs
    from myriad_amd.myriad import ParamStore
    dropout = request.param
    sd, lora_sd, emb, mask, ids = P.llama_case()
    st = ParamStore(lora_param_specs(P.LL_LAYERS, P.LL_D, P.LL_R), DEV)
    for n in lora_sd:
        st.p[n].copy_(lora_sd[n])
    lm = LlamaHIP(sd, P.LL_HEADS, DEV)
    lora = LoraQV(P.LL_LAYERS, P.LL_D, P.LL_R, P.LL_ALPHA, dropout, st.p, st.g, DEV)
    lm.attach_lora(lora)
    lora.step_seed = 3
    if dropout == 0:
        return lm, st, emb.to(DEV), mask, P.llama_ref()
    seed = lora._seed(0)
    ones = torch.ones(P.LL_B * P.LL_S, P.LL_D, dtype=torch.bfloat16, device=DEV)
    shape = (P.LL_B, P.LL_S, P.LL_D)
    dmask = {"q_proj": ops.dropout_bf16(ones, dropout, seed).float().cpu().view(shape),
             "v_proj": ops.dropout_bf16(ones, dropout, seed ^ V_TAG).float().cpu().view(shape)}
    assert 0.90 < float((dmask["q_proj"] > 0).float().mean()) < 0.99 and not torch.equal(dmask["q_proj"], dmask["v_proj"])
    return lm, st, emb.to(DEV), mask, P.LlamaRef(dmask)


def _llama_step(llama, labels):
    lm, st, emb, mask, _ = llama
    st.flat_g.zero_()
    loss = lm.forward_loss(emb, mask, labels)
    demb = lm.backward()
    torch.cuda.synchronize()
    return float(loss), demb.cpu(), {n: g.clone() for n, g in st.g.items()}


def _llama_gates(tag, llama, labels, per_row, sibling=None):
    tag = f"{tag} dropout={llama[0].lora.p}"
    loss, demb, lora = _llama_step(llama, labels)
    ref_loss, want, want_lora = llama[4].loss_and_grads(labels)
    lrel = abs(loss - ref_loss) / abs(ref_loss)
    err = P.max_relerr(demb, want)                                          # every column
    live = P.llama_live_rows(labels)                                        # the index rule is stated there
    dead = float(demb[~live].abs().max()) / float(demb.abs().max())
    print(f"{tag}: loss rel {lrel:.3e}, demb relerr {err:.3e}, rows without gradient / max |demb| {dead:.3e}")
    assert lrel < P.LLAMA_LOSS and err < P.LLAMA_DEMB, (tag, lrel, err)
    assert dead <= P.ZERO_ROW, (tag, dead)
    if per_row:
        g, w = demb[live].double(), want[live].double()
        rows = (g - w).abs().amax(1) / w.abs().amax(1)
        i = int(rows.argmax())
        print(f"{tag}: {rows.numel()} rows, largest row relerr {float(rows[i]):.3e} at live row {i}")
        assert bool((rows < P.LLAMA_DEMB).all()), (tag, i, float(rows[i]))
    for n, w in want_lora.items():
        sib = sibling(n) if sibling is not None else None
        if sib is not None:                                                 # exact zero: the error over the sibling's max-abs
            e = float((lora[n].double().cpu() - w.double()).abs().max() / want_lora[sib].double().abs().max())
        else:
            e = P.max_relerr(lora[n], w)
        print(f"{tag} {n}: relerr {e:.3e}" + (f" (exact zero, vs {sib})" if sib else ""))
        assert e < P.LLAMA_LORA, (tag, n, e)


@pytest.mark.parametrize("b,t", P.LL_SINGLE)
def test_llama_backward_of_a_single_label(llama, b, t):
    """Exactly one label, at position t of sample b.  R.llama_causal_lm pairs logits[:, :-1] with labels[:, 1:], so that label
    is predicted by the logit row t - 1, which under the causal mask reads input rows 0 .. t - 1 of sample b: the reference's
    demb is exactly zero in rows t .. S - 1 of sample b and in every row of the other sample (backward_probes.llama_live_rows;
    the CPU test checks the reference).  On the device those rows may hold at most 2^-20 of the largest |demb|."""
    labels = P.llama_single_labels(P.llama_ref().ids, b, t)
    _llama_gates(f"llama sample={b} label at {t}", llama, labels, per_row=False, sibling=lambda n: P.llama_zero_sibling(n, t))


@pytest.mark.parametrize("first", P.LL_DENSE)
def test_llama_input_gradient_row_by_row(llama, first):
    ref = P.llama_ref()
    _llama_gates(f"llama dense labels from {first}", llama, P.llama_dense_labels(ref.ids, ref.mask, first), per_row=True)
