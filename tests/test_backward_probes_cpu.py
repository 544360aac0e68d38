"""The backward probes of tests/backward_probes.py have the power they claim -- shown on the references alone, without a device.

A localised 2-D part must be rank one and non-zero: generic rows sum to a rank-one matrix only when a single row contributes,
so a backward that loses that row returns zero for the part, a relative error of 1.0 against the 6e-2 gate.  The vector parts
localised by association (biases, LayerNorm parameters) must move by at least half their norm when the probed row is zeroed.
The rows of the per-row checks must not be degenerate.  And the case that motivates all this is recorded: under a dense
cotangent, dropping one token row of the ViT stays inside the dense gate for every tensor."""
import pytest
import torch

from tests import backward_probes as P

RANK1 = 1e-9


def _assert_localised(tag, local, zeroed=None):
    for n, g in local.items():
        norm = float(g.norm())
        assert norm > 0, (tag, n)
        if g.dim() >= 2:
            res = P.rank_one_residual(g)
            print(f"{tag} {n}: rank-one residual {res:.2e}")
            assert res <= RANK1, (tag, n, res)
        elif zeroed is not None:
            moved = float((g - zeroed[n]).norm()) / norm
            assert moved >= 0.5, (tag, n, moved)


# ------------------------------------------------------------------------------------------------ ViT
VIT_COT = [(B, b, t) for B in P.VIT_BATCHES for b in P.vit_samples(B) for t in P.VIT_COT_TOKENS]
VIT_IN = [(B, b, p) for B in P.VIT_BATCHES for b in P.vit_samples(B) for p in P.VIT_PATCHES]


@pytest.fixture(scope="module")
def vit_zeroed():
    """The gradients of the all-zero cotangent -- what every one-row probe becomes when its row is zeroed -- walked through
    the graph once per batch size."""
    cache = {}

    def get(B):
        if B not in cache:
            g = P.vit_ref(1, B).grads(torch.zeros(B, P.VIT_TOK, P.VIT_D), skip_zero=False)
            cache[B] = {n: t for n, t in P.vit_split(g, 0)[0].items() if t.dim() < 2}
        return cache[B]
    return get


@pytest.mark.parametrize("B,b,t", VIT_COT)
def test_vit_one_row_cotangent_localises_its_parts(B, b, t, vit_zeroed):
    g = P.vit_ref(1, B).grads(P.vit_row_cot(B, b, t))
    local, rest = P.vit_split(g, 0)
    assert len(local) == 10 and len(local) + len(rest) == len(g) + 1
    _assert_localised(f"vit B={B} b={b} t={t}", local, vit_zeroed(B))
    # the k | v thirds are spread over the sample's rows by the attention: not rank one, which is why they are not in the list
    assert P.rank_one_residual(rest["visual_encoder.blocks.0.attn.qkv.weight[kv]"]) > 1e-3


@pytest.mark.parametrize("B,b,p", VIT_IN)
def test_vit_one_patch_image_localises_the_patch_embedding(B, b, p):
    ref = P.VitRef(P.vit_weights(1), P.vit_patch_image(B, b, p), samples=[b])      # the other samples' patches are all zero
    g = ref.grads(P.vit_dense_cot(B))
    _assert_localised(f"vit B={B} b={b} patch={p}", {"patch_embed.proj.weight": g["visual_encoder.patch_embed.proj.weight"]})


def test_vit_checkpoint_probe_localises_the_last_block_only():
    B = 2
    g = P.vit_ref(2, B, only_last=True).grads(P.vit_row_cot(B, B - 1, 256))
    local, rest = P.vit_split(g, 1)
    assert len(local) == 10 and all("blocks.1." in n for n in local)
    _assert_localised("vit depth 2", local)
    assert P.rank_one_residual(rest["visual_encoder.blocks.0.mlp.fc2.weight"]) > 1e-3


@pytest.mark.parametrize("B", P.VIT_BATCHES)
def test_vit_pos_embed_rows_are_not_degenerate(B):
    g = P.vit_ref(1, B).grads(P.vit_dense_cot(B))
    assert P.min_row_norm_over_median(g["visual_encoder.pos_embed"][0]) > 1e-3


def test_dense_gate_does_not_see_a_dropped_token_row():
    """B = 2, dense cotangent, the row of (sample 1, token 256) zeroed: every one of the 17 tensors moves by less than the gate."""
    B = 2
    ref = P.vit_ref(1, B)
    dout = P.vit_dense_cot(B)
    full = ref.grads(dout)
    dropped = dout.clone()
    dropped[1, 256] = 0
    lost = ref.grads(dropped)
    assert len(full) == 17
    worst_rel, worst_cos = 0.0, 1.0
    for n in full:
        rel, cos = P.rel_cos(lost[n], full[n])
        print(f"dropped row, {n}: rel {rel:.2e} cos {cos:.5f}")
        assert 1e-3 < rel < P.REL and cos > P.COS, (n, rel, cos)
        worst_rel, worst_cos = max(worst_rel, rel), min(worst_cos, cos)
    print(f"worst rel {worst_rel:.2e}, worst cos {worst_cos:.5f}")


# ------------------------------------------------------------------------------------------------ Q-Former
QF_COT = [(L, B, b, q) for L, Bs in P.QF_MODULES for B in Bs for b in P.vit_samples(B) for q in P.QF_QUERIES]
QF_ENC = [(L, B, b, r) for L, Bs in P.QF_MODULES for B in Bs for b in P.vit_samples(B) for r in P.QF_ENC_ROWS]


@pytest.mark.parametrize("L,B,b,q", QF_COT)
def test_qformer_one_query_cotangent_localises_the_last_layer(L, B, b, q):
    ref = P.qf_ref(L, B)
    g = ref.grads(P.qf_row_cot(B, b, q))
    zeroed = ref.grads(torch.zeros(B, P.QF_NQ, P.QF_D))
    names = P.qf_local_names(L)
    assert len(names) == (18 if L == 1 else 12)
    _assert_localised(f"qformer L={L} B={B} b={b} q={q}", {n: g[n] for n in names}, zeroed)
    if L == 2:      # the self-attention of the last layer spreads dk / dv over the queries: layer 0 is not localised
        assert P.rank_one_residual(g[P.QF_PREFIX + "encoder.layer.0.crossattention.self.query.weight"]) > 1e-3


@pytest.mark.parametrize("L,B,b,r", QF_ENC)
def test_qformer_one_row_encoder_input_localises_the_cross_key_and_value(L, B, b, r):
    q, _, dout = P.qf_inputs(B)
    g = P.QfRef(P.qf_weights(L), q, P.qf_row_enc(B, b, r)).grads(dout)
    _assert_localised(f"qformer L={L} B={B} b={b} enc row={r}", {n: g[n] for n in P.qf_enc_local_names(L)})


@pytest.mark.parametrize("L,B", [(L, B) for L, Bs in P.QF_MODULES for B in Bs])
def test_qformer_input_gradient_rows_are_not_degenerate(L, B):
    g = P.qf_ref(L, B).grads(P.qf_inputs(B)[2])
    assert P.min_row_norm_over_median(g["d_enc"].reshape(-1, P.QF_ENC)) > 1e-3
    assert P.min_row_norm_over_median(g["d_query_embeds"].reshape(-1, P.QF_D)) > 1e-3


# ------------------------------------------------------------------------------------------------ LLaMA
@pytest.mark.parametrize("b,t", P.LL_SINGLE)
def test_llama_single_label_reference_is_zero_outside_the_rows_before_the_label(b, t):
    ref = P.llama_ref()
    labels = P.llama_single_labels(ref.ids, b, t)
    live = P.llama_live_rows(labels)
    assert int(live.sum()) == t and bool(live[b, :t].all())
    _, demb, lora = ref.loss_and_grads(labels)
    assert float(demb[~live].abs().max()) == 0.0                      # exact zeros: the device is held to 2^-20 of max |demb|
    assert float(demb[live].norm(dim=1).min()) > 0
    for n, g in lora.items():
        sib = P.llama_zero_sibling(n, t)
        if sib is None:
            assert float(g.norm()) > 0, n
        else:
            assert float(g.norm()) <= 1e-6 * float(lora[sib].norm()), n


@pytest.mark.parametrize("first", P.LL_DENSE)
def test_llama_dense_label_rows_are_not_degenerate(first):
    ref = P.llama_ref()
    labels = P.llama_dense_labels(ref.ids, ref.mask, first)
    live = P.llama_live_rows(labels)
    assert int(live.sum()) == (P.LL_S - 1) + (P.LL_S - P.LL_PAD - 1)
    n_rows = int((labels[:, 1:] != -100).sum())
    assert (16 < n_rows <= P.LL_B * P.LL_S // 2) == (first == 45)     # the two dense cases sit on either side of the row gather
    _, demb, _ = ref.loss_and_grads(labels)
    assert float(demb[~live].abs().max()) == 0.0
    assert P.min_row_norm_over_median(demb[live]) > 1e-3
