"""Trainable Q-Former (freeze_qformer: False) on the MI355X: the TN weight-gradient GEMM, the LayerNorm parameter gradients,
and the model's Q-Former gradients and update against torch autograd / torch.optim.AdamW."""
import math

import pytest
import torch

from myriad_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32


def _bf(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF16).to(DEV)


def _check_tn(got, dy, x, base=None):
    ref = dy.double().t() @ x.double()
    if base is not None:
        ref = ref + base.double()
    bound = dy.double().abs().t() @ x.double().abs()
    err = (got.double() - ref).abs()
    assert bool((err <= 2e-6 * bound + 1e-6).all()), float((err / (bound + 1e-30)).max())


@pytest.mark.parametrize("M,N,K", [(648, 2304, 768), (648, 768, 768), (648, 3072, 768), (648, 768, 3072),
                                   (256, 768, 768), (2056, 9216, 1408), (77, 128, 192), (1001, 192, 64)])
def test_tn_wgrad_matches_fp64_and_is_deterministic(M, N, K):
    dy, x = _bf((M, N), 1, 0.5), _bf((M, K), 2)
    out = torch.full((N, K), float("nan"), dtype=F32, device=DEV)
    bias = torch.full((N,), float("nan"), dtype=F32, device=DEV)
    ops.gemm_tn_wgrad(dy, x, out, bias=bias)
    _check_tn(out, dy, x)
    ref_b = dy.double().sum(0)
    assert torch.allclose(bias.double(), ref_b, rtol=0, atol=1e-6 * float(dy.double().abs().sum(0).max()) + 1e-6)
    out2 = torch.empty_like(out)
    bias2 = torch.empty_like(bias)
    ops.gemm_tn_wgrad(dy, x, out2, bias=bias2)
    assert torch.equal(out, out2) and torch.equal(bias, bias2)          # bit-identical run to run
    one = torch.empty_like(out)
    ops.gemm_tn_wgrad(dy, x, one, splits=1)                               # the unsplit form agrees to fp32 rounding
    _check_tn(one, dy, x)


@pytest.mark.parametrize("splits", [1, 0, 3])
def test_tn_wgrad_accumulates_into_strided_output(splits):
    M, N, K = 333, 256, 128
    dy, x = _bf((M, N), 3), _bf((M, K), 4)
    big = torch.randn((N, K + 64), dtype=F32, device=DEV)
    base = big[:, :K].clone()
    bias = torch.randn((N,), dtype=F32, device=DEV)
    bias0 = bias.clone()
    ops.gemm_tn_wgrad(dy, x, big[:, :K], bias=bias, accumulate=True, splits=splits)
    _check_tn(big[:, :K], dy, x, base=base)
    assert torch.allclose(bias.double(), bias0.double() + dy.double().sum(0), atol=1e-4)


def test_tn_wgrad_rejects_unsupported_shapes():
    dy, x = _bf((64, 100), 5), _bf((64, 64), 6)
    with pytest.raises(Exception):
        ops.gemm_tn_wgrad(dy, x, torch.empty((100, 64), dtype=F32, device=DEV))


@pytest.mark.parametrize("M,D", [(648, 768), (2056, 1408), (37, 64)])
def test_layernorm_param_grads(M, D):
    g = torch.Generator().manual_seed(M)
    x = (torch.randn((M, D), generator=g) * 3 + 1).to(DEV)
    dy = torch.randn((M, D), generator=g).to(DEV)
    dg = torch.full((D,), float("nan"), dtype=F32, device=DEV)
    db = torch.full((D,), float("nan"), dtype=F32, device=DEV)
    ops.layernorm_param_grads(dy, x, 1e-12, dg, db)
    xd = x.double()
    xhat = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-12)
    ref_g, ref_b = (dy.double() * xhat).sum(0), dy.double().sum(0)
    scale = float(dy.double().abs().sum(0).max()) * 3
    assert (dg.double() - ref_g).abs().max() < 2e-5 * scale
    assert (db.double() - ref_b).abs().max() < 2e-5 * scale
    dg2, db2 = dg.clone(), db.clone()
    ops.layernorm_param_grads(dy, x, 1e-12, dg2, db2, accumulate=True)
    assert torch.allclose(dg2, 2 * dg, rtol=1e-6, atol=1e-5) and torch.allclose(db2, 2 * db, rtol=1e-6, atol=1e-5)
    dg3, db3 = torch.empty_like(dg), torch.empty_like(db)
    ops.layernorm_param_grads(dy, x, 1e-12, dg3, db3)
    assert torch.equal(dg3, dg) and torch.equal(db3, db)


# ------------------------------------------------------------------------------------------------ dropout kernels
def test_keep_mask_fraction_and_seeds():
    n, p = 1 << 20, 0.1
    m = ops.dropout_keep_mask(n, p, 12345, DEV)
    kept = int((m > 0).sum())
    sd = math.sqrt(n * p * (1 - p))
    assert abs((n - kept) - n * p) < 6 * sd                              # binomial bound
    assert torch.all((m == 0) | (m == torch.tensor(1 / (1 - p), dtype=F32, device=DEV)))
    assert torch.equal(m, ops.dropout_keep_mask(n, p, 12345, DEV))
    assert not torch.equal(m, ops.dropout_keep_mask(n, p, 12346, DEV))
    assert torch.all(ops.dropout_keep_mask(1000, 0.0, 7, DEV) == 1)


@pytest.mark.parametrize("Sq,Sk", [(81, 81), (81, 257), (32, 257)])
def test_attention_dropout_matches_torch_fed_the_kernel_mask(Sq, Sk):
    from tests.qformer_train_ref import attn_dropout_ref
    B, H, D, p, seed = 3, 12, 64, 0.1, 987654321
    scale = 1.0 / math.sqrt(D)
    q, k, v = _bf((B, Sq, H * D), 11), _bf((B, Sk, H * D), 12), _bf((B, Sk, H * D), 13)
    dout = _bf((B, Sq, H * D), 14)
    # p = 0 is the existing kernels, bit for bit
    o0, l0 = ops.attn_fwd(q, k, v, H, D, scale)
    o1, l1 = ops.attn_fwd_dropout(q, k, v, H, D, scale, 0.0, seed)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    o, lse = ops.attn_fwd_dropout(q, k, v, H, D, scale, p, seed)
    o2, _ = ops.attn_fwd_dropout(q, k, v, H, D, scale, p, seed)
    o3, _ = ops.attn_fwd_dropout(q, k, v, H, D, scale, p, seed + 1)
    assert torch.equal(o, o2) and not torch.equal(o, o3)
    keep = ops.dropout_keep_mask(B * H * Sq * Sk, p, seed, DEV).view(B, H, Sq, Sk)
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    ro, rl = attn_dropout_ref(qf, kf, vf, H, D, scale, keep)
    assert (o.float() - ro).abs().max() < 2e-2 * ro.abs().max()
    assert (lse - rl).abs().max() < 1e-3
    ro.backward(dout.float())
    dq, dk, dv = ops.attn_bwd_dropout(q, k, v, o, dout, lse, H, D, scale, p, seed)
    for got, want in ((dq, qf.grad), (dk, kf.grad), (dv, vf.grad)):
        rel = float((got.float() - want).norm() / want.norm())
        assert rel < 3e-2, rel


def test_hidden_dropout_layernorm_matches_torch_fed_the_kernel_mask():
    from tests.qformer_train_ref import ln_dropout_ref
    M, D, p, eps = 648, 768, 0.1, 1e-12
    g = torch.Generator().manual_seed(21)
    z, res = torch.randn(M, D, generator=g).to(DEV), torch.randn(M, D, generator=g).to(DEV)
    w, b = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV), (0.1 * torch.randn(D, generator=g)).to(DEV)
    dy = torch.randn(M, D, generator=g).to(DEV)
    si, so = 1111, 2222
    # p = 0: the existing LayerNorm forward / backward
    _, yb0, yf0 = ops.layernorm_fwd_dropout(z, None, w, b, eps)
    rb, rf = ops.layernorm_fwd(z, w, b, eps, want_bf16=True, want_f32=True)
    assert torch.allclose(yf0, rf, atol=1e-5) and (yb0.float() - rb.float()).abs().max() <= 1e-2
    ki = ops.dropout_keep_mask(M * D, p, si, DEV).view(M, D)
    ko = ops.dropout_keep_mask(M * D, p, so, DEV).view(M, D)
    for res_, kin, kout in ((res, ki, None), (None, None, ko)):
        x, yb, yf = ops.layernorm_fwd_dropout(z, res_, w, b, eps, p_in=p if res_ is not None else 0.0, seed_in=si,
                                              p_out=p if kout is not None else 0.0, seed_out=so)
        zf = z.clone().requires_grad_(True)
        rx, ry = ln_dropout_ref(zf, res_, w, b, eps, kin, kout)
        assert (yf - ry).abs().max() < 1e-4 * ry.abs().max()
        if res_ is not None:
            assert torch.allclose(x, rx, atol=1e-6)
        xin = x if res_ is not None else z
        dx, dzb = ops.layernorm_bwd_dropout(dy, xin, w, eps, p_in=p if res_ is not None else 0.0, seed_in=si,
                                            p_out=p if kout is not None else 0.0, seed_out=so)
        ry.backward(dy)
        assert (dzb.float() - zf.grad).abs().max() < 1e-2 * zf.grad.abs().max()
        if res_ is not None:                                              # the residual's gradient: unmasked
            assert torch.allclose(dx * ki, zf.grad, atol=1e-4 * float(zf.grad.abs().max()))
        dg, dbb = torch.empty(D, device=DEV), torch.empty(D, device=DEV)
        ops.layernorm_param_grads(dy, xin, eps, dg, dbb, p_out=p if kout is not None else 0.0, seed_out=so)
        wl, bl = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        _, ry2 = ln_dropout_ref(xin, None, wl, bl, eps, None, kout)
        ry2.backward(dy)
        assert torch.allclose(dg, wl.grad, rtol=1e-4, atol=1e-3) and torch.allclose(dbb, bl.grad, rtol=1e-4, atol=1e-3)


# ------------------------------------------------------------------------------------------------ model
def _tiny_model(arch, seed=7, dropout=0.0, drop_seed=None):
    from myriad_amd.myriad import MiniGPT4HIP, MyriadHIP
    from myriad_amd.synthetic import SyntheticWeights, full_config
    cfg = full_config(vit_depth=1, qf_layers=2, llm_layers=1, vocab=1024)
    w = SyntheticWeights(cfg, DEV, seed=seed, arch=arch, big_dtype=F32)
    cls = MyriadHIP if arch == "myriad" else MiniGPT4HIP
    extra = {} if drop_seed is None else dict(qformer_dropout_seed=drop_seed)
    model = cls(w, dict(fixed_stage=1, fixed_taskstage=0, freeze_qformer=False, qformer_dropout=dropout, **extra), device=DEV)
    return cfg, w, model


def _samples(vocab):
    from tests import golden_utils as gu
    image, maps, before, after, tgt, tmask = gu.synthetic_batch(2, vocab, seed=3)
    return dict(image=image, anomaly_maps=maps, oneshot_anomaly_maps=maps, before_ids=before, after_ids=after,
                target_ids=tgt, target_mask=tmask)


def _qf_names(model):
    return [n for n, _, _ in model.store.specs if n == "query_tokens" or n.startswith("Qformer.")]


@pytest.mark.parametrize("arch", ["myriad", "mini_gpt4"])
def test_qformer_gradients_match_torch_autograd_through_the_oracle(arch):
    """Every Q-Former parameter gradient (query_tokens included) of one training backward against
    oracle.myriad_ref.model_forward under torch autograd with the Q-Former weights as leaves."""
    from oracle import myriad_ref as R
    cfg, w, model = _tiny_model(arch)
    s = _samples(cfg["vocab"])
    model.train()
    loss = model(s)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    names = _qf_names(model)
    assert len(names) == 1 + 2 + 2 * 16 + 10                  # query_tokens, embeddings LN, 2 layers, one cross layer
    sd = {k: w[k].float().cpu() for k in w.keys()}
    leaves = {n: sd[n].clone().requires_grad_(True) for n in names}
    sd.update(leaves)
    ref = R.model_forward(sd, s["image"], s["anomaly_maps"] if arch == "myriad" else None, 1, s["before_ids"],
                          s["after_ids"], s["target_ids"], s["target_mask"], arch=arch)
    assert abs(float(loss.detach()) - float(ref.detach())) / abs(float(ref.detach())) < 5e-3
    ref.backward()
    for n in names:
        got, want = model.store.g[n].double().cpu(), leaves[n].grad.double()
        if n.endswith("self.key.bias"):
            # softmax is invariant to a per-row shift of the scores, which is all a key bias adds: its exact gradient is 0 and
            # both sides hold rounding noise.  Measured against the value bias gradient of the same attention.
            scale = leaves[n.replace("key.bias", "value.bias")].grad.double().norm()
            assert float((got - want).norm() / scale) < 6e-2, n
            continue
        rel = float((got - want).norm() / (want.norm() + 1e-30))
        cos = float((got * want).sum() / (got.norm() * want.norm() + 1e-30))
        assert rel < 6e-2 and cos > 0.998, (n, rel, cos)
        assert model._params[n].grad is not None                 # the torch-optimiser bridge sees the .grad view


def test_two_adamw_steps_match_torch_adamw_and_refresh_the_working_copies():
    cfg, w, model = _tiny_model("myriad", seed=9)
    s = _samples(cfg["vocab"])
    model.train()
    st = model.store
    names = _qf_names(model)
    ref = {n: torch.nn.Parameter(st.p[n].detach().double().cpu().clone()) for n in names}
    from myriad_amd.myriad import uses_weight_decay
    wd = [n for n in names if uses_weight_decay(n, len(st.ref_shape[n]))]
    opt = torch.optim.AdamW([{"params": [ref[n] for n in wd], "weight_decay": 0.05},
                             {"params": [ref[n] for n in names if n not in wd], "weight_decay": 0.0}], lr=1e-3)
    v0 = st.version
    L0 = model.qformer.layers[0]
    wqkv_ptr = L0["wqkv"].data_ptr()
    for step in range(2):
        model.train_step(s, lr=1e-3)
        model.finish_update()
        torch.cuda.synchronize()
        for n in names:
            ref[n].grad = st.g[n].detach().double().cpu().clone()
        opt.step()
        for n in names:
            got = st.p[n].detach().double().cpu()
            assert torch.allclose(got, ref[n].detach(), rtol=1e-5, atol=1e-7), (step, n)
    assert st.version > v0                                        # decode sessions keyed on it drop their cache
    model.eval()
    with torch.no_grad():
        model(s)                                                  # a forward rewrites the bf16 copies from the masters
    torch.cuda.synchronize()
    q = "Qformer.bert.encoder.layer.0.attention.self."
    want = torch.cat([st.p[q + f"{x}.weight"] for x in ("query", "key", "value")]).to(BF16)
    assert L0["wqkv"].data_ptr() == wqkv_ptr and torch.equal(L0["wqkv"], want)
    assert torch.equal(L0["wqkvT"], want.t().contiguous())


def test_dropout_is_on_by_default_deterministic_per_seed_and_off_in_eval():
    cfg, w, model = _tiny_model("myriad", dropout=0.1, drop_seed=5)
    assert model.qformer_dropout == 0.1
    s = _samples(cfg["vocab"])

    def run(m):
        m.train()
        loss = m(s)["loss"]
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach()), m.store.flat_g.clone()
    l1, g1 = run(model)
    _, _, model2 = _tiny_model("myriad", dropout=0.1, drop_seed=5)
    l2, g2 = run(model2)
    _, _, model3 = _tiny_model("myriad", dropout=0.1, drop_seed=6)
    l3, g3 = run(model3)
    assert math.isfinite(l1) and bool(torch.isfinite(g1).all())
    assert l1 == l2 and torch.equal(g1, g2)                          # same seed: bit-identical
    assert l1 != l3 and not torch.equal(g1, g3)                      # another seed: other masks
    _, _, model0 = _tiny_model("myriad", dropout=0.0)
    model.eval(); model0.eval()
    with torch.no_grad():
        e1, e0 = model(s)["loss"], model0(s)["loss"]                 # eval: dropout off
    assert float(e1) == float(e0)
