"""EVA ViT training pieces on the MI355X: the fused dgrad + LayerNorm backward (ops.gemm_layernorm_bwd), the attention LSE
of the ViT's whole-sequence kernel, EvaViTHIP.forward_train / backward against float64 autograd through the oracle, and
visual_encoder.* checkpoint keys loaded into a frozen model."""
import pytest
import torch

from myriad_amd import ops
from tests.fp64_bounds import U16, U32, assert_within, gemm_ref_bound, poisoned

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
EPS = 1e-6


def _rnd(shape, seed, scale=1.0, shift=0.0, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(dtype).to(DEV)


def _ln_case(M, N, K, seed):
    a = _rnd((M, K), seed, 0.5, dtype=BF16)
    b = _rnd((N, K), seed + 1, 0.05, dtype=BF16)
    x = _rnd((M, N), seed + 2, 2.0, 0.5)
    w = _rnd((N,), seed + 3, 0.2, 1.0)
    dres = _rnd((M, N), seed + 4, 0.1)
    return a, b, x, w, dres


# (M, K) at N = 1408: the ViT's LN1 (K = 4224, the qkv dgrad) and LN2 (K = 6144, the fc1 dgrad) at 1, 1 and 16 images,
# plus two reductions the planner never splits
CASES = [(1, 4224), (257, 4224), (257, 6144), (4112, 6144), (4112, 4224), (257, 1408), (4112, 64)]


def test_gemm_layernorm_bwd_cases_cover_split_and_unsplit():
    ops.ensure_workspace(DEV)
    splits = [ops.gemm_plan(M, 1408, K, out_f32=True)[1] for M, K in CASES]
    assert any(s > 1 for s in splits) and any(s == 1 for s in splits), splits


@pytest.mark.parametrize("M,K", CASES)
@pytest.mark.parametrize("params", [False, True])
def test_gemm_layernorm_bwd_bits_equal_the_unfused_launches(M, K, params):
    ops.ensure_workspace(DEV)
    N = 1408
    a, b, x, w, dres = _ln_case(M, N, K, M + K)
    dg = poisoned((N,), F32, DEV) if params else None
    db = poisoned((N,), F32, DEV) if params else None
    dx, dxb = ops.gemm_layernorm_bwd(a, b, x, w, EPS, dres=dres, dgamma=dg, dbeta=db)
    dy = ops.gemm(a, b, out_dtype=F32)
    rx, rxb = ops.layernorm_bwd(dy, x, w, EPS, dres=dres, want_f32=True, want_bf16=True)
    torch.cuda.synchronize()
    assert torch.equal(dx, rx) and torch.equal(dxb, rxb)
    if params:
        rg, rb = torch.empty(N, dtype=F32, device=DEV), torch.empty(N, dtype=F32, device=DEV)
        ops.layernorm_param_grads(dy, x, EPS, rg, rb)
        assert torch.equal(dg, rg) and torch.equal(db, rb)
        ops.gemm_layernorm_bwd(a, b, x, w, EPS, dres=dres, dgamma=dg, dbeta=db, accumulate=True)
        ops.layernorm_param_grads(dy, x, EPS, rg, rb, accumulate=True)
        assert torch.equal(dg, rg) and torch.equal(db, rb)


@pytest.mark.parametrize("M,N,K,params", [(1028, 3072, 4096, True), (257, 3072, 1024, True), (1028, 5120, 4096, False),
                                          (77, 8192, 512, False), (514, 4096, 4096, True), (257, 6144, 2048, False)])
def test_gemm_layernorm_bwd_wide_rows_bits(M, N, K, params):
    """Rows wider than 2048 (4 and 8 float4 chunks a thread in the slab kernel), split and unsplit."""
    ops.ensure_workspace(DEV)
    a, b, x, w, dres = _ln_case(M, N, K, 7 * M + N)
    dg = poisoned((N,), F32, DEV) if params else None
    db = poisoned((N,), F32, DEV) if params else None
    dx, dxb = ops.gemm_layernorm_bwd(a, b, x, w, EPS, dres=dres, dgamma=dg, dbeta=db)
    dy = ops.gemm(a, b, out_dtype=F32)
    rx, rxb = ops.layernorm_bwd(dy, x, w, EPS, dres=dres, want_f32=True, want_bf16=True)
    if params:
        rg, rb = torch.empty(N, dtype=F32, device=DEV), torch.empty(N, dtype=F32, device=DEV)
        ops.layernorm_param_grads(dy, x, EPS, rg, rb)
    torch.cuda.synchronize()
    assert torch.equal(dx, rx) and torch.equal(dxb, rxb)
    if params:
        assert torch.equal(dg, rg) and torch.equal(db, rb)


def test_gemm_layernorm_bwd_wide_cases_split():
    ops.ensure_workspace(DEV)
    assert ops.gemm_plan(1028, 3072, 4096, out_f32=True)[1] > 1 and ops.gemm_plan(1028, 5120, 4096, out_f32=True)[1] > 1


@pytest.mark.parametrize("M,K", [(1, 4224), (257, 6144), (4112, 4224)])
def test_gemm_layernorm_bwd_within_fp64_bounds_with_poisoned_outputs(M, K):
    """Every output buffer and the dY scratch start as NaN; the results are bounded against float64."""
    ops.ensure_workspace(DEV)
    N = 1408
    a, b, x, w, dres = _ln_case(M, N, K, 3 * M + K)
    dy, dx = poisoned((M, N), F32, DEV), poisoned((M, N), F32, DEV)
    dxb = poisoned((M, N), BF16, DEV)
    dg, db = poisoned((N,), F32, DEV), poisoned((N,), F32, DEV)
    nws = ops._L().mh_layernorm_param_grads_ws_floats(M, N)
    ws = poisoned((nws,), F32, DEV)
    rc = ops._L().mh_gemm_layernorm_bwd(a.data_ptr(), K, b.data_ptr(), K, dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                                        dres.data_ptr(), dx.data_ptr(), dxb.data_ptr(), dg.data_ptr(), db.data_ptr(), 0,
                                        ws.data_ptr(), nws, M, N, K, EPS, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    kern, splits = ops.gemm_plan(M, N, K, out_f32=True)
    g, e_g = gemm_ref_bound(a, b, splits=splits, bf16_slabs=splits > 1 and kern in (2, 4, 5))   # the 8-wave kernels' slabs are bf16
    x64, w64 = x.double(), w.double()
    assert_within(dy, g, e_g, "dY")
    mean = x64.mean(1, keepdim=True)
    r = 1.0 / torch.sqrt(x64.var(1, unbiased=False, keepdim=True) + EPS)
    xhat = (x64 - mean) * r
    gw = g * w64
    ref = r * (gw - gw.mean(1, keepdim=True) - xhat * (gw * xhat).mean(1, keepdim=True)) + dres.double()
    # dY's error through the linear map, plus f32 rounding of the row statistics, the sums over N and the output
    E1 = e_g * w64.abs()
    ag = gw.abs()
    bound = r * (E1 + E1.mean(1, keepdim=True) + xhat.abs() * (E1 * xhat.abs()).mean(1, keepdim=True)) + 64 * U32 * (
        r * (ag + ag.mean(1, keepdim=True) + (1 + xhat.abs()) * (ag * xhat.abs()).mean(1, keepdim=True)) + dres.double().abs())
    assert_within(dx, ref, bound, "dx")
    assert_within(dxb, ref, bound + U16 * (ref.abs() + bound), "dx bf16")
    rg, rb = (g * xhat).sum(0), g.sum(0)
    acc = 64 * U32 * (1 + M / 16)
    assert_within(dg, rg, (e_g * xhat.abs()).sum(0) + acc * (g.abs() * (1 + xhat.abs())).sum(0), "dgamma")
    assert_within(db, rb, e_g.sum(0) + acc * g.abs().sum(0), "dbeta")


def test_attn_full_lse_leaves_output_bits_and_matches_fp64():
    B, S, H, hd = 2, 257, 16, 88
    D = H * hd
    qkv = _rnd((B, S, 3 * D), 11, 1.0, dtype=BF16)
    q, k, v = qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:]
    scale = hd ** -0.5
    o0, none = ops.attn_fwd(q, k, v, H, hd, scale, need_lse=False)
    o1, lse = ops.attn_fwd(q, k, v, H, hd, scale, need_lse=True)
    torch.cuda.synchronize()
    assert none is None and torch.equal(o0, o1)
    qh = q.double().view(B, S, H, hd).transpose(1, 2)
    kh = k.double().view(B, S, H, hd).transpose(1, 2)
    ref = torch.logsumexp(qh @ kh.transpose(-1, -2) * scale, -1)
    assert float((lse.double() - ref).abs().max()) < 1e-3


# ------------------------------------------------------------------------------------------------ ViT backward
def _vit_weights(depth, seed=5, D=1408, Hd=6144, P=14, ntok=257):
    g = torch.Generator().manual_seed(seed)

    def n(*shape, s=0.02, m=0.0):
        return torch.randn(shape, generator=g) * s + m

    v = "visual_encoder."
    sd = {v + "cls_token": n(1, 1, D, s=0.5), v + "pos_embed": n(1, ntok, D, s=0.5),
          v + "patch_embed.proj.weight": n(D, 3, P, P, s=0.05), v + "patch_embed.proj.bias": n(D, s=0.1)}
    for i in range(depth):
        p = v + f"blocks.{i}."
        sd.update({p + "norm1.weight": n(D, s=0.1, m=1.0), p + "norm1.bias": n(D, s=0.1),
                   p + "attn.qkv.weight": n(3 * D, D, s=0.04), p + "attn.q_bias": n(D, s=0.1), p + "attn.v_bias": n(D, s=0.1),
                   p + "attn.proj.weight": n(D, D), p + "attn.proj.bias": n(D, s=0.1),
                   p + "norm2.weight": n(D, s=0.1, m=1.0), p + "norm2.bias": n(D, s=0.1),
                   p + "mlp.fc1.weight": n(Hd, D), p + "mlp.fc1.bias": n(Hd, s=0.1),
                   p + "mlp.fc2.weight": n(D, Hd), p + "mlp.fc2.bias": n(D, s=0.1)})
    return sd


def _ref_grads(sd, image, dout):
    """float64 autograd through oracle.myriad_ref.vit_forward, the GEMM weights rounded to bf16 as the kernels hold them."""
    from oracle import myriad_ref as R
    leaves = {}
    for k, t in sd.items():
        t = t.double()
        if k.endswith(("qkv.weight", "proj.weight", "fc1.weight", "fc2.weight")):
            t = t.to(BF16).double()
        leaves[k] = t.requires_grad_(True)
    out = R.vit_forward(leaves, image.double(), num_heads=16, eps=EPS)
    out.backward(dout.double())
    return out.detach(), {k: t.grad for k, t in leaves.items()}


def _check_grads(got, want):
    for n, w in want.items():
        gg = got[n].double().cpu()
        assert gg.shape == w.shape, (n, gg.shape, w.shape)
        rel = float((gg - w).norm() / (w.norm() + 1e-30))
        cos = float((gg * w).sum() / (gg.norm() * w.norm() + 1e-30))
        assert rel < 6e-2 and cos > 0.998, (n, rel, cos)


@pytest.fixture(scope="module")
def vit2():
    from myriad_amd.eva_vit import EvaViTHIP
    ops.ensure_workspace(DEV)
    sd = _vit_weights(2)
    image = _rnd((2, 3, 224, 224), 21)
    dout = _rnd((2, 257, 1408), 22, 0.1)
    ve = EvaViTHIP({k: t.to(DEV) for k, t in sd.items()}, 16, DEV)
    ref_out, ref = _ref_grads(sd, image.cpu(), dout.cpu())
    return sd, image, dout, ve, ref_out, ref


def test_vit_backward_matches_fp64_autograd(vit2):
    sd, image, dout, ve, ref_out, ref = vit2
    out = ve.forward_train(image)
    frozen = ve.forward(image)
    torch.cuda.synchronize()
    assert torch.equal(out, frozen)                                 # the training forward keeps the frozen forward's bits
    rel = float((out.double().cpu() - ref_out).norm() / ref_out.norm())
    assert rel < 2e-2, rel
    grads = ve.backward(dout)
    torch.cuda.synchronize()
    assert set(grads) == set(ref)
    _check_grads(grads, ref)


def test_vit_grad_checkpointing_is_bit_equal_and_uses_less_memory(vit2):
    sd, image, dout, ve, _, _ = vit2
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ve.forward_train(image)
    g0 = {k: t.clone() for k, t in ve.backward(dout).items()}
    torch.cuda.synchronize()
    peak0 = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ve.forward_train(image, checkpoint=True)
    g1 = ve.backward(dout)
    torch.cuda.synchronize()
    peak1 = torch.cuda.max_memory_allocated() - base
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    assert peak1 < peak0, (peak1, peak0)


def test_vit_backward_unpadded_hidden_width():
    """A hidden width that is not a multiple of 64 is zero-padded in the working weights; its gradients come back unpadded."""
    from myriad_amd.eva_vit import EvaViTHIP
    ops.ensure_workspace(DEV)
    sd = _vit_weights(1, seed=9, Hd=6100)
    image = _rnd((1, 3, 224, 224), 23)
    dout = _rnd((1, 257, 1408), 24, 0.1)
    ve = EvaViTHIP({k: t.to(DEV) for k, t in sd.items()}, 16, DEV)
    ve.forward_train(image)
    grads = ve.backward(dout)
    torch.cuda.synchronize()
    _, ref = _ref_grads(sd, image.cpu(), dout.cpu())
    _check_grads(grads, ref)


def test_vit_load_weights_after_backward_refreshes_transposes_and_leaves_the_source_alone():
    """load_weights into an encoder whose backward has built its transposed copies: the next backward equals a fresh encoder's
    built from the new weights, bit for bit, and the tensors the first encoder was built from are not written."""
    from myriad_amd.eva_vit import EvaViTHIP
    ops.ensure_workspace(DEV)
    sd_a = {k: t.to(DEV) for k, t in _vit_weights(1, seed=41).items()}
    keep = {k: t.clone() for k, t in sd_a.items()}
    sd_b = {k: t.to(DEV) for k, t in _vit_weights(1, seed=42).items()}
    image = _rnd((1, 3, 224, 224), 43)
    dout = _rnd((1, 257, 1408), 44, 0.1)
    ve = EvaViTHIP(sd_a, 16, DEV)
    ve.forward_train(image)
    ve.backward(dout)
    assert len(ve.load_weights(sd_b)) == len(sd_b)
    out = ve.forward_train(image).clone()
    got = {k: t.clone() for k, t in ve.backward(dout).items()}
    fresh = EvaViTHIP(sd_b, 16, DEV)
    want_out = fresh.forward_train(image)
    want = fresh.backward(dout)
    torch.cuda.synchronize()
    assert torch.equal(out, want_out)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    for k in keep:
        assert torch.equal(sd_a[k], keep[k]), k


# ------------------------------------------------------------------------------------------------ checkpoint keys
def test_frozen_model_loads_visual_encoder_keys():
    """A checkpoint of a run that trained the ViT holds visual_encoder.* and ln_vision.*: load_state_dict writes them into the
    frozen model's ViT (the reference's strict=False load), in place, so its output becomes the new weights' output."""
    from myriad_amd.eva_vit import EvaViTHIP
    from myriad_amd.myriad import MyriadHIP
    from myriad_amd.synthetic import SyntheticWeights, full_config
    cfg = full_config(vit_depth=2, vit_hidden=6100, qf_layers=1, llm_layers=1, vocab=1024)
    w = SyntheticWeights(cfg, DEV, seed=4, arch="myriad", big_dtype=F32)
    model = MyriadHIP(w, dict(fixed_stage=1, fixed_taskstage=0), device=DEV)
    image = _rnd((2, 3, 224, 224), 31)
    ve = model.visual_encoder
    storage = ve.blocks[0]["w1"].data_ptr(), ve.patch_w.data_ptr(), ve.cls_row.data_ptr()
    before = ve.forward(image).clone()
    new = {k: (t.float().cpu() + 0.05 * torch.randn(t.shape, generator=torch.Generator().manual_seed(len(k))))
           for k, t in _items(w, ("visual_encoder.", "ln_vision."))}
    sd = dict(model.state_dict())
    sd.update(new)
    missing = model.load_state_dict(sd, strict=False)
    assert missing == []
    after = ve.forward(image)
    fresh = EvaViTHIP({k: t.to(DEV) for k, t in new.items()}, cfg["vit_heads"], DEV).forward(image)
    torch.cuda.synchronize()
    assert not torch.equal(before, after)
    assert torch.equal(after, fresh)
    assert (ve.blocks[0]["w1"].data_ptr(), ve.patch_w.data_ptr(), ve.cls_row.data_ptr()) == storage
    assert torch.equal(model.ln_w.cpu(), new["ln_vision.weight"]) and torch.equal(model.ln_b.cpu(), new["ln_vision.bias"])


def _items(w, prefixes):
    return [(k, w[k]) for k in w.keys() if k.startswith(prefixes)]


def test_load_drops_a_pending_look_ahead_and_updates_the_captured_vit_graph():
    """A look-ahead ViT forward issued before the load is dropped, and the captured ViT graph -- which keeps reading the same
    weight storage -- replays with the loaded weights."""
    from myriad_amd.eva_vit import EvaViTHIP
    from myriad_amd.myriad import MyriadHIP
    from myriad_amd.synthetic import SyntheticWeights, full_config
    from tests import golden_utils as gu
    cfg = full_config(vit_depth=2, qf_layers=1, llm_layers=1, vocab=1024)
    w = SyntheticWeights(cfg, DEV, seed=6, arch="myriad", big_dtype=F32)
    model = MyriadHIP(w, dict(fixed_stage=1, fixed_taskstage=0), device=DEV)
    image, maps, before, after, tgt, tmask = gu.synthetic_batch(2, cfg["vocab"], seed=3)
    s = dict(image=image, anomaly_maps=maps, oneshot_anomaly_maps=maps, before_ids=before, after_ids=after, target_ids=tgt,
             target_mask=tmask)
    img = model._image_of(s)
    model.prepare_vit_graph(s)
    assert tuple(img.shape) in model._vit_graphs
    model.prefetch_vit(s)                                  # pending: replayed with the old weights
    new = {k: (t.float().cpu() + 0.05 * torch.randn(t.shape, generator=torch.Generator().manual_seed(len(k))))
           for k, t in _items(w, ("visual_encoder.",))}
    model.load_state_dict(new, strict=False)
    assert model._vit_rest is None and model._vit_prefetched is None
    assert model._take_prefetched_vit(s) is None
    model.prefetch_vit(s)
    model._prefetch_vit_rest()
    out = model._take_prefetched_vit(s)
    fresh = EvaViTHIP({k: t.to(DEV) for k, t in new.items()}, cfg["vit_heads"], DEV).forward(img)
    torch.cuda.synchronize()
    assert torch.equal(out, fresh)
