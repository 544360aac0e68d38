"""freeze_vit: False on the MI355X: the master -> working-copy refresh kernel bit for bit, the model's ViT / ln_vision gradients
against torch autograd through the oracle, the update against float64 torch.optim.AdamW, and what must not move (the frozen
bits, the look-ahead-free schedule, gradient checkpointing, accumulation, the checkpoint round trip)."""
import pytest
import torch

from myriad_amd import ops
from tests import fp64_bounds as fb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------ the refresh kernel
def _bordered(rows, cols, ld, dtype=BF16, border=4):
    """A poisoned [rows + 2 border, ld + 2 border] buffer and its [rows, ld] window (row stride of the buffer; a border of 4
    keeps a window whose ld is a multiple of 4 on the kernel's 8-byte store path)."""
    buf = fb.poisoned((rows + 2 * border, ld + 2 * border), dtype, DEV)
    return buf, buf[border:border + rows, border:border + ld]


def _cast(src):
    """ops.to_bf16 of the source (the library's cast takes multiples of four elements: zero-padded behind the last)."""
    n = src.numel()
    flat = torch.cat([src.reshape(-1), torch.zeros((-n) % 4, dtype=F32, device=src.device)])
    return ops.to_bf16(flat)[:n].view(src.shape)


def _check_pair(src, ld_dst, ld_t, want_dst=True, want_t=True):
    R, C = src.shape
    want = _cast(src)
    bd, wd = _bordered(R, C, ld_dst) if want_dst else (None, None)
    bt, wt = _bordered(C, R, ld_t) if want_t else (None, None)
    return want, (bd, wd), (bt, wt)


def _assert_pair(src, want, d, t, what):
    R, C = src.shape
    (bd, wd), (bt, wt) = d, t
    if wd is not None:
        assert torch.equal(wd[:, :C].view(torch.int16), want.view(torch.int16)), f"{what}: row-major copy"
        fb.assert_frame_untouched(bd, slice(4, 4 + R), slice(4, 4 + C), f"{what}: row-major")     # padding and border
    if wt is not None:
        assert torch.equal(wt[:, :R].view(torch.int16), want.t().contiguous().view(torch.int16)), f"{what}: transposed copy"
        fb.assert_frame_untouched(bt, slice(4, 4 + C), slice(4, 4 + R), f"{what}: transposed")


SHAPES = [(4224, 1408, 1408, 4224), (1408, 1408, 1408, 1408), (6144, 1408, 1408, 6144), (1408, 6144, 6144, 1408),
          (1408, 588, 640, 1408),                                   # patch_w: K = 588 into a 640-wide destination
          (837, 192, 192, 896), (192, 837, 896, 192),               # a tiny config's padded hidden width, odd strides
          (100, 70, 70, 100), (3, 200, 256, 5), (130, 7, 9, 131), (1, 1, 1, 1), (64, 64, 64, 64), (65, 129, 130, 67)]


@pytest.mark.parametrize("R,C,ld_dst,ld_t", SHAPES)
def test_refresh_pair_equals_cast_and_transpose_bit_for_bit(R, C, ld_dst, ld_t):
    src = (fb.rnd(R, C, seed=R * 7 + C) * 0.05).to(DEV)
    src.view(-1)[::97] *= 1e-38                                    # denormal results round like the cast kernel's
    want, d, t = _check_pair(src, ld_dst, ld_t)
    ops.refresh_bf16_pair(src, d[1], t[1])
    torch.cuda.synchronize()
    _assert_pair(src, want, d, t, f"{R}x{C}")


@pytest.mark.parametrize("which", ["dst", "dst_t"])
def test_refresh_pair_with_one_destination(which):
    src = fb.rnd(200, 136, seed=5).to(DEV)
    want, d, t = _check_pair(src, 136, 200, want_dst=which == "dst", want_t=which == "dst_t")
    ops.refresh_bf16_pair(src, d[1], t[1])
    torch.cuda.synchronize()
    _assert_pair(src, want, d, t, which)


def test_refresh_table_of_many_matrices_in_one_launch():
    shapes = [(256, 192, 192, 256), (100, 70, 72, 104), (64, 64, 64, 64), (1, 300, 300, 1), (837, 192, 192, 896), (5, 5, 8, 8)]
    flat = fb.rnd(sum(-(-r * c // 4) * 4 for r, c, _, _ in shapes), seed=11).to(DEV)      # masters side by side, 16-byte aligned
    entries, checks, o = [], [], 0
    for i, (R, C, ld, ldt) in enumerate(shapes):
        src = flat[o:o + R * C].view(R, C)
        o += -(-R * C // 4) * 4
        want, d, t = _check_pair(src, ld, ldt, want_t=i != 2)
        entries.append((src, d[1], t[1]))
        checks.append((src, want, d, t))
    table = ops.RefreshTable(entries, torch.device(DEV))
    assert table.n == len(shapes) and table.tiles == sum(-(-r // 64) * -(-c // 64) for r, c, _, _ in shapes)
    table.run()
    torch.cuda.synchronize()
    for i, (src, want, d, t) in enumerate(checks):
        _assert_pair(src, want, d, t, f"matrix {i}")
    flat.mul_(-3.0)                                                # the same table follows the masters
    table.run()
    torch.cuda.synchronize()
    for i, (src, _, d, t) in enumerate(checks):
        _assert_pair(src, _cast(src), d, t, f"matrix {i} after an update")


def test_refresh_table_rejects_a_short_destination():
    src = fb.rnd(64, 64, seed=1).to(DEV)
    with pytest.raises(Exception):
        ops.RefreshTable([(src, torch.empty((64, 128), dtype=BF16, device=DEV)[:, :60], None)], torch.device(DEV))


# ------------------------------------------------------------------------------------------------ model
def _tiny(arch="myriad", seed=7, freeze_vit=False, depth=2, **extra):
    from myriad_amd.myriad import MiniGPT4HIP, MyriadHIP
    from myriad_amd.synthetic import SyntheticWeights, full_config
    cfg = full_config(vit_depth=depth, qf_layers=2, llm_layers=1, vocab=1024)
    w = SyntheticWeights(cfg, DEV, seed=seed, arch=arch, big_dtype=F32)
    cls = MyriadHIP if arch == "myriad" else MiniGPT4HIP
    model = cls(w, dict(fixed_stage=1, fixed_taskstage=0, freeze_vit=freeze_vit, **extra), device=DEV)
    return cfg, w, model


def _samples(vocab, seed=3):
    from tests import golden_utils as gu
    image, maps, before, after, tgt, tmask = gu.synthetic_batch(2, vocab, seed=seed)
    return dict(image=image, anomaly_maps=maps, oneshot_anomaly_maps=maps, before_ids=before, after_ids=after,
                target_ids=tgt, target_mask=tmask)


def _vit_names(model):
    return [n for n, _, _ in model.store.specs if n.startswith(("visual_encoder.", "ln_vision."))]


@pytest.mark.parametrize("arch", ["myriad", "mini_gpt4"])
def test_vit_gradients_match_torch_autograd_through_the_oracle(arch):
    """Every visual_encoder.* and ln_vision.* gradient of one training backward (ViT depth 2) against
    oracle.myriad_ref.model_forward under torch autograd with those tensors as leaves: relative error < 6e-2, cosine > 0.998,
    per tensor, none skipped."""
    from oracle import myriad_ref as R
    cfg, w, model = _tiny(arch)
    s = _samples(cfg["vocab"])
    model.train()
    loss = model(s)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    names = _vit_names(model)
    assert len(names) == 4 + 2 * 13 + 2
    sd = {k: w[k].float().cpu() for k in w.keys()}
    leaves = {n: sd[n].clone().requires_grad_(True) for n in names}
    sd.update(leaves)
    ref = R.model_forward(sd, s["image"], s["anomaly_maps"] if arch == "myriad" else None, 1, s["before_ids"],
                          s["after_ids"], s["target_ids"], s["target_mask"], arch=arch)
    assert abs(float(loss.detach()) - float(ref.detach())) / abs(float(ref.detach())) < 5e-3
    ref.backward()
    bad = []
    for n in names:
        got, want = model.store.g[n].double().cpu().reshape(-1), leaves[n].grad.double().reshape(-1)
        rel = float((got - want).norm() / (want.norm() + 1e-30))
        cos = float((got * want).sum() / (got.norm() * want.norm() + 1e-30))
        print(f"{arch} {n}: rel {rel:.3e} cos {cos:.6f}")
        if not (rel < 6e-2 and cos > 0.998):
            bad.append((n, rel, cos))
        assert model._params[n].grad is not None                 # the torch-optimiser bridge sees the .grad view
    assert not bad, bad


@pytest.mark.parametrize("arch", ["myriad", "mini_gpt4"])
def test_nothing_else_moves(arch):
    """Equal weights: the trainable model's first training loss is the frozen model's, bit for bit, and so is every gradient
    outside the ViT and ln_vision."""
    cfg, _, frozen = _tiny(arch, freeze_vit=True)
    _, _, train = _tiny(arch)
    s = _samples(cfg["vocab"])
    out = []
    for m in (frozen, train):
        m.train()
        loss = m(s)["loss"]
        loss.backward()
        torch.cuda.synchronize()
        out.append(float(loss.detach()))
    assert out[0] == out[1]
    assert not frozen.train_vit and train.train_vit
    for n, _, _ in frozen.store.specs:
        assert torch.equal(frozen.store.g[n], train.store.g[n]), n
        assert float(frozen.store.g[n].abs().max()) > 0, n
    assert set(n for n, _, _ in train.store.specs) - set(n for n, _, _ in frozen.store.specs) == set(_vit_names(train))


def _working_copies_follow_the_masters(model, ptrs=None):
    ve, P, pre = model.vit, model.store.p, "visual_encoder."
    D = ve.D
    K = ve.C * ve.P * ve.P
    got_ptrs = []
    assert torch.equal(ve.patch_w[:, :K], P[pre + "patch_embed.proj.weight"].view(D, K).to(BF16))
    assert not bool(ve.patch_w[:, K:].any())
    got_ptrs.append(ve.patch_w.data_ptr())
    cls, pos = P[pre + "cls_token"].view(1, D), P[pre + "pos_embed"].view(-1, D)
    assert torch.equal(ve.cls_row, cls + pos[:1]) and torch.equal(ve.pos_patches, pos[1:])
    got_ptrs.append(ve.cls_row.data_ptr())
    for i, blk in enumerate(ve.blocks):
        b, Hd = pre + f"blocks.{i}.", blk["Hd"]
        T = ve._T[i]
        for key, name in (("wqkv", "attn.qkv.weight"), ("wproj", "attn.proj.weight")):
            want = P[b + name].to(BF16)
            assert torch.equal(blk[key], want) and torch.equal(T[key], want.t().contiguous()), (i, key)
        w1, w2 = P[b + "mlp.fc1.weight"].to(BF16), P[b + "mlp.fc2.weight"].to(BF16)
        assert torch.equal(blk["w1"][:Hd], w1) and not bool(blk["w1"][Hd:].any())
        assert torch.equal(blk["w2"][:, :Hd], w2) and not bool(blk["w2"][:, Hd:].any())
        assert torch.equal(T["w1"][:, :Hd], w1.t().contiguous()) and not bool(T["w1"][:, Hd:].any())
        assert torch.equal(T["w2"][:Hd], w2.t().contiguous()) and not bool(T["w2"][Hd:].any())
        want_b = torch.cat([P[b + "attn.q_bias"], torch.zeros(D, device=DEV), P[b + "attn.v_bias"]])
        assert torch.equal(blk["bqkv"], want_b)
        assert torch.equal(blk["b1"][:Hd], P[b + "mlp.fc1.bias"]) and not bool(blk["b1"][Hd:].any())
        for key, name in (("n1w", "norm1.weight"), ("n1b", "norm1.bias"), ("bproj", "attn.proj.bias"), ("n2w", "norm2.weight"),
                          ("n2b", "norm2.bias"), ("b2", "mlp.fc2.bias")):
            assert torch.equal(blk[key], P[b + name]), (i, key)
        got_ptrs += [blk[k].data_ptr() for k in ("wqkv", "wproj", "w1", "w2", "bqkv", "b1")] + [T[k].data_ptr() for k in T]
    if ptrs is not None:
        assert got_ptrs == ptrs
    return got_ptrs


def test_two_adamw_steps_match_torch_adamw_and_refresh_every_working_copy():
    from myriad_amd.myriad import uses_weight_decay
    cfg, w, model = _tiny("myriad", seed=9)
    s = _samples(cfg["vocab"])
    model.train()
    st = model.store
    names = _vit_names(model)
    ptrs = _working_copies_follow_the_masters(model)              # the copies exist from bind time
    ref = {n: torch.nn.Parameter(st.p[n].detach().double().cpu().clone()) for n in names}
    wd = [n for n in names if uses_weight_decay(n, len(st.ref_shape[n]))]
    opt = torch.optim.AdamW([{"params": [ref[n] for n in wd], "weight_decay": 0.05},
                             {"params": [ref[n] for n in names if n not in wd], "weight_decay": 0.0}], lr=1e-3)
    v0 = st.version
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
            assert not torch.equal(got, w[n].double().cpu().reshape(got.shape)), n     # it moved
    assert st.version > v0
    assert st.module_steps()["visual_encoder"] == 2 and st.module_steps()["ln_vision"] == 2
    model.eval()
    with torch.no_grad():
        model(s)                                                  # a forward rewrites the working copies from the masters
    torch.cuda.synchronize()
    _working_copies_follow_the_masters(model, ptrs)
    assert model.ln_w.data_ptr() == st.p["ln_vision.weight"].data_ptr()


def test_next_samples_changes_nothing_with_a_trainable_vit():
    cfg, _, a = _tiny("myriad", seed=5)
    _, _, b = _tiny("myriad", seed=5)
    batches = [_samples(cfg["vocab"], seed=20 + i) for i in range(4)]
    la, lb = [], []
    a.train(); b.train()
    for i in range(3):
        la.append(float(a.train_step(batches[i], lr=1e-3)))
        lb.append(float(b.train_step(batches[i], lr=1e-3, next_samples=batches[i + 1])))
    a.finish_update(); b.finish_update()
    torch.cuda.synchronize()
    assert la == lb
    for k in ("flat_p", "flat_m", "flat_v"):
        assert torch.equal(getattr(a.store, k), getattr(b.store, k)), k
    assert b._vit_prefetched is None and b._vit_rest is None and not b._vit_graphs


def test_grad_checkpoint_gives_the_same_gradients():
    cfg, _, a = _tiny("myriad", seed=4)
    _, _, b = _tiny("myriad", seed=4, use_grad_checkpoint=True)
    assert b.vit_checkpoint and not a.vit_checkpoint
    s = _samples(cfg["vocab"])
    losses = []
    for m in (a, b):
        m.train()
        loss = m(s)["loss"]
        loss.backward()
        torch.cuda.synchronize()
        losses.append(float(loss.detach()))
    assert losses[0] == losses[1] and torch.equal(a.store.flat_g, b.store.flat_g)
    assert b.vit._ctx is None


def test_accumulation_and_the_torch_optimiser_bridge():
    """accum_grad_iters = 2: two train_steps == one AdamW on g1 + g2 (the form of tests/test_dp_gpu.py); loss.backward() hands a
    torch optimiser non-None .grad views for the two new modules."""
    cfg, _, got = _tiny("myriad", seed=6)
    _, _, ref = _tiny("myriad", seed=6)
    batches = [_samples(cfg["vocab"], seed=30 + i) for i in range(2)]
    got.train(); ref.train()
    for i in range(2):
        got.train_step(batches[i], 1e-3, 0.05, accum_grad_iters=2)
    got.finish_update()
    st = ref.store
    gsum = None
    for i in range(2):
        with torch.no_grad():
            ref._forward_impl(batches[i], True)
            ref.backward()
        torch.cuda.synchronize()
        g = st.flat_g_comm.clone()
        gsum = g if gsum is None else g + gsum
    st.flat_g_comm.copy_(gsum)
    st.adamw_step(1e-3, 0.05)
    torch.cuda.synchronize()
    for k in ("flat_p", "flat_m", "flat_v"):
        assert torch.equal(getattr(got.store, k), getattr(st, k)), k
    assert got.store.module_steps() == st.module_steps() and st.module_steps()["visual_encoder"] == 1
    # the bridge, with a loss scale: the gradients are the unscaled ones times the scale
    _, _, m = _tiny("myriad", seed=6)
    m.train()
    (m(batches[0])["loss"] * 4.0).backward()
    torch.cuda.synchronize()
    names = _vit_names(m)
    assert all(m._params[n].grad is not None and m._params[n].grad.data_ptr() == m.store.g[n].data_ptr() for n in names)
    _, _, m1 = _tiny("myriad", seed=6)
    m1.train()
    m1(batches[0])["loss"].backward()
    torch.cuda.synchronize()
    for n in names:
        assert torch.equal(m.store.g[n], m1.store.g[n] * 4.0), n   # a power of two: exact
    opt = torch.optim.AdamW([m1._params[n] for n in names], lr=1e-3)
    before = m1.store.p["visual_encoder.blocks.1.mlp.fc2.weight"].clone()
    opt.step()
    assert not torch.equal(before, m1.store.p["visual_encoder.blocks.1.mlp.fc2.weight"])


def test_state_dict_round_trip_into_frozen_and_trainable_models():
    cfg, w, model = _tiny("myriad", seed=8)
    s = _samples(cfg["vocab"])
    model.train()
    for _ in range(2):
        model.train_step(s, lr=1e-3)
    model.finish_update()
    sd = model.state_dict()
    shapes = model.vit.grad_shapes()
    for n in _vit_names(model):
        assert n in sd and tuple(sd[n].shape) == tuple(shapes.get(n, (model.Dv,))), n
        assert torch.equal(sd[n], model.store.p[n].cpu().reshape(sd[n].shape))
    assert tuple(sd["visual_encoder.patch_embed.proj.weight"].shape) == (model.Dv, 3, 14, 14)
    model.eval()
    with torch.no_grad():
        want_loss = float(model(s)["loss"])
    want_ids = model.generate(s, max_new_tokens=6)["token_ids"]
    # into a fresh FROZEN model: the same eval loss and ids
    _, _, frozen = _tiny("myriad", seed=8, freeze_vit=True)
    frozen.load_state_dict(sd)
    frozen.eval()
    with torch.no_grad():
        assert float(frozen(s)["loss"]) == want_loss
    got_ids = frozen.generate(s, max_new_tokens=6)["token_ids"]
    assert [list(map(int, r)) for r in got_ids] == [list(map(int, r)) for r in want_ids]
    # into a fresh trainable model: the masters, exactly; a key that is missing is reported
    _, _, fresh = _tiny("myriad", seed=8)
    assert fresh.load_state_dict(sd) == []
    assert torch.equal(fresh.store.flat_p[:fresh.store.n_used], model.store.flat_p[:model.store.n_used])
    fresh.eval()
    with torch.no_grad():
        assert float(fresh(s)["loss"]) == want_loss
    short = {k: v for k, v in sd.items() if k != "ln_vision.bias"}
    assert fresh.load_state_dict(short) == ["ln_vision.bias"]
