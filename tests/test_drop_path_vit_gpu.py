"""Stochastic depth through the whole trainable ViT (EvaViTHIP.forward_train(keep=...) / backward) at full width: depth 3,
224-pixel images, B = 4, an injected mask set with keep_prob = [1, 0.8, 0.6]:

    block 0   attention all          MLP all            (never drops: the dense path's fused launches)
    block 1   attention {0, 2, 3}    MLP {1}
    block 2   attention nothing      MLP all            (a skipped branch; an all-kept branch that is still scaled)

against float64 autograd through tests/drop_path_ref.vit_forward_drop, with the tolerances tests/test_vit_train_gpu.py holds the
dense path to (output rel < 2e-2; per gradient rel < 6e-2 and cos > 0.998)."""
import pytest
import torch

from myriad_amd import ops
from tests import drop_path_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
EPS = 1e-6
B, N, D, DEPTH = 4, 257, 1408, 3
KEEP_PROB = [1.0, 0.8, 0.6]
KEEP = torch.tensor([[[1, 1, 1, 1], [1, 1, 1, 1]],
                     [[1, 0, 1, 1], [0, 1, 0, 0]],
                     [[0, 0, 0, 0], [1, 1, 1, 1]]], dtype=torch.bool)
SKIPPED = tuple("visual_encoder.blocks.2." + n for n in ("norm1.weight", "norm1.bias", "attn.q_bias", "attn.v_bias",
                                                         "attn.qkv.weight", "attn.proj.weight", "attn.proj.bias"))


def _rnd(shape, seed, s=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * s).to(DEV)


def _vit_weights(depth, seed=5, Hd=6144, P=14, ntok=N):
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


@pytest.fixture(scope="module")
def vit3():
    """The encoder, its inputs and the float64 reference (computed once, on the device, shared and left unchanged)."""
    from myriad_amd.eva_vit import EvaViTHIP
    ops.ensure_workspace(DEV)
    sd = {k: t.to(DEV) for k, t in _vit_weights(DEPTH).items()}
    image, dout = _rnd((B, 3, 224, 224), 21), _rnd((B, N, D), 22, 0.1)
    ve = EvaViTHIP(sd, 16, DEV)
    leaves = {k: t.detach().to(DEV).requires_grad_(True) for k, t in ref.bf16_weights(sd).items()}
    out = ref.vit_forward_drop(leaves, image.double(), KEEP.to(DEV), KEEP_PROB, num_heads=16, eps=EPS)
    out.backward(dout.double())
    grads = {k: t.grad for k, t in leaves.items()}
    return ve, image, dout, out.detach(), grads


def test_output_and_gradients_match_fp64_autograd(vit3):
    ve, image, dout, ref_out, want = vit3
    out = ve.forward_train(image, keep=KEEP, keep_prob=KEEP_PROB)
    grads = ve.backward(dout)
    torch.cuda.synchronize()
    rel = float((out.double() - ref_out).norm() / ref_out.norm())
    print(f"output rel {rel:.3g}")
    assert rel < 2e-2, rel
    assert set(grads) == set(want)
    for n, w in want.items():
        g = grads[n].double()
        assert g.shape == w.shape, (n, g.shape, w.shape)
        if n in SKIPPED:
            assert int(torch.count_nonzero(w)) == 0, n             # the reference: no sample went through this branch
            assert int(torch.count_nonzero(grads[n])) == 0, n      # exact zeros, written by this call
            continue
        rel = float((g - w).norm() / (w.norm() + 1e-30))
        cos = float((g * w).sum() / (g.norm() * w.norm() + 1e-30))
        print(f"{n}: rel {rel:.3g} cos {cos:.6f}")
        assert rel < 6e-2 and cos > 0.998, (n, rel, cos)


def test_dropped_samples_pass_through_bit_for_bit(vit3):
    """Sample 1 is dropped by block 1's attention: block 0's output for it reaches block 1's MLP unchanged, so a run in which
    block 1's MLP and all of block 2 are dropped as well returns block 0's output for that sample."""
    ve, image, _, _, _ = vit3
    keep = KEEP.clone()
    keep[1, 1] = False
    keep[2] = False
    out = ve.forward_train(image, keep=keep, keep_prob=KEEP_PROB)
    ve._ctx = None
    from myriad_amd.eva_vit import EvaViTHIP
    first = EvaViTHIP({k: t.to(DEV) for k, t in _vit_weights(1).items()}, 16, DEV)      # the same seed: block 0's weights
    want = first.forward(image)
    torch.cuda.synchronize()
    assert torch.equal(out[1], want[1])
    assert not torch.equal(out[0], want[0])                        # sample 0 went through block 1's attention
    assert ve.last_drop_stats["branches_skipped"] == 3


def test_checkpointing_is_bit_equal(vit3):
    ve, image, dout, _, _ = vit3
    o0 = ve.forward_train(image, keep=KEEP, keep_prob=KEEP_PROB).clone()
    g0 = {k: t.clone() for k, t in ve.backward(dout).items()}
    o1 = ve.forward_train(image, checkpoint=True, keep=KEEP, keep_prob=KEEP_PROB)
    g1 = ve.backward(dout)
    torch.cuda.synchronize()
    assert torch.equal(o0, o1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_no_keep_is_the_dense_path(vit3):
    ve, image, dout, _, _ = vit3
    a = ve.forward_train(image, keep=None).clone()
    ga = {k: t.clone() for k, t in ve.backward(dout).items()}
    b = ve.forward_train(image).clone()
    gb = ve.backward(dout)
    c = ve.forward(image)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    assert ve.last_drop_stats == dict(branch_rows_run=2 * DEPTH * B * N, branch_rows_dense=2 * DEPTH * B * N, branches_skipped=0)
    with pytest.raises(ValueError):
        ve.forward_train(image, keep_prob=KEEP_PROB)


def test_stats_count_the_rows_that_ran(vit3):
    ve, image, _, _, _ = vit3
    ve.forward_train(image, keep=KEEP, keep_prob=KEEP_PROB)
    ve._ctx = None
    kept = int(KEEP.sum())                                          # 4 + 4 + 3 + 1 + 0 + 4 samples
    assert kept == 16
    assert ve.last_drop_stats == dict(branch_rows_run=kept * N, branch_rows_dense=2 * DEPTH * B * N, branches_skipped=1)


def test_keep_arguments_are_checked(vit3):
    ve, image, _, _, _ = vit3
    for keep, prob in ((KEEP.to(DEV), KEEP_PROB), (KEEP.int(), KEEP_PROB), (KEEP[:2], KEEP_PROB), (KEEP[:, :, :3], KEEP_PROB),
                       (KEEP, KEEP_PROB[:2]), (KEEP, None), (KEEP, [1.0, 0.0, 0.6]), (KEEP, [1.0, 1.2, 0.6]),
                       (KEEP, [1.0, 1.0, 0.6])):                    # keep probability 1 with a dropped sample
        with pytest.raises(ValueError):
            ve.forward_train(image, keep=keep, keep_prob=prob)
    assert ve._ctx is None


def test_accumulating_leaves_a_skipped_branch_alone(vit3):
    ve, image, dout, _, _ = vit3
    ve.forward_train(image, keep=KEEP, keep_prob=KEEP_PROB)
    g = {k: t.clone() for k, t in ve.backward(dout).items()}
    acc = {k: torch.full_like(t, 0.5) for k, t in g.items()}
    for _ in range(2):
        ve.forward_train(image, keep=KEEP, keep_prob=KEEP_PROB)
        assert ve.backward(dout, grads=acc, accumulate=True) is acc
    torch.cuda.synchronize()
    for k in g:
        if k in SKIPPED:
            assert bool((acc[k] == 0.5).all()), k                  # untouched by both calls
        else:
            assert torch.equal(acc[k], (0.5 + g[k]) + g[k]), k     # two rounded sums onto what was there
    ve.forward_train(image)
    with pytest.raises(ValueError):
        ve.backward(dout, accumulate=True)                          # nothing to add to
