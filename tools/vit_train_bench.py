"""Cost of training the EVA ViT on one MI355X (one JSON line per measurement):

  ln_bwd     ops.gemm_layernorm_bwd (dgrad GEMM + LayerNorm backward + its parameter gradients) against the unfused launches
             (gemm f32 + layernorm_bwd + layernorm_param_grads) at the ViT's two shapes, M = batch * 257, N = 1408,
             K = 4224 (LN1, after the qkv dgrad) and 6144 (LN2, after the fc1 dgrad);
  vit        EvaViTHIP at full width (random weights, --depth blocks, default the full 39): the frozen forward, the training
             forward, the backward, with and without per-block recomputation (checkpoint), and the peak memory of each;
  vit_bwd_parts  one block's backward launches timed by kind at the same shapes (weight gradients, dgrad GEMMs with their
             fused epilogues / LayerNorm backwards, the attention backward), times the depth; `rest` is what the measured
             backward spends beyond them (casts, bias-third copies, the embedding, launch gaps).

    python tools/vit_train_bench.py [--batch 8] [--depth 39] [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from myriad_amd import ops  # noqa: E402
from myriad_amd.eva_vit import EvaViTHIP  # noqa: E402

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def bench_ln_bwd(B, reps):
    M, N = B * 257, 1408
    for K in (4224, 6144):
        a = (torch.randn((M, K), device=DEV) * 0.5).to(BF16)
        b = (torch.randn((N, K), device=DEV) * 0.05).to(BF16)
        x = torch.randn((M, N), device=DEV)
        w = torch.randn((N,), device=DEV) * 0.1 + 1
        dres = torch.randn((M, N), device=DEV)
        dg, db = torch.empty(N, device=DEV), torch.empty(N, device=DEV)

        def fused():
            ops.gemm_layernorm_bwd(a, b, x, w, 1e-6, dres=dres, dgamma=dg, dbeta=db)

        def unfused():
            dy = ops.gemm(a, b, out_dtype=F32)
            ops.layernorm_bwd(dy, x, w, 1e-6, dres=dres, want_f32=True, want_bf16=True)
            ops.layernorm_param_grads(dy, x, 1e-6, dg, db)

        kern, splits = ops.gemm_plan(M, N, K, out_f32=True)
        print(json.dumps(dict(what="ln_bwd", M=M, N=N, K=K, kernel=kern, splits=splits, fused_us=round(1e3 * timed(fused, reps * 20), 1),
                              unfused_us=round(1e3 * timed(unfused, reps * 20), 1))), flush=True)


def vit_weights(depth, D=1408, Hd=6144, P=14, ntok=257):
    v = "visual_encoder."

    def n(*shape, s=0.02, m=0.0):
        return torch.randn(shape, device=DEV) * s + m

    sd = {v + "cls_token": n(1, 1, D), v + "pos_embed": n(1, ntok, D), v + "patch_embed.proj.weight": n(D, 3, P, P),
          v + "patch_embed.proj.bias": n(D)}
    for i in range(depth):
        p = v + f"blocks.{i}."
        sd.update({p + "norm1.weight": n(D, m=1.0), p + "norm1.bias": n(D), p + "attn.qkv.weight": n(3 * D, D),
                   p + "attn.q_bias": n(D), p + "attn.v_bias": n(D), p + "attn.proj.weight": n(D, D),
                   p + "attn.proj.bias": n(D), p + "norm2.weight": n(D, m=1.0), p + "norm2.bias": n(D),
                   p + "mlp.fc1.weight": n(Hd, D), p + "mlp.fc1.bias": n(Hd), p + "mlp.fc2.weight": n(D, Hd),
                   p + "mlp.fc2.bias": n(D)})
    return sd


def bench_vit(B, depth, reps):
    ve = EvaViTHIP(vit_weights(depth), 16, DEV)
    image = torch.randn((B, 3, 224, 224), device=DEV)
    dout = torch.randn((B, 257, 1408), device=DEV) * 1e-3
    grads = {k: torch.empty(s, dtype=F32, device=DEV) for k, s in ve.grad_shapes().items()}
    res = dict(what="vit", batch=B, depth=depth, params_M=round(sum(g.numel() for g in grads.values()) / 1e6, 1))
    res["frozen_fwd_ms"] = round(timed(lambda: ve.forward(image), reps), 3)
    for ck in (False, True):
        tag = "_ckpt" if ck else ""
        res["train_fwd" + tag + "_ms"] = round(timed(lambda: (ve.forward_train(image, checkpoint=ck), setattr(ve, "_ctx", None)),
                                                     reps), 3)

        def step():
            ve.forward_train(image, checkpoint=ck)
            ve.backward(dout, grads)

        res["fwd_bwd" + tag + "_ms"] = round(timed(step, reps), 3)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        res["peak_extra" + tag + "_GiB"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 2)
    res["bwd_ms"] = round(res["fwd_bwd_ms"] - res["train_fwd_ms"], 3)
    res["bwd_ckpt_ms"] = round(res["fwd_bwd_ckpt_ms"] - res["train_fwd_ckpt_ms"], 3)
    print(json.dumps(res), flush=True)
    bench_bwd_parts(ve, image, dout, grads, depth, reps, res["bwd_ms"])


def bench_bwd_parts(ve, image, dout, grads, depth, reps, bwd_ms):
    ve.forward_train(image)
    s, ve._ctx = ve._ctx["saved"][0], None
    blk, T, pre = ve.blocks[0], ve._T[0], ve.prefix + "blocks.0."
    B, N, D = dout.shape
    M = B * N
    dh = dout.reshape(M, D)
    dhb = ops.to_bf16(dh)
    dpre = ops.gemm_gelu_bwd(dhb, T["w2"], s["pre"])
    dh_mid, dh_mid_b = ops.gemm_layernorm_bwd(dpre, T["w1"], s["h_mid"], blk["n2w"], ve.eps, dres=dh)
    do = ops.gemm(dh_mid_b, T["wproj"]).view(B, N, D)
    qkv = s["qkv"]
    dqkv = torch.empty((M, 3 * D), dtype=BF16, device=DEV)
    d3 = dqkv.view(B, N, 3 * D)
    gq = torch.empty((3 * D,), dtype=F32, device=DEV)
    g = {k: grads[pre + k] for k in ("mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "attn.proj.weight",
                                     "attn.proj.bias", "attn.qkv.weight", "norm1.weight", "norm1.bias", "norm2.weight",
                                     "norm2.bias")}

    def wgrad():
        ops.gemm_tn_wgrad(dhb, s["a"], g["mlp.fc2.weight"], bias=g["mlp.fc2.bias"])
        ops.gemm_tn_wgrad(dpre, s["xn2"], g["mlp.fc1.weight"], bias=g["mlp.fc1.bias"])
        ops.gemm_tn_wgrad(dh_mid_b, s["o"].view(M, D), g["attn.proj.weight"], bias=g["attn.proj.bias"])
        ops.gemm_tn_wgrad(dqkv, s["xn1"], g["attn.qkv.weight"], bias=gq)

    def dgrad():
        ops.gemm_gelu_bwd(dhb, T["w2"], s["pre"])
        ops.gemm_layernorm_bwd(dpre, T["w1"], s["h_mid"], blk["n2w"], ve.eps, dres=dh, dgamma=g["norm2.weight"],
                               dbeta=g["norm2.bias"])
        ops.gemm(dh_mid_b, T["wproj"])
        ops.gemm_layernorm_bwd(dqkv, T["wqkv"], s["h_in"], blk["n1w"], ve.eps, dres=dh_mid, dgamma=g["norm1.weight"],
                               dbeta=g["norm1.bias"])

    def attn():
        ops.attn_bwd(qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:], s["o"], do, s["lse"], ve.H, ve.hd, ve.hd ** -0.5,
                     dq=d3[:, :, :D], dk=d3[:, :, D:2 * D], dv=d3[:, :, 2 * D:])

    parts = {k: timed(f, reps * 4) * depth for k, f in (("wgrad", wgrad), ("dgrad", dgrad), ("attn_bwd", attn))}
    out = dict(what="vit_bwd_parts", depth=depth, **{k + "_ms": round(v, 3) for k, v in parts.items()})
    out["rest_ms"] = round(bwd_ms - sum(parts.values()), 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--depth", type=int, default=39)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    ops.ensure_workspace(DEV)
    bench_ln_bwd(args.batch, args.reps)
    bench_vit(args.batch, args.depth, args.reps)


if __name__ == "__main__":
    main()
