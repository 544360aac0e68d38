"""Cost of freeze_qformer: False on one MI355X, three measurements (one JSON line each):

  step       train_step ms at bench.py's shape (Myriad stage 1, batch 8, full-size synthetic weights), Q-Former frozen vs
             trainable without dropout vs trainable with the default dropout 0.1, same process, same build;
  wgrad      the Q-Former's weight-gradient products of one step (12 layers at M = B * 81 plus the cross key/value product
             over B * 257 rows): the TN kernel (ops.gemm_tn_wgrad) vs the route it replaces (two transposed bf16 copies +
             gemm_auto_f32);
  adamw      the gated AdamW over the Q-Former's ~105 M fp32 parameters.

    python tools/qformer_train_bench.py [--batch 8] [--steps 10] [--skip-step]
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


def bench_wgrad(B, reps):
    nq, D, I, Ne, We, L = 81, 768, 3072, 257, 1408, 12
    M = B * nq
    g = torch.Generator().manual_seed(0)
    shapes = []
    for i in range(L):
        shapes += [(M, 3 * D, D), (M, D, D), (M, I, D), (M, D, I)]
        if i % 2 == 0:
            shapes += [(M, D, D), (M, D, D)]
    shapes.append((B * Ne, 6 * 2 * D, We))
    ops_in = []
    for (m, n, k) in shapes:
        dy = (torch.randn(m, n, generator=g) * 0.1).to(DEV, BF16)
        x = torch.randn(m, k, generator=g).to(DEV, BF16)
        ops_in.append((dy, x, torch.empty((n, k), dtype=F32, device=DEV)))

    def tn():
        for dy, x, out in ops_in:
            ops.gemm_tn_wgrad(dy, x, out)

    def nt():
        for dy, x, out in ops_in:
            ops.gemm_auto_f32(ops.transpose_to_bf16(dy, 64), ops.transpose_to_bf16(x, 64), out)
    flop = sum(2.0 * m * n * k for m, n, k in shapes)
    t_tn, t_nt = timed(tn, reps), timed(nt, reps)
    return dict(bench="wgrad", batch=B, products=len(shapes), gflop=round(flop / 1e9, 1), tn_ms=round(t_tn, 3),
                transpose_nt_ms=round(t_nt, 3), tn_tflops=round(flop / t_tn / 1e9, 1))


def bench_adamw(reps):
    from myriad_amd.myriad import ParamStore
    from myriad_amd.qformer import qformer_param_specs
    from myriad_amd.synthetic import full_config, shape_table
    cfg = full_config(vit_depth=1, llm_layers=1)
    sd = {n: torch.empty(s, device="meta") for n, (s, _) in shape_table(cfg, "myriad").items()}
    st = ParamStore(qformer_param_specs(sd), DEV)
    st.flat_g.normal_()
    st.used.fill_(1.0)
    t = timed(lambda: st.adamw_step(1e-4, 0.05), reps)
    n = st.n_params()
    return dict(bench="adamw", params_m=round(n / 1e6, 1), ms=round(t, 3), gbytes=round(n * 7 * 4 / 1e9, 2),
                tb_per_s=round(n * 7 * 4 / t / 1e9, 2))


def bench_step(B, steps):
    sys.path.insert(0, ROOT)
    from bench import make_samples
    from myriad_amd.myriad import MyriadHIP
    from myriad_amd.synthetic import SyntheticWeights, full_config
    cfg = full_config()
    w = SyntheticWeights(cfg, DEV, seed=0)
    out = dict(bench="step", batch=B, steps=steps)
    for key, extra in (("frozen_ms", {}), ("trainable_ms", dict(freeze_qformer=False, qformer_dropout=0.0)),
                       ("trainable_dropout_ms", dict(freeze_qformer=False))):
        model = MyriadHIP(w, dict(fixed_stage=1, fixed_taskstage=0, **extra), device=DEV)
        s = make_samples(B, cfg["vocab"], 42, DEV)
        model.train()
        model.prepare_vit_graph(s)
        for _ in range(2):
            model.train_step(s, 1e-5, 0.05, next_samples=s)
        model.finish_update()
        t = timed(lambda: model.train_step(s, 1e-5, 0.05, next_samples=s), steps)
        model.finish_update()
        out[key] = round(t, 2)
        del model
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    ops.ensure_workspace(torch.device(DEV))
    print(json.dumps(bench_wgrad(a.batch, 20)), flush=True)
    print(json.dumps(bench_adamw(20)), flush=True)
    if not a.skip_step:
        print(json.dumps(bench_step(a.batch, a.steps)), flush=True)


if __name__ == "__main__":
    main()
