"""Cost of freeze_vit: False on one MI355X, one process, one JSON line per measurement:

  refresh    the fp32 master -> bf16 working copy + transposed copy of all 39 x 4 ViT matrices: the one-pass batched kernel
             (ops.RefreshTable, 8 bytes per weight, one launch) against the launches it replaces (mh_cast_f32_to_bf16 +
             mh_transpose_to_bf16 per matrix, 10 bytes per weight), alternating A/B in this process, median of --rounds;
  step       train_step ms at bench.py's shape (Myriad stage 1, batch 8, full-size synthetic weights): ViT frozen (with its
             look-ahead), freeze_vit: False, and freeze_vit: False with use_grad_checkpoint; median of --rounds runs of --steps
             timed steps each, and the peak device memory of each configuration;
  drop_path  (--drop-path R [R ...]) train_step ms with freeze_vit: False at drop_path_rate 0 and at every R, one model each in
             this process, their rounds interleaved (rate 0, R1, R2, ..., rate 0, ...), median of --rounds; with the share of
             branch rows the ViT ran (EvaViTHIP.last_drop_stats summed over the timed steps) and the branches it skipped.

    python tools/vit_finetune_bench.py [--batch 8] [--steps 30] [--rounds 5] [--skip-refresh] [--skip-step] [--drop-path 0.1 0.2 0.4]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
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


def bench_refresh(rounds, reps=5, depth=39, D=1408, Hd=6144):
    shapes = [(3 * D, D), (D, D), (Hd, D), (D, Hd)] * depth
    n = sum(r * c for r, c in shapes)
    flat = torch.empty(n, dtype=F32, device=DEV).normal_(0, 0.02)
    entries, o = [], 0
    for r, c in shapes:
        entries.append((flat[o:o + r * c].view(r, c), torch.empty((r, c), dtype=BF16, device=DEV),
                        torch.empty((c, r), dtype=BF16, device=DEV)))
        o += r * c
    table = ops.RefreshTable(entries, torch.device(DEV))

    def old():
        for src, w, wt in entries:
            ops.to_bf16(src, out=w)
            ops.transpose_to_bf16(w, pad_to=1, out=wt)
    new_ms, old_ms = [], []
    for _ in range(rounds):                                          # alternating: both see the same clocks and temperature
        new_ms.append(timed(table.run, reps))
        old_ms.append(timed(old, reps))
    t_new, t_old = statistics.median(new_ms), statistics.median(old_ms)
    return dict(bench="refresh", matrices=len(shapes), weights_m=round(n / 1e6, 1), pair_kernel_ms=round(t_new, 3),
                cast_transpose_ms=round(t_old, 3), pair_launches=1, cast_transpose_launches=2 * len(shapes),
                pair_tb_per_s=round(n * 8 / t_new / 1e9, 2), cast_transpose_tb_per_s=round(n * 10 / t_old / 1e9, 2))


def bench_step(B, steps, rounds):
    from bench import make_samples
    from myriad_amd.myriad import MyriadHIP
    from myriad_amd.synthetic import SyntheticWeights, full_config
    cfg = full_config()
    w = SyntheticWeights(cfg, DEV, seed=0)
    out = dict(bench="step", batch=B, steps=steps, rounds=rounds)
    for key, extra in (("frozen", {}), ("trainable", dict(freeze_vit=False)),
                       ("trainable_checkpoint", dict(freeze_vit=False, use_grad_checkpoint=True))):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        model = MyriadHIP(w, dict(fixed_stage=1, fixed_taskstage=0, **extra), device=DEV)
        s = make_samples(B, cfg["vocab"], 42, DEV)
        model.train()
        model.prepare_vit_graph(s)
        for _ in range(2):
            model.train_step(s, 1e-5, 0.05, next_samples=s)
        model.finish_update()
        ms = []
        for _ in range(rounds):
            ms.append(timed(lambda: model.train_step(s, 1e-5, 0.05, next_samples=s), steps))
            model.finish_update()
        out[key + "_ms"] = round(statistics.median(ms), 2)
        out[key + "_peak_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)
        del model
    return out


def bench_drop_path(B, steps, rounds, rates):
    from bench import make_samples
    from myriad_amd.myriad import MyriadHIP
    from myriad_amd.synthetic import SyntheticWeights, full_config
    cfg = full_config()
    w = SyntheticWeights(cfg, DEV, seed=0)
    s = make_samples(B, cfg["vocab"], 42, DEV)
    rates = [0.0] + [r for r in rates if r > 0]
    models, rows = [], []
    for r in rates:
        model = MyriadHIP.from_config(dict(weights=w, device=DEV, fixed_stage=1, fixed_taskstage=0, freeze_vit=False,
                                           vit_precision="fp32", drop_path_rate=r, vit_drop_path=True, drop_path_seed=1234))
        model.train()
        for _ in range(2):
            model.train_step(s, 1e-5, 0.05)
        models.append(model)
        rows.append(dict(run=0, dense=0, skipped=0, steps=0))
    ms = [[] for _ in rates]

    def step(i):
        models[i].train_step(s, 1e-5, 0.05)
        st = models[i].vit.last_drop_stats
        rows[i]["run"] += st["branch_rows_run"]
        rows[i]["dense"] += st["branch_rows_dense"]
        rows[i]["skipped"] += st["branches_skipped"]
        rows[i]["steps"] += 1
    for _ in range(rounds):                                          # interleaved: every rate sees the same clocks and temperature
        for i in range(len(rates)):
            ms[i].append(timed(lambda: step(i), steps))
    out = dict(bench="drop_path", batch=B, steps=steps, rounds=rounds)
    for i, r in enumerate(rates):
        out[f"rate_{r:g}"] = dict(median_ms=round(statistics.median(ms[i]), 2), min_ms=round(min(ms[i]), 2),
                                  max_ms=round(max(ms[i]), 2), rows_run_share=round(rows[i]["run"] / rows[i]["dense"], 4),
                                  branch_rows_per_step=rows[i]["run"] // rows[i]["steps"],
                                  branches_skipped_per_step=round(rows[i]["skipped"] / rows[i]["steps"], 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-refresh", action="store_true")
    ap.add_argument("--drop-path", type=float, nargs="+", default=None, metavar="R",
                    help="also time the trainable step at drop_path_rate 0 and at these rates, interleaved in this process")
    a = ap.parse_args()
    ops.ensure_workspace(torch.device(DEV))
    if not a.skip_refresh:
        print(json.dumps(bench_refresh(a.rounds)), flush=True)
    if not a.skip_step:
        print(json.dumps(bench_step(a.batch, a.steps, a.rounds)), flush=True)
    if a.drop_path:
        print(json.dumps(bench_drop_path(a.batch, a.steps, a.rounds, a.drop_path)), flush=True)


if __name__ == "__main__":
    main()
