"""Cost of max_grad_norm / skip_nonfinite on one MI355X (one JSON line each):

  step   train_step ms at bench.py's shape (Myriad stage 1, batch 8, full-size synthetic weights, LoRA, look-ahead ViT) with the
         options off and on, interleaved in ONE process on one model: `--reps` rounds (default 5) of `--steps` steps each way,
         the median round of each.  "on" pays the norm pass and loses the early tokenizer update (the update moves to the
         tail of the step, behind the norm of the whole gradient);
  norm   the norm alone on that model's store: one mh_grad_sumsq launch per module range plus mh_clip_finalize.

    python tools/grad_clip_bench.py [--batch 8] [--steps 10] [--reps 5]
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


def timed(fn, reps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from bench import make_samples
    from myriad_amd.myriad import GradClip, MyriadHIP, update_pieces
    from myriad_amd.synthetic import SyntheticWeights, full_config
    ops.ensure_workspace(torch.device(DEV))
    cfg = full_config()
    w = SyntheticWeights(cfg, DEV, seed=0)
    model = MyriadHIP(w, dict(fixed_stage=1, fixed_taskstage=0, use_lora=True), device=DEV)
    s = make_samples(a.batch, cfg["vocab"], 42, DEV)
    model.train()
    model.prepare_vit_graph(s)
    on = dict(max_grad_norm=1.0, skip_nonfinite=True)
    off_step = lambda: model.train_step(s, 1e-5, 0.05, next_samples=s)
    on_step = lambda: model.train_step(s, 1e-5, 0.05, next_samples=s, **on)
    for _ in range(2):
        off_step()
        on_step()
    t_off, t_on = [], []
    for _ in range(a.reps):
        t_off.append(timed(off_step, a.steps))
        t_on.append(timed(on_step, a.steps))
    model.finish_update()
    stats = model.grad_stats()
    print(json.dumps(dict(bench="step", batch=a.batch, steps=a.steps, reps=a.reps, off_ms=round(statistics.median(t_off), 3),
                          on_ms=round(statistics.median(t_on), 3), off_all=[round(t, 3) for t in t_off],
                          on_all=[round(t, 3) for t in t_on], grad_norm=stats["grad_norm"], skipped_steps=stats["skipped_steps"])),
          flush=True)
    st = model.store
    todo = update_pieces(st.ranges)
    clip = GradClip(1.0, True)
    norm = lambda: st._prepare_clip(todo, 1.0, clip)
    norm()
    t = [timed(norm, 50) for _ in range(a.reps)]
    n = sum(b - a_ for _, a_, b, _ in todo)
    ms = statistics.median(t)
    print(json.dumps(dict(bench="norm", elements_m=round(n / 1e6, 1), launches=len(todo) + 1, ms=round(ms, 4),
                          tb_per_s=round(n * 4 / ms / 1e9, 2))), flush=True)


if __name__ == "__main__":
    main()
