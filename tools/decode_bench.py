#!/usr/bin/env python3
"""Decode throughput of the full-size model: prefill + N single-token steps with KV cache.
python tools/decode_bench.py [--batch 1] [--new 32] [--sample] [--penalty P] [--modes greedy,host,device] [--repeats 5]
--sample: the chat call's do_sample=True, top_p=0.9, top_k=50 (drawn on the device when MYRIAD_DEVICE_SAMPLING=1, else on the
host); --modes times several decodes in one process, interleaved per repeat: greedy, host (sampled, host draw), device (sampled,
device draw), beam (num_beams = --beams, which also times greedy at batch * beams: the same row count); --penalty adds
repetition_penalty to every mode but beam."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from myriad_amd.myriad import MyriadHIP
from myriad_amd.synthetic import SyntheticWeights, full_config

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--new", type=int, default=32)
ap.add_argument("--llm-layers", type=int, default=32)
ap.add_argument("--lora", type=int, default=0, help="1: PEFT LoRA r = 8 on q_proj / v_proj attached (the fine-tuned model's generate)")
ap.add_argument("--sample", action="store_true", help="do_sample=True, top_p=0.9, top_k=50")
ap.add_argument("--penalty", type=float, default=1.0, help="repetition_penalty")
ap.add_argument("--modes", default="", help="comma list of greedy / host / device, timed interleaved in one process")
ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--beams", type=int, default=4, help="num_beams of the beam mode")
a = ap.parse_args()
modes = [m for m in a.modes.split(",") if m] or ["sample" if a.sample else "greedy"]
if "beam" in modes and "greedy" in modes:
    modes.append("greedy_x%d" % a.beams)             # greedy at batch * beams rows: the beam step's row count
dev = "cuda:0"
cfg = full_config(llm_layers=a.llm_layers)
model = MyriadHIP(SyntheticWeights(cfg, dev, seed=0), dict(need_backward=False, use_lora=bool(a.lora)), device=dev)
model.eval()
g = torch.Generator().manual_seed(1)
B = a.batch


def make_samples(n):
    return dict(image=torch.randn(n, 3, 224, 224, generator=g), anomaly_maps=torch.rand(n, 1, 224, 224, generator=g),
                before_ids=torch.randint(3, 32000, (1, 4), generator=g).expand(n, -1).contiguous(),
                after_ids=torch.randint(3, 32000, (1, 28), generator=g).expand(n, -1).contiguous())


smp = make_samples(B)
smp_rows = make_samples(B * a.beams) if "beam" in modes else None
default_dev = model.llama.device_sampling


def run(n, mode):
    kw, sm = {}, smp
    if mode == "beam":
        kw = dict(num_beams=a.beams, early_stopping="never")    # no early stop: every run decodes n tokens
    elif mode.startswith("greedy_x"):
        sm = smp_rows
    elif mode != "greedy":
        kw = dict(do_sample=True, top_p=0.9, top_k=50, generator=torch.Generator().manual_seed(0))
    if mode != "beam":
        kw["repetition_penalty"] = a.penalty
    model.llama.device_sampling = {"host": False, "device": True}.get(mode, default_dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.generate(sm, max_new_tokens=n, stop_ids=((-1,),), min_length=0, eos_token_id=-5, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


for m in modes:
    run(2, m); run(6, m)                 # warm-up: kernels, then the token-step graph of this batch size is captured
res = {m: [] for m in modes}
for _ in range(a.repeats):
    for m in modes:
        t_short, _ = run(a.new // 4, m)
        t_long, out = run(a.new, m)
        n_long, n_short = out["token_ids"].shape[1], a.new // 4
        if m == "beam":
            n_long = model.last_generate_stats["steps"]       # hypotheses may end before the last step; the step count does not
        res[m].append(((t_long - t_short) / (n_long - n_short), t_long, n_long, dict(model.last_generate_stats)))
for m in modes:
    ts = sorted(r[0] for r in res[m])
    per_tok, t_long, n_long, st = res[m][-1][0], res[m][-1][1], res[m][-1][2], res[m][-1][3]
    per_tok = ts[len(ts) // 2]                        # prefill / vision cancel: pure single-token decode steps (median)
    extra = (f" [{m}: device-drawn rows {st.get('device_sampled_rows', 0)}, host-drawn {st.get('host_sampled_rows', 0)}, "
             f"graph replays {st.get('graph_replays', 0)}]" if m != "greedy" or a.penalty != 1.0 else "")
    rows = B * a.beams if m in ("beam", "greedy_x%d" % a.beams) else B
    print(f"batch {B} rows {rows}{' +LoRA' if a.lora else ''} {m}{f' penalty {a.penalty}' if a.penalty != 1.0 else ''}: {n_long} tokens in "
          f"{t_long*1e3:.1f} ms (incl. ViT+Q-Former+prefill); decode step {per_tok*1e3:.3f} ms/token (median of {len(ts)}, "
          f"min {ts[0]*1e3:.3f}, max {ts[-1]*1e3:.3f}) -> {rows / per_tok:.1f} row-tok/s steady; weight stream "
          f"{13.2e9 / per_tok / 1e12:.2f} TB/s of 6.3 achievable{extra}")
