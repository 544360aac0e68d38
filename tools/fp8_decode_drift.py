#!/usr/bin/env python3
"""FP8 against bf16 decode weights on the full-size synthetic LLaMA, teacher-forced: the bf16 token step's greedy ids are fed
to both kinds of step, and every step's logits are compared (max |delta logit|, relative to the step's max |logit|, and top-1
agreement).  Random weights: a sanity figure for the arithmetic, not a quality claim for a trained model.
python tools/fp8_decode_drift.py [--steps 64] [--batch 1] [--prompt 32] [--llm-layers 32]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from myriad_amd import ops
from myriad_amd.myriad import MyriadHIP
from myriad_amd.synthetic import SyntheticWeights, full_config

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--prompt", type=int, default=32)
ap.add_argument("--llm-layers", type=int, default=32)
a = ap.parse_args()
dev = "cuda:0"
model = MyriadHIP(SyntheticWeights(full_config(llm_layers=a.llm_layers), dev, seed=0), dict(need_backward=False), device=dev)
lm = model.llama
B, S0, D, n = a.batch, a.prompt, lm.D, a.steps
g = torch.Generator().manual_seed(2)
prompt_ids = torch.randint(3, lm.V, (B, S0), generator=g).to(dev)
emb = lm.embed[prompt_ids].float()


@torch.no_grad()
def forced_logits(fp8: bool, feed: torch.Tensor) -> torch.Tensor:
    """[B, n, V] logits of the n single-token steps fed with feed [B, n] (the prefill on bf16 weights, as in generate())."""
    lm.decode_fp8 = fp8
    lm._pack_for_decode()
    caches = [torch.zeros((B, S0 + n + 2, 2 * D), dtype=torch.bfloat16, device=dev) for _ in lm.layers]
    lm._prefill(emb, caches)                                          # fills the caches; its logits are not needed
    pos_dev = torch.full((B,), S0, dtype=torch.int32, device=dev)
    kvlen = torch.full((B,), S0 + 1, dtype=torch.int32, device=dev)
    ws = dict(caches=caches, pos=pos_dev, kvlen=kvlen, split=None, row_limit=ops.GEMV_MAX_ROWS)   # what _step_layers reads
    out = []
    for t in range(n):
        ws["x_in"] = lm.embed[feed[:, t]].float().contiguous()
        h = lm._step_layers(ws)
        out.append(ops.gemv_packed(ops.rmsnorm_fwd(h, lm.norm, lm.eps), lm._packed["lm_head"], out_dtype=torch.float32))
        pos_dev += 1
        kvlen += 1
    return torch.stack(out, 1)


lm.decode_fp8 = False
ids = lm.greedy_generate(emb, max_new_tokens=n + 1, stop_ids=(), eos_id=-5, min_length=0)   # id 0 is the prefill's pick
feed = ids[:, :n].to(dev)
lb = forced_logits(False, feed)
l8 = forced_logits(True, feed)
scale = lb.abs().amax(-1, keepdim=True)
d = (l8 - lb).abs()
agree = (l8.argmax(-1) == lb.argmax(-1)).float().mean().item()
same = torch.equal(lb.argmax(-1).cpu(), ids[:, 1:n + 1].cpu())     # the forced bf16 steps are generate()'s own steps
print(f"{a.llm_layers} layers, batch {B}, prompt {S0}, {n} teacher-forced steps: max |dlogit| {d.max().item():.4f} "
      f"(max |logit| {scale.max().item():.3f}; max relative to the step's max |logit| {(d / scale).max().item():.4f}, mean "
      f"{(d / scale).mean().item():.5f}); top-1 agreement fp8 vs bf16 {agree * 100:.1f} % of {B * n} steps; forced bf16 ids "
      f"{'equal' if same else 'DIFFER from'} generate()'s")
