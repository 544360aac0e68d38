"""`Myriad` / `MiniGPT4` model classes on the MI355X HIP path -- the drop-in boundary.

Mirror of the reference's registered model classes (minigpt4/models/myriad.py:62-517, mini_gpt4.py:14-307):
`from_config(cfg)`, `forward(samples) -> {"loss"}`, `generate(samples, **kw) -> {"token_ids", "ve_anomaly_maps"}`,
`named_parameters()` / `requires_grad`, `state_dict()` / `load_state_dict(strict=False)` with the reference's key
names, `.device`, `.train()/.eval()`.  The forward follows `Myriad.forward` (myriad.py:377-431) ->
`encode_img` (:241-272) -> `prompt_wrap` (:354-375) -> label/mask assembly (:395-421) -> LLaMA loss; every tensor
op runs in libmyriad_hip.so.  The backward is explicit (frozen ViT/Q-Former/LLaMA => dgrad only) and
is also reachable through `loss.backward()` via a thin autograd bridge so the reference's step loop
(tasks/base_task.py:236-271) works unchanged.

Out of scope here: the ImageBind vision expert.  Its outputs are inputs to this model:
`samples["anomaly_maps"]` / `samples["oneshot_anomaly_maps"]` [B,1,224,224] in [0,1].
"""
from __future__ import annotations

import numbers
import os
import random
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, ops
from .eva_vit import EvaViTHIP
from .llama import LlamaHIP
from .networks import LoraAdaptor, VENet, from_reference_layout, to_reference_layout, ve_param_specs
from .qformer import QFormerHIP, qformer_param_specs
from .registry import registry

BF16, F32 = torch.bfloat16, torch.float32


def uses_weight_decay(name: str, ndim: int) -> bool:
    """Parameter grouping of `RunnerBase.optimizer` (reference runners/runner_base.py:115-118)."""
    return not (ndim < 2 or "bias" in name or "ln" in name or "bn" in name)


MODULES = ("expert_adaptor", "VETokenizer", "VEInstructor", "llama_proj", "lora", "Qformer")
# freeze_vit: False adds two modules BEHIND those (myriad.py:134-144 trains visual_encoder.* and ln_vision.*): the flat-buffer
# layout of every earlier recipe stays as it was.  MODULE_ORDER is the order the ParamStore lays modules out in.  The two tuples
# are kept apart on purpose: MODULES is the set a model without a trainable ViT can hold, and
# tests/test_qformer_train_cpu.py pins its last entry ("Qformer"); do not merge them.
VIT_MODULES = ("visual_encoder", "ln_vision")
MODULE_ORDER = MODULES + VIT_MODULES


def module_of(name: str) -> str:
    """The top-level reference module a trainable parameter belongs to (the unit torch's AdamW skips when unused).
    `query_tokens` (a direct parameter of the reference model) is counted with the Q-Former: both are trainable exactly
    when freeze_qformer is False (myriad.py:159-165) and both are used on every step."""
    for m in MODULES[:4] + VIT_MODULES:
        if name.startswith(m + "."):
            return m
    if name.startswith("Qformer.") or name == "query_tokens":
        return "Qformer"
    if "lora_" in name:
        return "lora"
    raise KeyError(name)



def accum_update_due(calls_since_update: int, accum_grad_iters: int, accum_index=None) -> bool:
    """Whether the optimiser steps after this backward (base_task.py:262-271).  With the iteration index of the epoch the
    reference's rule `(i + 1) % accum_grad_iters == 0`; without it, every accum_grad_iters-th call."""
    n = max(int(accum_grad_iters), 1)
    if accum_index is not None:
        return (int(accum_index) + 1) % n == 0
    return calls_since_update >= n


def update_pieces(ranges, shard=None, exclude=(), skip_idx=()):
    """The slices of the flat buffers one optimiser update touches, in launch order: [(module index, lo, hi, weight decay?)] --
    every module range of `ranges`, minus the modules `skip_idx`, cut to the slices `shard` (None: everything) and with the
    spans `exclude` taken out.  ParamStore.adamw_step walks exactly this list, and norms exactly this list when it clips."""
    out = []
    for mi, a0, b0, decays in ranges:
        if mi in skip_idx:
            continue
        for lo, hi in (shard if shard is not None else [(a0, b0)]):
            a, b = max(a0, lo), min(b0, hi)
            if a >= b:
                continue
            todo = [(a, b)]
            for ex_lo, ex_hi in exclude:                      # spans adamw_pieces() already updated this step
                todo = [q for (x, y) in todo for q in ((x, min(y, ex_lo)), (max(x, ex_hi), y)) if q[0] < q[1]]
            out.extend((mi, a, b, decays) for a, b in todo)
    return out


class GradClip:
    """What ParamStore.adamw_step(clip=...) needs to clip and / or guard one update.  max_norm: clip_grad_norm_'s threshold on
    the total 2-norm of the averaged gradient (None: no clipping); skip_nonfinite: leave parameters, moments and step counts
    alone when the gradient holds an inf or a NaN; rank_sums = (rank, world, all_reduce): sharded data parallel ('rs_ag'), where
    this rank norms only the slices it owns -- all_reduce(vector) sums the world-long fp64 vector of per-rank sums in place."""

    def __init__(self, max_norm=None, skip_nonfinite: bool = False, rank_sums=None):
        if max_norm is not None and not float(max_norm) > 0.0:
            raise ValueError(f"GradClip(max_norm={max_norm!r}): a positive threshold, or None for no clipping")
        self.max_norm = None if max_norm is None else float(max_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.rank_sums = rank_sums

    @classmethod
    def of(cls, max_grad_norm=None, skip_nonfinite: bool = False):
        """train_step's two options -> a GradClip, or None when both are off (max_grad_norm None or <= 0 is off)."""
        mg = None if (max_grad_norm is None or not float(max_grad_norm) > 0.0) else float(max_grad_norm)
        return cls(mg, skip_nonfinite) if (mg is not None or skip_nonfinite) else None

    def for_dp(self, dp):
        """The same options for an update behind `dp`'s exchange: in 'rs_ag' with the per-rank sums travelling through it."""
        if dp is None or dp.world == 1 or getattr(dp, "mode", "allreduce") != "rs_ag":
            return self
        return GradClip(self.max_norm, self.skip_nonfinite, (dp.rank, dp.world, dp.allreduce_sums))


class ParamStore:
    """All trainable parameters in ONE flat fp32 buffer (+ grad, Adam m, v): a single RCCL all-reduce and a handful of
    fused AdamW launches per step.  Layout: [weight-decay group | no-decay group | per-module use flags]; inside each
    group the parameters of one reference module are contiguous, segments 16-byte aligned.

    torch.optim.AdamW (runner_base.py:132-137) skips a parameter whose .grad is None: a module that no rank used in a
    step (VEInstructor at prompt stage 0, VETokenizer at stage 2; myriad.py:378,252,265) keeps its weights, moments and
    step count.  Here every module has a device-resident use flag at the tail of the gradient buffer -- so the data-
    parallel all-reduce sums it over ranks for free -- and a device-resident step counter; the gated AdamW kernel
    (mh_adamw_gated) reads both, the host never synchronises."""

    def __init__(self, specs: List[Tuple[str, Tuple[int, ...], Tuple[int, ...]]], device):
        self.dev = torch.device(device)
        order = {m: i for i, m in enumerate(MODULE_ORDER)}
        self.modules = [m for m in MODULE_ORDER if any(module_of(s[0]) == m for s in specs)]
        midx = {m: i for i, m in enumerate(self.modules)}
        key = lambda s: order[module_of(s[0])]                    # stable: keeps each module's own order
        wd = sorted([s for s in specs if uses_weight_decay(s[0], len(s[2]))], key=key)
        nwd = sorted([s for s in specs if not uses_weight_decay(s[0], len(s[2]))], key=key)
        self.specs = wd + nwd
        self.offsets: Dict[str, Tuple[int, int]] = {}
        self.ranges: List[Tuple[int, int, int, bool]] = []        # (module index, start, end, weight decay?)
        off = 0
        for group, decays in ((wd, True), (nwd, False)):
            if not decays:
                self.n_wd = off
            for name, ishape, _ in group:
                n = 1
                for sdim in ishape:
                    n *= sdim
                self.offsets[name] = (off, n)
                mi = midx[module_of(name)]
                if self.ranges and self.ranges[-1][0] == mi and self.ranges[-1][3] == decays:
                    self.ranges[-1] = (mi, self.ranges[-1][1], off + ops.round_up(n, 4), decays)
                else:
                    self.ranges.append((mi, off, off + ops.round_up(n, 4), decays))
                off += ops.round_up(n, 4)
        # padded to a multiple of 32 elements: at 2 / 4 / 8 ranks the reduce-scatter / all-gather shards (multiples of 4
        # elements) tile the buffer exactly, so DataParallel mode 'rs_ag' never pads or copies it (the tail belongs to no
        # module range: zero gradient, never updated)
        self.n_used = off                                         # the parameters proper end here
        off = ops.round_up(off, 32)
        self.total = off
        self.moments_complete = True                              # False while Adam moments exist for this rank's shard only
        nm = len(self.modules)
        self.flat_p = torch.zeros(off, dtype=F32, device=self.dev)
        self.flat_g_comm = torch.zeros(off + ops.round_up(max(nm, 1), 4), dtype=F32, device=self.dev)   # what DP exchanges
        self.flat_g = self.flat_g_comm[:off]
        self.used = self.flat_g_comm[off:off + nm]                # per-module use count (summed over ranks by the all-reduce)
        self.steps_dev = torch.zeros(max(nm, 1), dtype=torch.int32, device=self.dev)
        self.flat_m = torch.zeros(off, dtype=F32, device=self.dev)
        self.flat_v = torch.zeros(off, dtype=F32, device=self.dev)
        self.p, self.g = {}, {}
        self.ref_shape = {}
        for name, ishape, rshape in self.specs:
            o, n = self.offsets[name]
            self.p[name] = self.flat_p[o:o + n].view(ishape)
            self.g[name] = self.flat_g[o:o + n].view(ishape)
            self.ref_shape[name] = rshape
        # gradient clipping / non-finite guard (adamw_step(clip=...)): the device control block [s, norm, apply, skipped] and
        # the fp64 partial-sum workspace of the norm, allocated on first use and then kept
        self.ctl = None
        self._norm_ws = None
        self._rank_sums = None
        self.step = 0                                             # optimiser calls so far (host)
        self.version = 0                                          # bumped by every update / load of flat_p (decode sessions)

    def n_params(self) -> int:
        return sum(n for _, n in self.offsets.values())

    def mark_used(self, used_modules) -> None:
        """Write this rank's use flags (1.0 per used module) into the tail of the gradient buffer."""
        if not self.modules:
            return
        flags = torch.tensor([1.0 if m in used_modules else 0.0 for m in self.modules], dtype=F32)
        self.used.copy_(ops.h2d(flags, self.dev))

    def module_steps(self) -> Dict[str, int]:
        """Updates applied per module so far (device -> host: checkpointing only)."""
        st = self.steps_dev.cpu().tolist()
        return {m: int(st[i]) for i, m in enumerate(self.modules)}

    def set_module_steps(self, steps: Dict[str, int]) -> None:
        host = torch.tensor([int(steps.get(m, 0)) for m in self.modules] or [0], dtype=torch.int32)
        self.steps_dev.copy_(host.to(self.dev))

    def module_range(self, module: str, decays: bool = True):
        """(start, end) of one module's contiguous run inside a weight-decay group of the flat buffers, or None."""
        if module not in self.modules:
            return None
        mi = self.modules.index(module)
        for m2, a, b, d in self.ranges:
            if m2 == mi and d == decays:
                return a, b
        return None

    def adamw_module(self, module: str, lr: float, weight_decay: float = 0.05, beta2: float = 0.999) -> None:
        """The gated AdamW of ONE module's ranges, on the current stream (single-process training: a module whose gradient is
        complete may be updated while the rest of the backward still runs; adamw_step(..., skip={module}) then leaves it out
        and bumps every module's step counter as usual)."""
        mi = self.modules.index(module)
        self.version += 1
        for m2, a, b, decays in self.ranges:
            if m2 == mi:
                ops.adamw_gated(self.flat_p[a:b], self.flat_g[a:b], self.flat_m[a:b], self.flat_v[a:b], lr,
                                weight_decay if decays else 0.0, self.used[mi:mi + 1], self.steps_dev[mi:mi + 1], beta2=beta2)

    def adamw_pieces(self, pieces, lr: float, weight_decay: float = 0.05, beta2: float = 0.999, grad_scale: float = 1.0) -> None:
        """The gated AdamW on the slices `pieces` [(lo, hi)] of the flat buffers only -- no step-counter bump: a part of the step's
        update issued early (a data-parallel segment whose exchange is complete); adamw_step(..., exclude=pieces' span) does the
        rest and bumps the counters.  Same kernel, same per-module flags and step counts as the one-shot update."""
        self.version += 1
        for mi, a0, b0, decays in self.ranges:
            for lo, hi in pieces:
                a, b = max(a0, lo), min(b0, hi)
                if a < b:
                    ops.adamw_gated(self.flat_p[a:b], self.flat_g[a:b], self.flat_m[a:b], self.flat_v[a:b], lr,
                                    weight_decay if decays else 0.0, self.used[mi:mi + 1], self.steps_dev[mi:mi + 1], beta2=beta2,
                                    grad_scale=grad_scale)

    def adamw_step(self, lr: float, weight_decay: float = 0.05, beta2: float = 0.999, grad_scale: float = 1.0, shard=None,
                   skip=(), exclude=(), clip=None):
        """torch.optim.AdamW semantics (runner_base.py:132-137), fused, on the flat buffers; modules unused on every rank
        this step are left alone (see class docstring).  `shard` = (lo, hi) or a list of such: update only those slices of the
        flat buffer (DataParallel mode 'rs_ag': each rank owns 1/world of every exchange segment's optimiser state).  `exclude`:
        spans adamw_pieces() already updated this step.  `skip`: modules adamw_module() already
        updated this step.  `clip` (a GradClip): the 2-norm of grad_scale * gradient over exactly the elements about to be
        updated is taken first, on the device (_prepare_clip), and the update runs under its verdict: scaled by
        min(1, max_norm / (norm + 1e-6)), or not at all when the guard finds a non-finite element."""
        self.step += 1
        self.version += 1
        pieces = None
        if shard is not None:
            pieces = [tuple(shard)] if isinstance(shard[0], int) else [tuple(p) for p in shard]
            if sum(hi - lo for lo, hi in pieces) < self.total:
                self.moments_complete = False                     # DataParallel.gather_state() restores it
        skip_idx = {self.modules.index(m) for m in skip if m in self.modules}
        todo = update_pieces(self.ranges, pieces, exclude, skip_idx)
        if clip is not None:
            self._prepare_clip(todo, grad_scale, clip)
        for mi, a, b, decays in todo:
            if clip is None:
                ops.adamw_gated(self.flat_p[a:b], self.flat_g[a:b], self.flat_m[a:b], self.flat_v[a:b], lr,
                                weight_decay if decays else 0.0, self.used[mi:mi + 1], self.steps_dev[mi:mi + 1], beta2=beta2,
                                grad_scale=grad_scale)
            else:
                ops.adamw_gated_ctl(self.flat_p[a:b], self.flat_g[a:b], self.flat_m[a:b], self.flat_v[a:b], lr,
                                    weight_decay if decays else 0.0, self.used[mi:mi + 1], self.steps_dev[mi:mi + 1], self.ctl,
                                    beta2=beta2)
        if self.modules:
            if clip is None:
                ops.adamw_bump(self.used, self.steps_dev)
            else:
                ops.adamw_bump_ctl(self.used, self.steps_dev, self.ctl)

    def _prepare_clip(self, todo, grad_scale: float, clip) -> None:
        """Fill the control block for the update of the pieces `todo`: one sum-of-squares launch per piece (gated by its
        module's use flag, like the update), then the one-workgroup finalise.  Sharded ('rs_ag'): this rank's sum goes into
        its slot of a world-long vector, one small sum all-reduce, and every rank finalises from the same slots in rank order."""
        if self.ctl is None:
            self.ctl = torch.zeros(4, dtype=torch.float64, device=self.dev)
        need = sum(ops.grad_sumsq_slots(b - a) for _, a, b, _ in todo)
        if self._norm_ws is None or self._norm_ws.numel() < need:
            # every module range whole is the usual case; shards and excluded spans cut ranges into more, shorter pieces
            whole = sum(ops.grad_sumsq_slots(b - a) for _, a, b, _ in self.ranges)
            self._norm_ws = torch.zeros(max(need, whole) + 64, dtype=torch.float64, device=self.dev)
        ws, off = self._norm_ws, 0
        for mi, a, b, _ in todo:
            off += ops.grad_sumsq(self.flat_g[a:b], self.used[mi:mi + 1], ws[off:])
        if clip.rank_sums is None:
            ops.clip_finalize(ws, off, None, clip.max_norm, grad_scale, clip.skip_nonfinite, self.ctl)
            return
        rank, world, all_reduce = clip.rank_sums
        if self._rank_sums is None or self._rank_sums.numel() != world:
            self._rank_sums = torch.zeros(world, dtype=torch.float64, device=self.dev)
        ops.clip_rank_sum(ws, off, self._rank_sums, rank)
        all_reduce(self._rank_sums)
        ops.clip_finalize(ws, 0, self._rank_sums, clip.max_norm, grad_scale, clip.skip_nonfinite, self.ctl)

    def grad_stats(self) -> dict:
        """The last clipped / guarded update's verdict (one small device -> host copy: logging only)."""
        if self.ctl is None:
            return {"grad_norm": None, "clip_scale": None, "applied": True, "skipped_steps": 0}
        s, norm, apply, skipped = self.ctl.cpu().tolist()
        return {"grad_norm": norm, "clip_scale": s, "applied": apply != 0.0, "skipped_steps": int(skipped)}


def init_trainable(name: str, rshape) -> torch.Tensor:
    """Fresh trainable parameter, drawn from torch's global CPU RNG with the distribution the reference's constructor uses:
    LoraAdaptorV2 N(0, 0.02) (networks.py:78-79), nn.Conv2d default (kaiming-uniform, a = sqrt(5): U(+-1/sqrt(fan_in)) for
    weight and bias, networks.py:98-127,159-189), base_prompts N(0, 1) (:189).  llama_proj (MiniGPT-4 stage 2) is an
    nn.Linear whose reset_parameters the reference disables (common/utils.py:41-47): it must come from a checkpoint."""
    import math
    if name.startswith("expert_adaptor."):
        return torch.randn(rshape) * 0.02
    if name.endswith("base_prompts"):
        return torch.randn(rshape)
    if ".meta_net." in name:
        if name.endswith(".weight"):
            fan_in = rshape[1] * rshape[2] * rshape[3]
        else:                                   # bias bound uses the layer's fan-in: recover it from the stack's geometry
            idx = int(name.split(".meta_net.")[1].split(".")[0])
            cin = {0: 1, 3: 4, 6: 16, 9: 64, 12: 256, 15: 1024}[idx]
            k = 3 if idx < 15 else (5 if name.startswith("VETokenizer.") else 1)
            fan_in = cin * k * k
        bound = 1.0 / math.sqrt(fan_in)
        return (torch.rand(rshape) * 2 - 1) * bound
    raise KeyError(f"{name}: not in the weight files and no constructor init exists (load it with `ckpt`)")


class _LossBridge(torch.autograd.Function):
    """Lets `loss.backward()` (reference base_task.py:256-259) drive the explicit HIP backward: gradients are
    written straight into the parameters' .grad views of the flat buffer (no extra copy)."""

    @staticmethod
    def forward(ctx, anchor, model, loss):
        ctx.model = model
        return loss.detach().clone()

    @staticmethod
    def backward(ctx, gout):
        # gout is the scalar the caller back-propagates (1.0, or the GradScaler's loss scale under amp=True,
        # base_task.py:256-259): the gradients are multiplied by it so that scaler.unscale_() / step() see what they expect.
        # The read-back is a host sync per step, like the reference's own loss.item() (base_task.py:276).
        ctx.model.backward(float(gout), accumulate=ctx.model._grads_live())
        return None, None, None


class MyriadHIP(nn.Module):
    """The model.  `self.vit` is the HIP vision encoder (EvaViTHIP) in every configuration: use it to reach the encoder's blocks,
    forward or backward.  `self.visual_encoder` is the same object only while the ViT is frozen; with freeze_vit: False that name
    belongs to the nn.Module node that carries the `visual_encoder.*` parameters, so that named_parameters() / an external
    optimiser see the reference's names (as `Qformer`, `ln_vision`, `expert_adaptor`, ... are parameter nodes), and it has no
    `blocks` list or `forward` of the encoder."""
    arch = "myriad"

    def __init__(self, weights, cfg: Optional[dict] = None, device="cuda:0"):
        super().__init__()
        cfg = dict(cfg or {})
        self.cfg = cfg
        self._dev = torch.device(device)
        self.max_txt_len = cfg.get("max_txt_len", 160)
        self.end_sym = cfg.get("end_sym", "###")
        self.k_shot = cfg.get("k_shot", 0)
        # generate_stream's decode slots: positions (prompt + generated) one slot's KV cache holds, and the engine once built
        self.slot_capacity = int(cfg.get("slot_capacity", 512))
        self._slot_decoder = None
        self.fixed_stage = cfg.get("fixed_stage", None)        # None => random.choice like the reference
        self.fixed_taskstage = cfg.get("fixed_taskstage", None)
        self.bos_id, self.pad_id = cfg.get("bos_token_id", 1), cfg.get("pad_token_id", 2)
        self.llama_tokenizer = cfg.get("tokenizer", None)
        self.prompt_list = cfg.get("prompt_list", [])
        need_bwd = cfg.get("need_backward", True)
        # freeze_qformer: False (myriad.py:159-165): Qformer.* and query_tokens are trainable, and -- the module is no longer put
        # in eval() -- BERT's dropout is live in training forwards: hidden_dropout_prob = attention_probs_dropout_prob = 0.1
        # (cfg qformer_dropout).  Like lora_dropout_seed: the counter-based masks draw from torch's seed (train.py:63-72 seeds it
        # with seed + rank, so ranks drop different elements) unless cfg qformer_dropout_seed is given.
        self.train_qformer = cfg.get("freeze_qformer", True) is False
        self.qformer_dropout = float(cfg.get("qformer_dropout", 0.1)) if self.train_qformer else 0.0
        if not 0.0 <= self.qformer_dropout < 1.0:
            raise ValueError(f"qformer_dropout {self.qformer_dropout}: must be in [0, 1)")
        self.qformer_seed = int(cfg.get("qformer_dropout_seed", torch.initial_seed())) & ((1 << 31) - 1)
        self._qf_step = 0                                      # training forwards so far: one mask set per forward
        # freeze_vit: False (myriad.py:134-144): visual_encoder.* and ln_vision.* are trainable -- fp32 masters in the flat
        # buffer, bf16 working copies (the reference's fp32 ViT under autocast: vit_precision "fp32"); use_grad_checkpoint keeps
        # only each block's input and recomputes the block in the backward (eva_vit.py:176-180)
        self.train_vit = cfg.get("freeze_vit", True) is False
        self.vit_checkpoint = self.train_vit and bool(cfg.get("use_grad_checkpoint", False))
        # drop_path_rate (from_config admits it behind vit_drop_path / MYRIAD_VIT_DROP_PATH): every training forward draws one
        # keep bit per (block, branch, sample) on the host (eva_vit.drop_path_keep_bits: a pure integer function of the seed, the
        # data-parallel rank, the optimiser step, the micro-step inside an accumulation window and the position) and the ViT
        # skips the dropped samples' branches.  Like qformer_dropout_seed the seed defaults to torch's (train.py seeds it with
        # seed + rank); the rank enters the draw as well, so ranks differ even under one explicit drop_path_seed.
        self.drop_path_rate = float(cfg.get("drop_path_rate", 0.0)) if self.train_vit else 0.0
        if not 0.0 <= self.drop_path_rate < 1.0:
            raise ValueError(f"drop_path_rate {self.drop_path_rate}: must be in [0, 1)")
        self.drop_path_seed = int(cfg.get("drop_path_seed", torch.initial_seed())) & ((1 << 63) - 1)
        self.drop_path_rank = 0                                # train_step(dp=...) sets it to dp.rank
        self.drop_path_step = 0                                # optimiser updates so far (a resumed run sets it to its iteration)
        self._drop_micro = 0                                   # training forwards since the last update
        ops.ensure_workspace(self._dev)                       # scratch for the automatic split-K GEMM path
        # the HIP encoder.  Frozen, it is also `visual_encoder`; with freeze_vit: False that name is the nn.Module node that
        # carries the visual_encoder.* parameters (named_parameters() yields the reference's names)
        self.vit = EvaViTHIP(weights, cfg.get("vit_heads", 16), self._dev)
        if not self.train_vit:
            self.visual_encoder = self.vit
        self.qformer = QFormerHIP(weights, cfg.get("qf_heads", 12), self._dev,
                                  need_backward=need_bwd and (self.arch == "myriad" or self.train_qformer or self.train_vit))
        self.llama = LlamaHIP(weights, cfg.get("llm_heads", 32), self._dev, eps=float(cfg.get("llm_eps", 1e-6)),
                              need_backward=need_bwd)
        # copies: _load_vision_keys writes them in place
        self.ln_w = weights["ln_vision.weight"].to(self._dev, F32, copy=True).contiguous()
        self.ln_b = weights["ln_vision.bias"].to(self._dev, F32, copy=True).contiguous()
        self.query_tokens_f32 = weights["query_tokens"].to(self._dev, F32).contiguous()      # frozen (myriad.py:165)
        self.proj_w = weights["llama_proj.weight"].to(self._dev, BF16).contiguous()
        self.proj_b = weights["llama_proj.bias"].to(self._dev, F32).contiguous()
        self.proj_wT = self.proj_w.t().contiguous()
        self.Dv, self.Dq, self.Dl = self.vit.D, self.qformer.D, self.llama.D
        self.nq0 = self.query_tokens_f32.shape[1]
        # ---- trainables
        specs = []
        if self.arch == "myriad":
            specs.append(("expert_adaptor.conv1.weight", (4, self.Dv), (4, self.Dv)))
            specs.append(("expert_adaptor.conv2.weight", (self.Dv, 4), (self.Dv, 4)))
            specs += ve_param_specs("VETokenizer.", self.Dl, 5)
            specs.append(("VETokenizer.base_prompts", (9, self.Dl), (9, self.Dl)))
            specs += ve_param_specs("VEInstructor.", self.Dq, 1)
        else:
            specs.append(("llama_proj.weight", (self.Dl, self.Dq), (self.Dl, self.Dq)))
            specs.append(("llama_proj.bias", (self.Dl,), (self.Dl,)))
        if self.train_qformer:
            specs += qformer_param_specs(weights)
        if self.train_vit:
            specs += self.vit.param_specs()
            specs += [("ln_vision.weight", (self.Dv,), (self.Dv,)), ("ln_vision.bias", (self.Dv,), (self.Dv,))]
        # PEFT LoRA on q_proj/v_proj (myriad.py:170-180): off in the shipped recipe, on with cfg use_lora
        self.use_lora = bool(cfg.get("use_lora", False))
        lora_init = {}
        if self.use_lora:
            from .lora import LoraQV, init_lora_weights, lora_param_specs
            r = int(cfg.get("lora_r", 8))
            n_l = len(self.llama.layers)
            specs = lora_param_specs(n_l, self.Dl, r) + specs      # LoRA tensors first: keeps A_q|A_v adjacent
            lora_init = init_lora_weights(n_l, self.Dl, r, seed=int(cfg.get("lora_seed", 1234)), device=self._dev)
        self.store = ParamStore(specs, self._dev)
        self._params = OrderedDict()
        for name, ishape, rshape in self.store.specs:
            if name in lora_init and name not in weights:
                src = lora_init[name]
            elif name in weights:
                src = weights[name]
            else:
                src = init_trainable(name, rshape)      # built from the frozen files only: the reference's constructors' init
            self.store.p[name].copy_(from_reference_layout(src.to(self._dev, F32), ishape))
            prm = nn.Parameter(self.store.p[name], requires_grad=True)
            prm.grad = self.store.g[name]
            self._params[name] = prm
            self._register_dotted(name, prm)
        if self.arch == "myriad":
            self.adaptor = LoraAdaptor(self.store.p, self.store.g)
            self.ve_tok = VENet("VETokenizer.", 5, self.Dl, self.store.p, self.store.g, self._dev)
            self.ve_ins = VENet("VEInstructor.", 1, self.Dq, self.store.p, self.store.g, self._dev)
        if self.use_lora:
            self.lora = LoraQV(len(self.llama.layers), self.Dl, int(cfg.get("lora_r", 8)),
                               float(cfg.get("lora_alpha", 16)), float(cfg.get("lora_dropout", 0.05)),
                               self.store.p, self.store.g, self._dev)
            # peft's nn.Dropout draws from torch's RNG, which train.py:63-72 seeds with seed + rank: the counter-based masks
            # take that seed, so ranks (and runs with another seed) drop different elements (cfg lora_dropout_seed overrides)
            self.lora.base_seed = int(cfg.get("lora_dropout_seed", torch.initial_seed())) & ((1 << 31) - 1)
            self.llama.attach_lora(self.lora)
        if self.train_qformer:
            self.query_tokens_f32 = self.store.p["query_tokens"]       # fp32 master, read in place
            self.qformer.bind_trainable(self.store, need_denc=self.arch == "myriad" or self.train_vit)
        if self.train_vit:
            self.ln_w, self.ln_b = self.store.p["ln_vision.weight"], self.store.p["ln_vision.bias"]   # fp32 masters, in place
            self.vit.bind_trainable(self.store, need_backward=need_bwd)
        self._pending_update = None
        self._vit_stream, self._vit_prefetched = None, None
        self._vit_graphs, self._vit_seen, self._vit_rest = {}, {}, None
        # blocks in the look-ahead's first piece (of 39): measured 39 -> 50.9, 30 -> 49.6, 24 -> 49.1, 20 -> 49.1, 12 -> 50.8, 0 -> 52.3 ms
        self._vit_split = int(os.environ.get("MYRIAD_VIT_SPLIT", "22"))
        self._vit_graph_on = os.environ.get("MYRIAD_VIT_GRAPH", "1") != "0"
        self._leaf_aside = os.environ.get("MYRIAD_LEAF_STREAM", "1") != "0"
        self._anchor = torch.zeros((), device=self._dev, requires_grad=True)
        self._ctx = None
        self._has_grads, self._bwd_gscale, self._bwd_prev = False, 1.0, None
        self._accum_count = 0                                  # train_step calls since the last optimiser update (accum_grad_iters)
        self._bridge_used = set()

    # ------------------------------------------------------------------ nn.Module plumbing
    def _register_dotted(self, name: str, prm: nn.Parameter):
        mod = self
        parts = name.split(".")
        for part in parts[:-1]:
            if not hasattr(mod, part) or not isinstance(getattr(mod, part), nn.Module):
                setattr(mod, part, nn.Module())
            mod = getattr(mod, part)
        mod.register_parameter(parts[-1], prm)

    @property
    def device(self):
        return self._dev

    def to(self, *args, **kwargs):   # the model is built in place on its device
        dev = args[0] if args else kwargs.get("device", self._dev)
        if isinstance(dev, (str, torch.device)):
            d = torch.device(dev)
            if d.type != self._dev.type or (d.index is not None and d.index != self._dev.index):
                raise RuntimeError(f"{type(self).__name__} lives on {self._dev}; build it there (cfg.device; no CPU path exists)")
        return self

    def before_evaluation(self, **kwargs):   # base_model.py:102-103
        pass

    def state_dict(self, *a, **k):
        """Trainable parameters under the reference's key names and tensor layouts (runner_base.py:598-605 keeps
        exactly the requires_grad parameters)."""
        self.finish_update()
        out = OrderedDict()
        for name, _, rshape in self.store.specs:
            out[name] = to_reference_layout(self.store.p[name].detach(), rshape).cpu()
        return out

    @torch.no_grad()
    def merged_lora_state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """PEFT's merge_and_unload view of the q/v LoRA: per layer the merged q_proj / v_proj weights (bf16 [D, D], on the device)
        under the reference LLaMA names llama_model.model.layers.{i}.self_attn.{q,v}_proj.weight (lora.merged_qv_names), computed
        by the merge kernel's row-major output from the current fp32 masters (ops.lora_merge: the rule of
        include/myriad_hip.h).  The model itself keeps its unmerged LoRA.  Raises without LoRA."""
        if not self.use_lora:
            raise ValueError("merged_lora_state_dict: no LoRA is attached (cfg use_lora)")
        from .lora import merged_qv_names
        self.finish_update()
        out, D = OrderedDict(), self.Dl
        for i, L in enumerate(self.llama.layers):
            m = self.lora.merge_layer(i, L, "rows")
            nq, nv = merged_qv_names(i)
            out[nq], out[nv] = m[:D].clone(), m[2 * D:].clone()
        return out

    def load_state_dict(self, sd, strict: bool = False):
        self.finish_update()                              # a delayed update must not land on top of the loaded values
        self.store.version += 1
        missing = []
        for name, ishape, _ in self.store.specs:
            if name in sd:
                self.store.p[name].copy_(from_reference_layout(sd[name].to(self._dev, F32), ishape))
            else:
                missing.append(name)
        if self.train_vit:
            self.vit.refresh()                 # the masters took the visual_encoder.* / ln_vision.* keys above
        else:
            self._load_vision_keys(sd)
        if strict and missing:
            raise KeyError(missing)
        return missing

    @torch.no_grad()
    def _load_vision_keys(self, sd) -> None:
        """visual_encoder.* / ln_vision.* entries go into the ViT and ln_vision even while they are frozen: the reference's
        load_state_dict(strict=False) of a checkpoint from a run that trained them.  Written in place (captured ViT graphs
        keep their storage); a look-ahead forward made with the old weights is dropped.  Nothing happens without such keys."""
        if not any(k.startswith(("visual_encoder.", "ln_vision.")) for k in sd.keys()):
            return
        main = torch.cuda.current_stream()
        self._vit_rest, self._vit_prefetched = None, None  # a pending or finished look-ahead of the old weights: dropped
        if self._vit_stream is not None:
            main.wait_stream(self._vit_stream)            # nothing on the side stream still reads the weights being replaced
        self.vit.load_weights(sd)
        for key, dst in (("ln_vision.weight", self.ln_w), ("ln_vision.bias", self.ln_b)):
            if key in sd:
                dst.copy_(sd[key].to(self._dev, F32).reshape(dst.shape))

    @classmethod
    def from_config(cls, cfg):
        """`Myriad.from_config` / `MiniGPT4.from_config` (myriad.py:456-517, mini_gpt4.py:259-307) with the reference's own
        keys: vit_model, q_former_model, image_size, num_query_token, llama_model, drop_path_rate, use_grad_checkpoint,
        vit_precision, freeze_vit, freeze_qformer, freeze_llama, use_lora, k_shot, round_index, prompt_path,
        prompt_template, max_txt_len, end_sym, low_resource, device_8bit, ckpt (drop_path_rate > 0 needs freeze_vit: False and
        the opt-in vit_drop_path: True or MYRIAD_VIT_DROP_PATH=1; drop_path_seed seeds its draw).  The frozen weights and the tokenizer are
        loaded from the files those keys name (checkpoint.load_reference_weights); `cfg["weights"]` / `cfg["tokenizer"]`
        (an in-memory mapping keyed by the reference's state_dict names, e.g. synthetic.SyntheticWeights) replace the
        files in tests and in bench.py."""
        get = cfg.get if hasattr(cfg, "get") else (lambda k, d=None: getattr(cfg, k, d))
        if get("low_resource", False):
            raise NotImplementedError("low_resource (8-bit LLaMA + ViT on the CPU, myriad.py:186-192) is not part of the MI355X path")
        if get("freeze_llama", True) is False:
            raise NotImplementedError("freeze_llama: False -- the HIP path keeps LLaMA frozen (dgrad only), as every "
                                      "shipped recipe does (train_configs/*.yaml)")
        train_vit = get("freeze_vit", True) is False
        if train_vit and get("vit_precision", "fp16") != "fp32":
            # the HIP path trains fp32 masters with bf16 working copies: the reference's fp32 ViT under autocast.  With
            # vit_precision fp16 (the default) the reference trains fp16 parameters directly (eva_vit.py:397-412,439-441),
            # which GradScaler.unscale_ refuses under amp: nothing to mirror
            raise NotImplementedError("freeze_vit: False needs vit_precision: fp32 (fp32 masters, bf16 working copies); "
                                      f"vit_precision: {get('vit_precision', 'fp16')} (fp16 masters) is not implemented")
        rate = get("drop_path_rate", 0)
        if rate:
            # stochastic depth (eva_vit.py:162,173-176,276) is opt-in: model key vit_drop_path: True or MYRIAD_VIT_DROP_PATH=1
            drop_on = bool(get("vit_drop_path", False)) or os.environ.get("MYRIAD_VIT_DROP_PATH") == "1"
            if not (drop_on and train_vit):
                raise NotImplementedError("drop_path_rate > 0 (stochastic depth in the ViT's training forward) is not implemented"
                                          if train_vit else "drop_path_rate only matters for an unfrozen ViT")
            if not 0.0 <= float(rate) < 1.0:
                raise ValueError(f"drop_path_rate {rate}: must be in [0, 1)")
        if get("use_grad_checkpoint", False) and not train_vit:
            raise NotImplementedError("use_grad_checkpoint only matters for an unfrozen ViT (freeze_vit: False)")
        keys = ("max_txt_len", "end_sym", "k_shot", "round_index", "fixed_stage", "fixed_taskstage", "tokenizer",
                "vit_heads", "qf_heads", "llm_heads", "need_backward", "bos_token_id", "pad_token_id", "use_lora",
                "lora_r", "lora_alpha", "lora_dropout", "lora_seed", "num_query_token", "llm_eps", "freeze_qformer",
                "qformer_dropout", "qformer_dropout_seed", "freeze_vit", "use_grad_checkpoint")
        sub = {k: get(k) for k in keys if get(k) is not None}
        if rate:                                          # accepted above: the constructor draws the keep bits from these
            sub["drop_path_rate"] = float(rate)
            if get("drop_path_seed") is not None:
                sub["drop_path_seed"] = int(get("drop_path_seed"))
        if get("max_txt_len") is None:
            sub["max_txt_len"] = 32                       # from_config defaults (myriad.py:483-484)
        if get("end_sym") is None:
            sub["end_sym"] = "\n"
        weights = get("weights")
        if weights is None:
            from .checkpoint import load_llama_tokenizer, load_reference_weights
            weights, meta = load_reference_weights(cfg, arch=cls.arch)
            for k, v in meta.items():
                sub.setdefault(k, v)
            if "tokenizer" not in sub:
                sub["tokenizer"] = load_llama_tokenizer(get("llama_model"))
        prompt_path, template = get("prompt_path", ""), get("prompt_template", "")
        if prompt_path:                                   # myriad.py:221-231
            with open(prompt_path, "r") as f:
                raw = f.read().splitlines()
            sub["prompt_list"] = [template.format(p_) for p_ in raw if "<ImageHere>" in p_]
        dev = get("device")
        if dev is None or dev == "cuda":
            dev = f"cuda:{torch.cuda.current_device()}" if torch.cuda.is_available() else "cuda:0"
        model = cls(weights, sub, device=dev)
        ckpt = get("ckpt", "")
        if ckpt:
            print("Load BLIP2-LLM Checkpoint: {}".format(ckpt))
            model.load_state_dict(torch.load(ckpt, map_location="cpu")["model"], strict=False)
        return model

    # ------------------------------------------------------------------ hot path
    def _tokenize(self, samples, B, stage, training):
        """prompt_wrap tokenisation (myriad.py:358-366) + targets (:395-405); integer ids may be supplied directly."""
        if "before_ids" in samples:
            before, after = samples["before_ids"], samples["after_ids"]
            tgt, tmask = samples.get("target_ids"), samples.get("target_mask")
            return before, after, tgt, tmask
        tok = self.llama_tokenizer
        if tok is None:
            raise RuntimeError("no tokenizer: pass integer ids (before_ids/after_ids/target_ids/target_mask) in samples")
        key = {0: "question", 1: "question2", 2: "question3"}[stage] if self.arch == "myriad" else "question"
        qs = samples[key]
        if training and "aug_image" in samples:
            qs = list(qs) + list(qs)
        prompts = ["###Human: " + q + " ###Assistant: " for q in qs]
        bs, as_ = [], []
        for p in prompts:
            pb, pa = p.split("<ImageHere>")
            bs.append(tok(pb, return_tensors="pt", add_special_tokens=False).input_ids[0])
            as_.append(tok(pa, return_tensors="pt", add_special_tokens=False).input_ids[0])
        before, after = torch.stack(bs), torch.stack(as_)     # torch.stack => equal lengths, like myriad.py:371
        tgt = tmask = None
        if training:
            texts = list(samples["text_input"]) + list(samples.get("aug_text_input", []))
            tok.padding_side = "right"
            enc = tok([t + self.end_sym for t in texts], return_tensors="pt", padding="longest", truncation=True,
                      max_length=self.max_txt_len, add_special_tokens=False)
            tgt, tmask = enc.input_ids, enc.attention_mask
        return before, after, tgt, tmask

    def _draw_drop_path(self, B: int):
        """This training forward's stochastic-depth keep bits (host bool [depth, 2, B]) and the blocks' keep probabilities: one
        draw per (drop_path_seed, rank, optimiser step, micro-step) -- see eva_vit.drop_path_keep_bits."""
        from .eva_vit import drop_path_keep_bits, drop_path_keep_prob
        depth = len(self.vit.blocks)
        keep = drop_path_keep_bits(self.drop_path_seed, self.drop_path_rank, self.drop_path_step, self._drop_micro, depth, B,
                                   self.drop_path_rate)
        self._drop_micro += 1
        return keep, drop_path_keep_prob(self.drop_path_rate, depth)

    def encode_img(self, image, maps, stage, save=True, vit_out=None):
        """`Myriad.encode_img` (myriad.py:241-272).  Returns img tokens [B, n_img, Dl] f32."""
        B = image.shape[0]
        if vit_out is not None:
            x = vit_out
        elif self.train_vit:
            # the working copies follow the fp32 masters, whoever changed them (fused AdamW, a torch optimiser through the .grad
            # views, load_state_dict): rewritten in place before every use
            self.vit.refresh()
            if save and self.drop_path_rate > 0.0:
                keep, keep_prob = self._draw_drop_path(B)
                x = self.vit.forward_train(image, checkpoint=self.vit_checkpoint, keep=keep, keep_prob=keep_prob)
            else:
                x = (self.vit.forward_train(image, checkpoint=self.vit_checkpoint) if save
                     else self.vit.forward(image))
        else:
            x = self.vit.forward(image)                                    # [B,257,Dv] f32, frozen
        N = x.shape[1]
        x2 = x.view(B * N, self.Dv)
        y = self.adaptor.forward(x2, save) if self.arch == "myriad" else x2
        enc_b, _ = ops.layernorm_fwd(y, self.ln_w, self.ln_b, 1e-5)   # ln_vision (blip2.py:119-125)
        use_ins = self.arch == "myriad" and stage in (1, 2)
        use_tok = self.arch == "myriad" and stage in (0, 1)
        nq = self.nq0 + (49 if use_ins else 0)
        # The map tokenizer's conv stack (networks.py:159-197) reads only the anomaly map and its tokens are first needed by the
        # prompt assembly, behind the whole Q-Former forward: it runs on the leaf side stream (its own split-K scratch; the stream
        # its backward runs on) beside that chain instead of ~0.3 ms behind it.  Joined before the tokens are used.
        tok_out, tok_ev = None, None
        if use_tok and self._leaf_aside and self._dev.type == "cuda":
            aux, main = self._side_stream("leaf"), torch.cuda.current_stream()
            aux.wait_stream(main)                                     # parameters (AdamW) and the map are ordered on the main stream
            maps.record_stream(aux)
            with torch.cuda.stream(aux):
                tok_out = self.ve_tok.forward(maps, save)
                tok_ev = torch.cuda.Event()
                tok_ev.record()
        q = torch.empty((B, nq, self.Dq), dtype=F32, device=self._dev)
        ops.copy3d(self.query_tokens_f32.expand(B, -1, -1), q[:, :self.nq0])
        if use_ins:
            ops.copy3d(self.ve_ins.forward(maps, save), q[:, self.nq0:])
        if self.train_qformer:
            # the bf16 working copies follow the fp32 masters, whoever updated them (fused AdamW, a torch optimiser through the
            # .grad views, load_state_dict): rewritten in place before every use
            self.qformer.refresh()
        drop = self.qformer_dropout if (save and self.training and self.train_qformer) else 0.0
        if drop > 0:
            self._qf_step += 1
        qo = self.qformer.forward(q, enc_b.view(B, N, self.Dv), save and (self.arch == "myriad" or self.train_qformer or self.train_vit),
                                  dropout=drop, seed=(self.qformer_seed << 32) + self._qf_step)
        qo_b = ops.to_bf16(qo.view(B * nq, self.Dq))
        if self.arch == "myriad":
            pw, pb = self.proj_w, self.proj_b                         # frozen (myriad.py:218-219)
        else:
            pw, pb = ops.to_bf16(self.store.p["llama_proj.weight"]), self.store.p["llama_proj.bias"]
        img = ops.gemm(qo_b, pw, bias=pb, out_dtype=F32)
        parts = [img.view(B, nq, self.Dl)]
        if use_tok:
            parts.append(self.store.p["VETokenizer.base_prompts"].view(1, 9, self.Dl).expand(B, -1, -1))
            if tok_ev is not None:
                torch.cuda.current_stream().wait_event(tok_ev)
                tok_out.record_stream(torch.cuda.current_stream())    # allocated on the side stream, read here
                parts.append(tok_out)
            else:
                parts.append(self.ve_tok.forward(maps, save))
        if save:
            self._ctx = dict(B=B, N=N, y=y, nq=nq, use_ins=use_ins, use_tok=use_tok, qo_b=qo_b)
        return parts

    def _assemble(self, parts, before, after, tgt, tmask):
        """inputs_embeds = cat(bos, before, img, after, text) (myriad.py:370-371,413-419) + mask/labels (:395-421)."""
        B = parts[0].shape[0]
        nb, na = before.shape[1], after.shape[1]
        n_img = sum(p.shape[1] for p in parts)
        T = 0 if tgt is None else tgt.shape[1]
        S = 1 + nb + n_img + na + T
        emb = torch.empty((B, S, self.Dl), dtype=F32, device=self._dev)
        col = 1 + nb
        img_slices = []
        for p in parts:
            ops.copy3d(p, emb[:, col:col + p.shape[1]])
            img_slices.append((col, p.shape[1]))
            col += p.shape[1]
        ids, rows = [], []
        for b in range(B):
            base = b * S
            ids.append(torch.tensor([self.bos_id]))
            rows.append(torch.tensor([base]))
            ids.append(before[b]); rows.append(base + 1 + torch.arange(nb))
            ids.append(after[b]); rows.append(base + 1 + nb + n_img + torch.arange(na))
            if T:
                ids.append(tgt[b]); rows.append(base + 1 + nb + n_img + na + torch.arange(T))
        ids = ops.h2d(torch.cat(ids).long(), self._dev)
        rows = ops.h2d(torch.cat(rows).int(), self._dev)
        self.llama.embed_tokens_into(ids, emb.view(B * S, self.Dl), rows)
        attn = labels = None
        if T:
            attn = torch.cat([torch.ones(B, 1 + nb + n_img + na, dtype=torch.long), tmask.long().cpu()], 1)
            targets = tgt.cpu().masked_fill(tgt.cpu() == self.pad_id, -100)
            labels = torch.cat([torch.full((B, 1 + nb + n_img + na), -100, dtype=torch.long), targets], 1)
        return emb, attn, labels, img_slices

    def _image_of(self, samples):
        """[B(+B aug), 3, H, W] f32 on the device.  The uploaded tensor is remembered in the batch dict (keyed by the identity
        of its host tensors): a look-ahead batch is touched twice -- its ViT forward one step early, the rest of its step
        later -- and must cross PCIe once."""
        src, aug = samples["image"], (samples.get("aug_image") if self.training else None)
        cached = samples.get("_image_dev") if isinstance(samples, dict) else None
        if cached is not None and cached[0] is src and cached[1] is aug:
            return cached[2]
        image = src if aug is None else torch.cat([src, aug])         # myriad.py:315-316
        image = image.to(self._dev, F32, non_blocking=True)
        if isinstance(samples, dict) and not src.is_cuda:
            samples["_image_dev"] = (src, aug, image)
        return image

    def attach_vision_expert(self, expert) -> None:
        """Optional in-model producer of the anomaly maps (`self.vision_expert` of the reference, myriad.py:83-90):
        a `myriad_amd.vision_expert.VisionExpertHIP`.  With it attached, samples may carry `expert_text_feats`
        [B,2,C] (the cached per-class [normal, abnormal] text embeddings) and `ref_images` [B*k,3,224,224] instead of
        ready-made maps; both map pairs then come from one trunk pass (myriad.py:331-345).  `ref_bank`, a list of B class
        names (what a loader passes as `scene`), stands in for `ref_images` once the classes are registered with the expert's
        `add_references`; `expert_text_feats` is then optional and wins over the bank's text pairs."""
        self.vision_expert = expert

    def _maps_for(self, samples, key: str, image: torch.Tensor) -> torch.Tensor:
        if key in samples:
            return samples[key].to(self._dev, F32)
        expert = getattr(self, "vision_expert", None)
        if expert is not None and "ref_images" not in samples and "ref_bank" in samples:
            # class names instead of reference images: the classes were registered with expert.add_references()
            (zs, _), (os_, _) = expert.forward_banked(image, list(samples["ref_bank"]), samples.get("expert_text_feats"))
            samples["anomaly_maps"], samples["oneshot_anomaly_maps"] = zs, os_
            return samples[key]
        if expert is None or "expert_text_feats" not in samples or "ref_images" not in samples:
            raise KeyError(f"samples['{key}'] is required (or attach_vision_expert() + samples['expert_text_feats'] and "
                           "samples['ref_images']): the vision expert is an upstream producer (SURVEY 2.1 row 10); "
                           "samples['ref_bank'], the B class names, stands in for ref_images once the classes are registered "
                           "with add_references()")
        (zs, _), (os_, _) = expert.forward(image, samples["expert_text_feats"], samples["ref_images"])
        samples["anomaly_maps"], samples["oneshot_anomaly_maps"] = zs, os_      # both are computed once per batch
        return samples[key]

    def _forward_impl(self, samples, need_grad: bool, vit_out=None):
        if self.use_lora:
            self.lora.step_seed = (self.lora.step_seed + 1) if need_grad else self.lora.step_seed
        stage = self.fixed_stage if self.fixed_stage is not None else random.choice([0, 1, 2])   # myriad.py:378
        if self.arch != "myriad":
            stage = 0
        image = self._image_of(samples)
        maps = None
        if self.arch == "myriad":
            task = self.fixed_taskstage if self.fixed_taskstage is not None else random.choice([0, 1])  # :381
            key = "anomaly_maps" if task == 0 else "oneshot_anomaly_maps"
            maps = self._maps_for(samples, key, image)
        before, after, tgt, tmask = self._tokenize(samples, image.shape[0], stage, True)
        parts = self.encode_img(image, maps, stage, need_grad, vit_out=vit_out)
        emb, attn, labels, img_slices = self._assemble(parts, before, after, tgt, tmask)
        loss = self.llama.forward_loss(emb, attn, labels, save_for_backward=need_grad,
                                       lora_training=need_grad and self.training)   # peft's Dropout is off in eval()
        if need_grad:
            self._ctx["img_slices"] = img_slices
        return loss

    def forward(self, samples):
        """`Myriad.forward` (myriad.py:377-431).  Returns {"loss": 0-d tensor}; `loss.backward()` works."""
        need_grad = torch.is_grad_enabled() and self.training and self.store.total > 0
        self.finish_update()                              # a delayed update of train_step() lands before parameters are read
        with torch.no_grad():
            loss = self._forward_impl(samples, need_grad)
        if need_grad:
            return {"loss": _LossBridge.apply(self._anchor, self, loss)}
        return {"loss": loss}

    def _grads_live(self) -> bool:
        """True when gradients of an earlier backward are still attached (no optimizer.zero_grad() since): the reference
        loop accumulates over `accum_grad_iters` backward calls before it steps (base_task.py:256-271)."""
        return self._has_grads and any(prm.grad is not None for prm in self._params.values())

    def backward(self, gscale: float = 1.0, accumulate: bool = False, early_adamw=None, early_exchange=None):
        """Explicit backward of the last forward: fills the flat gradient buffer, multiplied by `gscale` (a GradScaler's
        loss scale; 1.0 otherwise).  Modules this step did not use keep zero gradients AND a zero use flag, so the gated
        AdamW leaves them untouched unless another rank used them (ParamStore).  With `accumulate` the result is added to
        the gradients already in the buffer.
        early_exchange = (DataParallel, segment index): the data-parallel exchange of that segment of the gradient buffer -- the
        map tokenizer's conv head, 91 % of the bytes -- is started as soon as the tokenizer's backward is queued, on the stream
        that ran it, so the collective runs under the Q-Former / adaptor backward (runner_base.py:94-98: DDP's bucketed overlap;
        here two buckets, cut where the backward's own order puts the bytes).  Every rank issues it at the same point, also a rank
        whose prompt stage skipped the tokenizer (its zeros are its contribution)."""
        c = self._ctx
        if c is None:
            raise RuntimeError("backward() without a training forward")
        # Accumulation (base_task.py:262-271): this call's gradients are added to the buffer's.  The map tokenizer's conv-head
        # weight -- 420 of the buffer's 460 MB -- accumulates IN PLACE in its weight-gradient GEMM (VENet.backward: the residual
        # operand), so only the other ~10 M gradients are set aside, zero-filled and added back (the former form
        # cloned, zero-filled and re-added the whole buffer).  A loss scale other than 1 keeps the whole-buffer form (it multiplies
        # this call's gradients only).
        head = None
        if accumulate and float(gscale) == 1.0 and self.arch == "myriad" and self.ve_tok.head_accumulates_in_place:
            o_n = self.store.offsets.get("VETokenizer.meta_net.15.weight")
            if o_n is not None and o_n[1] >= (1 << 20):
                head = (o_n[0], o_n[0] + o_n[1])
        self._acc_head = head
        fg = self.store.flat_g_comm
        if not accumulate:
            prev = None
        elif head is None:
            prev = fg.clone()
        else:
            prev = (fg[:head[0]].clone(), fg[head[1]:].clone())
        zeroed, self._g_zeroed = getattr(self, "_g_zeroed", None), None
        if zeroed is not None and not accumulate:
            torch.cuda.current_stream().wait_event(zeroed)        # train_step filled it on the leaf stream during the forward
        elif head is None:
            fg.zero_()
        else:
            fg[:head[0]].zero_()
            fg[head[1]:].zero_()
        used = {"lora"} if self.use_lora else set()
        if self.arch == "myriad":
            used.add("expert_adaptor")
            if c["use_tok"]:
                used.add("VETokenizer")
            if c["use_ins"]:
                used.add("VEInstructor")
        else:
            used.add("llama_proj")
        if self.train_qformer:
            used.add("Qformer")
        if self.train_vit:
            used.update(("visual_encoder", "ln_vision"))
        self.store.mark_used(used)
        # modules whose parameters receive a gradient in this accumulation window (the bridge path hands torch's optimiser
        # `.grad is None` for the others, exactly what autograd leaves for a module the forward never touched)
        self._bridge_used = (self._bridge_used | used) if accumulate else set(used)
        self._bwd_gscale, self._bwd_prev = float(gscale), prev
        self._early_done = set()
        demb = self.llama.backward(defer_lora_join=True)              # [B,S,Dl] f32; LoRA wgrads run on a side stream
        self._prefetch_vit_rest()                                     # the look-ahead's second piece: beside the light tail of the step
        B, nq = c["B"], c["nq"]
        (c0, n0) = c["img_slices"][0]
        dimg = torch.empty((B, nq, self.Dl), dtype=F32, device=self._dev)
        ops.copy3d(demb[:, c0:c0 + n0], dimg)
        dimg_b = ops.to_bf16(dimg.view(B * nq, self.Dl))
        if self.arch != "myriad":
            # MiniGPT-4 stage-2: llama_proj is the trainable piece (mini_gpt4.py:98-100): wgrad only
            ops.gemm_auto_f32(ops.transpose_to_bf16(dimg_b, 64), ops.transpose_to_bf16(c["qo_b"], 64),
                              self.store.g["llama_proj.weight"])
            self.store.g["llama_proj.bias"].copy_(ops.colsum(dimg.view(B * nq, self.Dl)))
            # dqo feeds the Q-Former's weight gradients (trainable Q-Former) and, through it, d(image tokens) = denc, which only
            # a trainable ViT consumes; with both frozen nothing below llama_proj needs a gradient
            if self.train_qformer or self.train_vit:
                pwT = ops.transpose_to_bf16(ops.to_bf16(self.store.p["llama_proj.weight"]), 64)
                dqo = ops.gemm(dimg_b, pwT, out_dtype=F32).view(B, nq, self.Dq)
                dq, denc = self.qformer.backward(dqo, wgrads=self.train_qformer, want_denc=self.train_vit)
                if self.train_qformer:
                    self._query_tokens_grad(dq)
                if self.train_vit:
                    dy = self._ln_vision_backward(denc, c)
                    self.vit.backward(dy.view(B, c["N"], self.Dv), grads=self.vit.grad_views)
            if self.llama.lora is not None:
                self.llama.lora.join_wgrads()
            self._finish_backward()
            return
        dqo = ops.gemm(dimg_b, self.proj_wT, out_dtype=F32).view(B, nq, self.Dq)
        if c["use_tok"]:
            (cb, _), (ct, _) = c["img_slices"][1], c["img_slices"][2]
            dbase = torch.empty((B, 9, self.Dl), dtype=F32, device=self._dev)
            ops.copy3d(demb[:, cb:cb + 9], dbase)
            self.store.g["VETokenizer.base_prompts"].view(-1).copy_(ops.colsum(dbase.view(B, 9 * self.Dl)))
            dtok = torch.empty((B, 9, self.Dl), dtype=F32, device=self._dev)
            ops.copy3d(demb[:, ct:ct + 9], dtok)
            # the tokenizer's conv stack is a leaf (its input is the anomaly map): its backward feeds only the optimiser and
            # runs on a side stream beside the Q-Former backward
            aux, main = (self._side_stream("leaf") if self._leaf_aside else torch.cuda.current_stream()), torch.cuda.current_stream()
            aux.wait_stream(main)
            leaf_keep = (dtok, self.ve_tok._saved)       # main-stream allocations the side stream reads: alive until the join
            with torch.cuda.stream(aux):
                self.ve_tok.backward(dtok, accumulate_head=self._acc_head is not None)
                if early_adamw is not None and self._leaf_aside:
                    # single-process step: the map tokenizer holds 91 % of the trainable parameters (its 105 M-weight head) and its
                    # gradient is complete here, right behind the LLaMA backward -- its AdamW (0.55 ms of HBM traffic) runs on the
                    # leaf stream beside the Q-Former backward instead of at the tail of the step.  Same kernel, same inputs.
                    self.store.adamw_module("VETokenizer", *early_adamw)
                    self._early_done = {"VETokenizer"}
                if early_exchange is not None:
                    self._start_early_exchange(early_exchange)
                leaf_ev = torch.cuda.Event()
                leaf_ev.record()
        else:
            leaf_ev, leaf_keep = None, None
            if early_exchange is not None:                # unused at this rank's prompt stage: the segment's zeros travel now
                self._start_early_exchange(early_exchange)
        dq, denc = self.qformer.backward(dqo, wgrads=self.train_qformer)
        if self.train_qformer:
            self._query_tokens_grad(dq)
        ins_ev, ins_keep = None, None
        if c["use_ins"]:
            dins = torch.empty((B, 49, self.Dq), dtype=F32, device=self._dev)
            ops.copy3d(dq[:, self.nq0:], dins)
            if self._leaf_aside and self._dev.type == "cuda" and os.environ.get("MYRIAD_INS_ASIDE", "1") != "0":
                # the instructor's conv stack is a leaf too (its input is the anomaly map): its backward runs on the leaf stream
                # beside ln_vision's and the adaptor's backward
                aux, main = self._side_stream("leaf"), torch.cuda.current_stream()
                aux.wait_stream(main)
                ins_keep = (dins, self.ve_ins._saved)     # main-stream allocations the side stream reads: alive until the join
                with torch.cuda.stream(aux):
                    self.ve_ins.backward(dins)
                    ins_ev = torch.cuda.Event()
                    ins_ev.record()
            else:
                self.ve_ins.backward(dins)
        dy = self._ln_vision_backward(denc, c)
        dx = self.adaptor.backward(dy, need_dx=self.train_vit)
        if self.train_vit:
            # the ViT's backward: on the main stream, last -- its gradients complete the buffer
            self.vit.backward(dx.view(B, c["N"], self.Dv), grads=self.vit.grad_views)
        if self.llama.lora is not None:
            self.llama.lora.join_wgrads()                 # the side-stream LoRA weight gradients land before anyone reads flat_g
        if leaf_ev is not None:
            torch.cuda.current_stream().wait_event(leaf_ev)
        if ins_ev is not None:
            torch.cuda.current_stream().wait_event(ins_ev)
        del leaf_keep, ins_keep                           # freed only now: later main-stream work is ordered behind the events
        self._finish_backward()

    def _ln_vision_backward(self, denc: torch.Tensor, c) -> torch.Tensor:
        """ln_vision's backward: d(its input) [B*N, Dv] f32; with a trainable ViT also ln_vision.weight / .bias gradients."""
        d2 = denc.view(c["B"] * c["N"], self.Dv)
        if self.train_vit:
            ops.layernorm_param_grads(d2, c["y"], 1e-5, self.store.g["ln_vision.weight"], self.store.g["ln_vision.bias"])
        return ops.layernorm_bwd(d2, c["y"], self.ln_w, 1e-5)[0]

    def _query_tokens_grad(self, dq: torch.Tensor) -> None:
        """d query_tokens = the batch sum of the Q-Former input gradient over its first nq0 (query-token) rows."""
        B, nq, D = dq.shape
        self.store.g["query_tokens"].view(-1).copy_(ops.colsum(dq.reshape(B, nq * D)[:, :self.nq0 * D]))

    def _start_early_exchange(self, early_exchange) -> None:
        """early_exchange = (dp, segment index[, (lr, weight_decay, beta2)]): start the segment's collective behind the current stream;
        with the third item the segment's optimiser update follows its collective on the exchange's own stream order -- the gated
        AdamW on this rank's slices of the segment (its 1/world piece in 'rs_ag') with grad_scale 1/world, then in 'rs_ag' the
        all-gather of the updated parameters -- so both run under the Q-Former backward as well (finish_update() does the rest of
        the buffer and bumps the step counters)."""
        dp, k = early_exchange[0], early_exchange[1]
        st = self.store
        if len(early_exchange) > 2 and getattr(dp, "supports_early_update", False):
            lr, wd, beta2 = early_exchange[2]

            def then():
                st.adamw_pieces(dp.part_shards(st.total, k), lr, wd, beta2=beta2, grad_scale=1.0 / dp.world)
                dp.gather_part(st.flat_p, k)
            dp.start_part(st.flat_g_comm, st.total, k, then=then)
        else:
            dp.start_part(st.flat_g_comm, st.total, k)

    def _finish_backward(self):
        if self._bwd_gscale != 1.0:
            ops.scale_(self.store.flat_g, self._bwd_gscale)
        if self._bwd_prev is not None:
            fg = self.store.flat_g_comm
            if isinstance(self._bwd_prev, tuple):                 # the head's segment accumulated in place (backward())
                a, b = self._acc_head
                for pv, dst in ((self._bwd_prev[0], fg[:a]), (self._bwd_prev[1], fg[b:])):
                    if pv.numel():
                        ops.copy2d(pv.view(1, -1), dst.view(1, -1), accumulate=True)
            else:
                n = fg.numel()
                ops.copy2d(self._bwd_prev.view(1, n), fg.view(1, n), accumulate=True)
            self._bwd_prev = None
        self._has_grads = True
        self._reattach_grads()
        self._ctx = None

    def _reattach_grads(self):
        """Autograd-bridge path (`model(samples)["loss"].backward()` + an external torch optimiser): `.grad` aliases the flat
        buffer for the parameters of modules this step (or accumulation window) used, and is None for the others -- a module
        unused at this prompt stage (VEInstructor at stage 0, VETokenizer at stage 2; myriad.py:378,252,265) then gets no
        weight decay, no moment decay and no step increment from torch.optim.AdamW, as in the reference."""
        used = getattr(self, "_bridge_used", None)
        for name, prm in self._params.items():
            if used is not None and module_of(name) not in used:
                prm.grad = None
            elif prm.grad is None or prm.grad.data_ptr() != self.store.g[name].data_ptr():
                prm.grad = self.store.g[name]

    def _side_stream(self, name: str):
        return ops.side_stream(self._dev, name)

    def prefetch_vit(self, samples) -> None:
        """Launch the frozen ViT forward of a LATER step on a side stream.  The result is picked up by the train_step() that
        receives the same `samples` object.  Its split-K GEMMs use their own scratch (mh_set_stream_workspace).

        The forward is issued in two pieces.  Its GEMMs are work the chip has to do -- run beside the LLaMA part they cost
        almost their own duration -- but the step has two phases in which the main stream leaves most CUs idle (chains of
        5-30 us launches): the adaptor / Q-Former forward at its start, and the Q-Former / adaptor backward + AdamW at its
        end.  The first `MYRIAD_VIT_SPLIT` blocks are launched here, at the start of the step; the rest by
        _prefetch_vit_rest(), which backward() calls once the LLaMA backward is enqueued.
        From the second batch of a given size on, both pieces are replayed from hipGraphs captured on that stream (fixed
        shapes, frozen weights, no host-side arguments): enqueueing ~290 launches costs the launch thread ~0.2 ms instead of
        ~2.8 ms during which the main stream had nothing to run (MYRIAD_VIT_GRAPH=0 disables).

        With a trainable ViT (freeze_vit: False) there is no look-ahead -- a forward of batch t+1 issued during step t would
        read weights step t is about to change -- and this is a no-op."""
        if self.train_vit:
            return
        if self._vit_stream is None:
            self._vit_stream = self._side_stream("vit")
        self._prefetch_vit_rest()                        # a look-ahead that was never consumed / finished: finish it first
        main = torch.cuda.current_stream()
        image = self._image_of(samples)
        key = tuple(image.shape)
        graph = self._vit_graphs.get(key)
        if graph is None and self._vit_graph_on and self._vit_seen.get(key, 0) >= 1 and image.dtype == F32:
            graph = self._capture_vit(image)
        self._vit_seen[key] = self._vit_seen.get(key, 0) + 1
        nb = len(self.vit.blocks)
        split = min(max(self._vit_split, 0), nb)
        self._vit_stream.wait_stream(main)               # inputs uploaded / buffers freed on the main stream so far
        with torch.cuda.stream(self._vit_stream), torch.no_grad():
            if graph is not None:
                graph["in"].copy_(image)
                graph["a"].replay()
                state = None
            else:
                state = self.vit.run_blocks(self.vit.embed(image), 0, split)
        self._vit_rest = (samples, graph, state, split)

    def _prefetch_vit_rest(self) -> None:
        """Second piece of a look-ahead ViT forward (see prefetch_vit): ordered behind everything the main stream has queued."""
        if self._vit_rest is None:
            return
        samples, graph, state, split = self._vit_rest
        self._vit_rest = None
        self._vit_stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._vit_stream), torch.no_grad():
            if graph is not None:
                if graph["b"] is not None:
                    graph["b"].replay()
                out = graph["out"].clone()               # the next replay overwrites it while this step's backward reads `out`
            else:
                ve = self.vit
                out = ve.finish(ve.run_blocks(state, split, len(ve.blocks)))
            ev = torch.cuda.Event()
            ev.record()
        self._vit_prefetched = (samples, out, ev)

    def prepare_vit_graph(self, samples) -> None:
        """Capture the look-ahead graphs for this batch's image shape now (one eager pass + the capture: ~0.1 s), so that no
        later train_step pays for it.  Without this call the capture happens at the second look-ahead of a shape."""
        if self.train_vit:
            return                                         # no look-ahead, no captured forward (prefetch_vit)
        image = self._image_of(samples)
        key = tuple(image.shape)
        if not self._vit_graph_on or key in self._vit_graphs or image.dtype != F32:
            return
        if self._vit_stream is None:
            self._vit_stream = self._side_stream("vit")
        self._vit_stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._vit_stream), torch.no_grad():
            self.vit.forward(image)            # first-call set-up of every kernel happens outside the capture
        self._vit_seen[key] = max(1, self._vit_seen.get(key, 0))
        self._capture_vit(image)

    def _capture_vit(self, image):
        """Capture the two pieces of visual_encoder.forward at this input shape into hipGraphs on the ViT side stream (whose
        split-K scratch the captured launches keep using on replay).  Called after one eager pass at the shape, so no kernel
        does first-call set-up inside the capture.  The pieces share one memory pool: piece b reads piece a's state."""
        torch.cuda.synchronize()
        ve = self.vit
        split = min(max(self._vit_split, 0), len(ve.blocks))
        static_in = torch.empty_like(image).contiguous()
        static_in.copy_(image)
        ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        # thread_local: a data-parallel run has RCCL's watchdog thread polling events while this thread captures
        with torch.no_grad(), torch.cuda.graph(ga, stream=self._vit_stream, capture_error_mode="thread_local"):
            state = ve.run_blocks(ve.embed(static_in), 0, split)
        if split < len(ve.blocks):
            with torch.no_grad(), torch.cuda.graph(gb, pool=ga.pool(), stream=self._vit_stream, capture_error_mode="thread_local"):
                static_out = ve.finish(ve.run_blocks(state, split, len(ve.blocks)))
        else:
            gb, static_out = None, ve.finish(state)          # a shallow encoder: everything is in the first piece
        g = dict(a=ga, b=gb, out=static_out, state=state)
        g["in"] = static_in
        self._vit_graphs[tuple(image.shape)] = g
        return g

    def _take_prefetched_vit(self, samples):
        if self._vit_rest is not None and self._vit_rest[0] is samples:
            self._prefetch_vit_rest()                    # its second piece was never issued (no backward in between)
        if self._vit_prefetched is None or self._vit_prefetched[0] is not samples:
            return None
        _, out, ev = self._vit_prefetched
        self._vit_prefetched = None
        main = torch.cuda.current_stream()
        main.wait_event(ev)
        out.record_stream(main)                          # allocated on the side stream, consumed (and freed) on this one
        return out

    def train_step(self, samples, lr: float, weight_decay: float = 0.05, allreduce=None, world: int = 1, dp=None,
                   overlap: bool = True, next_samples=None, accum_grad_iters: int = 1, accum_index=None, beta2: float = 0.999,
                   max_grad_norm=None, skip_nonfinite: bool = False):
        """forward + backward (+ gradient all-reduce) + fused AdamW: one optimisation step of
        `BaseTask._train_inner_loop` (base_task.py:233-271) without the autograd bridge.
        With a `DataParallel` (`dp`) and overlap=True the all-reduce + AdamW of step t are hidden behind the frozen
        ViT forward of step t+1 (95 % of the gradient bytes only exist after the whole LLaMA backward, so
        overlapping with backward hides nothing); call `finish_update()` after the last step.

        accum_grad_iters > 1 (base_task.py:262-271, runner_base.py:311-312): the gradients -- and the per-module use flags -- of
        that many consecutive calls are summed in the flat buffer (no division, as the reference); the exchange and the AdamW
        run on the last call of a window, with that call's lr.  A module is skipped by the gated AdamW only if no call of the
        window (on any rank) used it, which is what `optimizer.zero_grad()` (set_to_none) + DDP leave torch's AdamW.  The
        reference all-reduces every backward; one exchange of the window's sum is the same gradient.
        `accum_index` = the iteration index inside the epoch (RunnerBase passes it): the update then lands where the reference
        puts it, `(i + 1) % accum_grad_iters == 0` with i restarting every epoch (base_task.py:265), so when iters_per_epoch is
        not a multiple of accum_grad_iters the left-over gradients of an epoch's tail are folded into the next epoch's first
        update, as the reference's un-zeroed .grad does.  Without it the window is counted in calls.
        `beta2`: AdamW's second-moment decay (run.beta2, runner_base.py:130-135); beta1 is 0.9 as in the reference.
        `max_grad_norm` (None or <= 0: off): torch.nn.utils.clip_grad_norm_ on the whole trainable gradient of the update -- the
        rank average, and an accumulation window's sum, which is where the reference's loop would clip.  `skip_nonfinite`: an
        update whose gradient holds an inf or a NaN is not applied at all (what GradScaler.step did under fp16 AMP): parameters,
        moments and step counts keep their bits.  Both are decided on the device (ParamStore.adamw_step(clip=...)); grad_stats()
        reads the verdict back for logging.  While either is on nothing is updated before the norm of the WHOLE gradient is
        known: the early tokenizer update and the update behind the early exchange fall back to their late forms (the early
        collective itself stays).  With both off the step issues exactly the launches it issued without them."""
        clip = GradClip.of(max_grad_norm, skip_nonfinite)
        if dp is not None:
            self.drop_path_rank = int(getattr(dp, "rank", 0))     # ranks draw different stochastic-depth bits
        with torch.no_grad():
            vit_out = self._take_prefetched_vit(samples)
            if next_samples is not None:
                self.prefetch_vit(next_samples)         # runs beside everything below
            if self._pending_update is not None and vit_out is not None:
                self.finish_update()
            elif self._pending_update is not None and self.train_vit:
                self.finish_update()                    # this step's ViT forward reads the weights that update writes
            elif self._pending_update is not None:
                # The previous step's gradient all-reduce is still in flight on the side stream: run this step's
                # frozen ViT forward (independent of the update) under it, then apply the delayed AdamW.
                vit_out = self.vit.forward(self._image_of(samples))
                self.finish_update()
            if (self._accum_count == 0 and self._leaf_aside and self._dev.type == "cuda"
                    and os.environ.get("MYRIAD_EARLY_ZERO", "1") != "0"):
                # the gradient buffer's zero fill (460 MB, ~55 us) leaves the chain between forward and backward: nothing writes a
                # gradient before the backward, and the last update (main stream, and the leaf stream itself) has read them
                aux, main = self._side_stream("leaf"), torch.cuda.current_stream()
                aux.wait_stream(main)
                with torch.cuda.stream(aux):
                    self.store.flat_g_comm.zero_()
                    self._g_zeroed = torch.cuda.Event()
                    self._g_zeroed.record(aux)
            try:
                loss = self._forward_impl(samples, True, vit_out=vit_out)
            except Exception:
                self._g_zeroed = None                 # a forward that raised ("no valid labels"): no stale event for a later backward()
                raise
            accumulate = self._accum_count > 0                   # > 0: the flat buffer holds gradients no update has consumed
            due = accum_update_due(self._accum_count + 1, accum_grad_iters, accum_index)
            # no gradient exchange, no accumulation window: modules whose gradient is complete early are updated early (backward())
            # (world == 1 as well: a caller-scaled update -- `world` > 1 without dp / allreduce -- must see ONE grad_scale)
            early = (lr, weight_decay, beta2) if (due and not accumulate and (dp is None or dp.world == 1) and allreduce is None
                                                  and world == 1 and clip is None
                                                  and os.environ.get("MYRIAD_EARLY_ADAMW", "1") != "0") else None
            if dp is not None and dp.world > 1 and self.arch == "myriad" and hasattr(dp, "set_segments"):
                # the exchange's segmentation -- in 'rs_ag' the slices of the Adam moments each rank owns -- is fixed before the
                # first exchange, whether or not this step overlaps it: every step then shards the optimiser state the same way
                self._dp_segment(dp)
            # data parallel with the exchange overlapped: the tokenizer's segment of the gradient buffer starts its collective from
            # inside the backward (backward(): early_exchange); accumulation windows exchange the window's sum at its end instead
            early_x = None
            if (dp is not None and dp.world > 1 and overlap and due and not accumulate and self.arch == "myriad"
                    and hasattr(dp, "start_part") and os.environ.get("MYRIAD_DP_EARLY", "1") != "0"):
                k = self._dp_segment(dp)
                if k is not None:
                    early_upd = clip is None and os.environ.get("MYRIAD_DP_EARLY_ADAMW", "1") != "0"
                    early_x = (dp, k, (lr, weight_decay, beta2)) if early_upd else (dp, k)
            self.backward(accumulate=accumulate, early_adamw=early, early_exchange=early_x)
            self._accum_count += 1
            if not due:
                return loss                                   # inside an accumulation window: no exchange, no update
            self._accum_count = 0
            self.drop_path_step, self._drop_micro = self.drop_path_step + 1, 0
            if dp is not None and dp.world > 1 and overlap:
                dp.start(self.store.flat_g_comm, self.store.total)   # RCCL exchange on the side HIP stream (grads + use flags)
                self._pending_update = (dp, lr, weight_decay, beta2, clip)
            else:
                shard = None
                if dp is not None and dp.world > 1:
                    dp.allreduce(self.store.flat_g_comm, self.store.total)
                    shard = self._dp_shards(dp)
                elif allreduce is not None:
                    allreduce(self.store.flat_g_comm)
                    world = max(world, 1)
                self.store.adamw_step(lr, weight_decay, beta2=beta2, grad_scale=1.0 / (dp.world if dp is not None else world),
                                      shard=shard, skip=self._early_done, clip=clip.for_dp(dp) if clip is not None else None)
                if shard is not None:
                    dp.gather_params(self.store.flat_p)
        return loss

    def _dp_shards(self, dp):
        """rs_ag: the slices of the flat buffers this rank's AdamW owns (one per exchange segment); None: the whole buffer."""
        if getattr(dp, "mode", "allreduce") != "rs_ag":
            return None
        return dp.shards(self.store.total) if hasattr(dp, "shards") else [dp.shard(self.store.total)[:2]]

    def _dp_segment(self, dp):
        """Cut the exchange at the map tokenizer's conv-head weights (its weight-decay run of the flat buffer: 105 M of the 115 M
        trainables) and return that segment's index, or None when the model has no such run worth an exchange of its own.  The
        cut points are rounded inwards to multiples of 32 elements, so that at 2 / 4 / 8 ranks every segment's reduce-scatter
        tiles it exactly (ParamStore pads the total the same way)."""
        if getattr(self, "_dp_seg_of", None) is not None and self._dp_seg_of[0] is dp:
            return self._dp_seg_of[1]
        k = None
        rng = self.store.module_range("VETokenizer", True)
        if rng is not None:
            a, b = ops.round_up(rng[0], 32), rng[1] // 32 * 32
            if b - a >= (1 << 20):
                dp.set_segments(self.store.total, [a, b])
                segs = dp.segments(self.store.total)
                k = segs.index((a, b)) if (a, b) in segs else None
        self._dp_seg_of = (dp, k)
        return k

    def finish_update(self):
        """Apply a delayed optimiser update (overlap mode): wait for the gradient exchange, if any, then fused AdamW."""
        if self._pending_update is not None:
            dp, lr, wd, beta2, clip = self._pending_update
            self._pending_update = None
            if dp is None:
                self.store.adamw_step(lr, wd, beta2=beta2, clip=clip)
                return
            dp.wait()
            shard = self._dp_shards(dp)
            done = dp.take_early_done() if hasattr(dp, "take_early_done") else set()      # segments updated behind their collective
            segs = dp.segments(self.store.total) if done else []
            self.store.adamw_step(lr, wd, beta2=beta2, grad_scale=1.0 / dp.world, shard=shard, exclude=[segs[k] for k in done],
                                  clip=clip.for_dp(dp) if clip is not None else None)
            if shard is not None:
                dp.gather_params(self.store.flat_p, skip=done) if done else dp.gather_params(self.store.flat_p)

    def grad_stats(self) -> dict:
        """{"grad_norm", "clip_scale", "applied", "skipped_steps"} of the last update run with max_grad_norm / skip_nonfinite:
        the total norm of the averaged gradient before clipping, the one multiplier the AdamW applied to the raw gradient
        (grad_scale included), whether the update was applied, and how many were not so far.  One small device -> host copy,
        for logging; the training path never calls it."""
        return self.store.grad_stats()

    def _generate_args(self, generate_kwargs) -> dict:
        """generate()'s keyword arguments, checked and with their defaults (its docstring states the contract)."""
        kw = dict(generate_kwargs)
        stops = kw.pop("stop_ids", None)
        crit = kw.pop("stopping_criteria", None)
        if crit is not None:
            stops = [tuple(int(t) for t in torch.as_tensor(st).reshape(-1).tolist()) for c in crit for st in getattr(c, "stops", [])]
        if stops is None:
            stops = ()                                     # HF without a criterion stops on EOS / max_new_tokens only
        max_new = kw.pop("max_new_tokens", None)
        if max_new is None:
            max_len = kw.pop("max_length", None)
            max_new = 20 if max_len is None else None
        do_sample = bool(kw.pop("do_sample", False))
        top_p = float(kw.pop("top_p", 1.0))
        temperature = float(kw.pop("temperature", 1.0))
        min_length = int(kw.pop("min_length", 0))
        eos_id = kw.pop("eos_token_id", self.pad_id)
        kw.pop("pad_token_id", None)
        if not kw.pop("use_cache", True):
            raise NotImplementedError("use_cache=False: decode here always keeps a KV cache (same tokens)")
        top_k = kw.pop("top_k", 50)                         # HF's generation default; only a sampled (host-drawn) row sees it
        top_k = 0 if top_k is None else int(top_k)
        if do_sample and not temperature > 0:
            raise ValueError(f"generate(temperature={temperature}): must be > 0 when do_sample=True")
        rep_pen = kw.pop("repetition_penalty", 1.0)
        rep_pen = 1.0 if rep_pen is None else float(rep_pen)
        if not rep_pen > 0:
            raise ValueError(f"generate(repetition_penalty={rep_pen}): must be > 0")
        beams = kw.get("num_beams")
        # the beam path's own switch (a model without the attribute has it off)
        beam_sampling = bool(getattr(self.llama, "beam_sampling", False) and isinstance(beams, numbers.Real) and beams > 1)
        if rep_pen != 1.0 and not self.llama.device_sampling and not beam_sampling:
            # opt-in like the device sampler itself: with the switch off generate() keeps its earlier contract and refuses it
            raise NotImplementedError(f"generate(repetition_penalty={rep_pen}) needs the device sampling switch "
                                      "(MYRIAD_DEVICE_SAMPLING=1 or model.llama.device_sampling = True)")
        num_beams = kw.pop("num_beams", 1)
        num_beams = 1 if num_beams is None else num_beams
        integral = isinstance(num_beams, numbers.Integral) or (isinstance(num_beams, numbers.Real) and float(num_beams).is_integer())
        if not integral or num_beams < 1:                  # HF refuses these too (ValueError)
            raise ValueError(f"generate(num_beams={num_beams!r}): must be a positive integer")
        num_beams = int(num_beams)
        beam_kw = {}
        if num_beams > 1:
            if do_sample and not beam_sampling:
                raise NotImplementedError(f"generate(num_beams={num_beams}, do_sample=True): beam sampling needs its switch "
                                          "(MYRIAD_BEAM_SAMPLING=1 or model.llama.beam_sampling = True)")
            if rep_pen != 1.0 and not beam_sampling:
                raise NotImplementedError(f"generate(num_beams={num_beams}, repetition_penalty={rep_pen}) needs the beam sampling "
                                          "switch (MYRIAD_BEAM_SAMPLING=1 or model.llama.beam_sampling = True)")
            if num_beams > ops.BEAM_MAX:
                raise NotImplementedError(f"generate(num_beams={num_beams}): at most {ops.BEAM_MAX} beams on the HIP decode path")
            if do_sample and not 1 <= top_k <= ops.SAMPLE_CAP:
                raise NotImplementedError(f"generate(num_beams={num_beams}, do_sample=True, top_k={top_k}): beam sampling draws on "
                                          f"the device only, top_k in 1..{ops.SAMPLE_CAP}")
            lp = kw.pop("length_penalty", 1.0)
            nrs = kw.pop("num_return_sequences", 1)
            es = kw.pop("early_stopping", False)
            beam_kw = dict(length_penalty=1.0 if lp is None else float(lp), num_return_sequences=1 if nrs is None else int(nrs),
                           early_stopping=False if es is None else es)
            if not 1 <= beam_kw["num_return_sequences"] <= num_beams:
                raise ValueError(f"generate(num_return_sequences={nrs}) has to be between 1 and num_beams={num_beams}")
            if beam_kw["early_stopping"] not in (True, False, "never"):
                raise ValueError(f"generate(early_stopping={es!r}): True, False or 'never'")
            if beam_sampling:                              # switch off: beam_generate is called with today's arguments
                beam_kw.update(do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=rep_pen)
        for k, neutral in (("num_beams", 1), ("length_penalty", 1), ("num_return_sequences", 1)):
            v = kw.pop(k, neutral)
            if v not in (neutral, None):
                raise NotImplementedError(f"generate({k}={v}) is not implemented on the HIP decode path")
        generator = kw.pop("generator", None)
        output_scores = bool(kw.pop("output_scores", False))
        watch_ids = kw.pop("watch_ids", None)
        watch_ids = () if watch_ids is None else tuple(watch_ids)
        if watch_ids and not output_scores:
            raise ValueError("generate(watch_ids=...) names the ids whose log-probs output_scores=True returns: pass both")
        watch_ids = tuple(ops.score_watch_ids(watch_ids, self.llama.V))     # at most 8 integers in [0, V): ValueError otherwise
        if output_scores and num_beams > 1:
            raise NotImplementedError(f"generate(num_beams={num_beams}, output_scores=True): beam search reports "
                                      "sequences_scores (last_generate_stats); per-token scores are not implemented with beams")
        draft, draft_k = kw.pop("draft", None), kw.pop("draft_k", 4)
        if draft is not None and num_beams > 1:
            raise NotImplementedError(f"generate(draft=..., num_beams={num_beams}): draft decoding is greedy decoding of one sequence")
        if kw:
            raise TypeError(f"generate() got unsupported arguments: {sorted(kw)}")
        return dict(draft=draft, draft_k=draft_k, stops=stops, max_new=max_new, max_len=None if max_new is not None else max_len, do_sample=do_sample,
                    top_p=top_p, temperature=temperature, min_length=min_length, eos_id=eos_id, top_k=top_k, rep_pen=rep_pen,
                    num_beams=num_beams, beam_kw=beam_kw, generator=generator, output_scores=output_scores, watch_ids=watch_ids)

    @torch.no_grad()
    def generate(self, samples, **generate_kwargs):
        """`Myriad.generate` (myriad.py:433-454): stage-1 prompt layout, then the HF `generate(inputs_embeds=..., **kw)`
        contract for the arguments the evaluation script passes (evaluation_aqa_dataset.py:289-301):
        max_new_tokens, stopping_criteria (a list whose items carry `.stops` = id tensors, conversation.py:96-107, applied
        to batch row 0), do_sample + top_p + temperature (see LlamaHIP.greedy_generate: arg-max whenever p_max >= top_p,
        a host-side draw otherwise), min_length, use_cache.  Anything that would change the decoding rule and is not
        implemented raises instead of being ignored.

        Also the chat call's sampling knobs (conversation.py:144-168): top_k (HF default 50; 0 / None = no top-k),
        temperature (> 0 when sampling) and `generator`.  With `self.llama.device_sampling` (MYRIAD_DEVICE_SAMPLING=1, off by
        default) and 1 <= top_k <= 1024 every draw happens on the device inside the captured token step, reproducible per seed
        (drawn once per call from `generator`) but not bit-comparable with torch.multinomial; otherwise rows with p_max < top_p
        are drawn on the host.  The same switch enables repetition_penalty (> 0; HF's rule over the generated ids, applied on
        the device before every pick, greedy or sampled); with it off a penalty other than 1 raises as before.

        num_beams > 1 (with do_sample=False) runs HF's beam search (LlamaHIP.beam_generate) and then also takes length_penalty,
        early_stopping (True / False / "never") and num_return_sequences (<= num_beams, else ValueError): token_ids is
        [B * num_return_sequences, L], item-major, best first, and last_generate_stats gains num_beams, sequences_scores,
        finished_hypotheses and graph_replays.  Beam search applies the stop sequences per hypothesis, greedy / sampled decoding
        keeps the reference's row-0 rule.  Refused with beams: do_sample (beam sampling), repetition_penalty != 1 and
        num_beams > 8.  With `self.llama.beam_sampling` (MYRIAD_BEAM_SAMPLING=1, off by default) num_beams > 1 also takes
        do_sample, temperature, top_k (1 .. 1024 when sampling), top_p, repetition_penalty and generator: HF's beam-search
        multinomial sampling with its processor chain on the log-probs, drawn on the device and reproducible per seed
        (LlamaHIP.beam_generate); last_generate_stats gains beam_sampled_steps and beam_host_steps.  Without beams, length_penalty / num_return_sequences other than 1 raise NotImplementedError and
        early_stopping is an unknown argument, as before.

        output_scores=True (opt-in, with watch_ids = up to 8 token ids) adds "token_logprobs" [B, L] f32, the log-probability of
        every returned id, and "watch_logprobs" [B, L, W], that of each watched id at the same step: the log-softmax at
        temperature 1 of the logits the pick was made from (after the repetition penalty when on; temperature, top-k, top-p and
        the EOS ban do not enter), computed inside the captured token step (LlamaHIP.greedy_generate).  Positions padded after
        a row finished are 0.0.  watch_logprobs[:, 0] of the "Yes" / "No" ids is the model's own anomaly score
        (eval_aqa.py --llm-score).  With num_beams > 1 it raises NotImplementedError; more than 8 ids, a non-integer or an id
        outside the vocabulary is a ValueError.

        draft=<drafter> (opt-in; decode_host.NgramDrafter or any object with propose / observe) with draft_k = K in 1 .. 8 rows:
        draft-and-verify greedy decoding of ONE sample (LlamaHIP.greedy_generate): the same token_ids as without it, in fewer
        passes over the decoder weights when the drafter guesses well; last_generate_stats gains verify_steps, plain_steps,
        draft_proposed and draft_accepted.  NotImplementedError with a batch of more than one sample and beams, and -- unless
        `self.llama.draft_sampling` (MYRIAD_DRAFT_SAMPLING=1, off by default) is on -- with device sampling, repetition_penalty != 1
        or output_scores; with it on the sampled, penalised or scored answer is that of the call without `draft`.  The caller
        teaches the drafter (drafter.observe(ids))."""
        self.finish_update()
        a = self._generate_args(generate_kwargs)
        stops, max_new, max_len, do_sample, top_p, temperature = (a[k] for k in ("stops", "max_new", "max_len", "do_sample", "top_p",
                                                                                 "temperature"))
        min_length, eos_id, top_k, rep_pen, num_beams, beam_kw, generator = (a[k] for k in ("min_length", "eos_id", "top_k", "rep_pen",
                                                                                            "num_beams", "beam_kw", "generator"))
        stage = 1 if self.arch == "myriad" else 0
        image = samples["image"].to(self._dev, F32)
        maps = None
        if self.arch == "myriad":
            key = "oneshot_anomaly_maps" if self.k_shot > 0 else "anomaly_maps"
            maps = self._maps_for(samples, key, image)
        before, after, _, _ = self._tokenize(samples, image.shape[0], stage, False)
        parts = self.encode_img(image, maps, stage, False)
        emb, _, _, _ = self._assemble(parts, before, after, None, None)
        emb = emb[:, 1:].contiguous()         # generate() wraps without BOS (myriad.py:446-449)
        if max_new is None:
            max_new = max(1, max_len - emb.shape[1])
        self.llama.decode_lora_version = self.store.version    # decode_merge_lora re-merges only when the LoRA weights moved
        if num_beams > 1:
            if "do_sample" in beam_kw:                     # the beam sampling switch is on: the draw's generator goes with it
                beam_kw = dict(beam_kw, generator=generator)
            ids = self.llama.beam_generate(emb, num_beams, max_new_tokens=max_new, stop_ids=stops, eos_id=eos_id,
                                           min_length=min_length, **beam_kw)
        else:
            ids = self.llama.greedy_generate(emb, max_new_tokens=max_new, stop_ids=stops, min_length=min_length, eos_id=eos_id,
                                             do_sample=do_sample, top_p=top_p, temperature=temperature, generator=generator,
                                             top_k=top_k, repetition_penalty=rep_pen, return_scores=a["output_scores"],
                                             watch_ids=a["watch_ids"], draft=a["draft"], draft_k=a["draft_k"])
        self.last_generate_stats = self.llama.last_generate_stats
        if a["output_scores"]:
            ids, sc = ids
            return {"token_ids": ids, "ve_anomaly_maps": maps, **sc}
        return {"token_ids": ids, "ve_anomaly_maps": maps}

    def score_answers(self, samples, candidates=None, candidate_ids=None, normalize: str = "sum", bos: bool = False):
        """Rank candidate answers by their teacher-forced log-likelihood after the prompt, nothing decoded (closed-set
        evaluation: BLIP-2's rank mode).  The prompt is generate()'s: finish_update, image, maps, encode_img, the stage-1 prompt
        layout, without the BOS as generate() wraps it, or with it for `bos=True` -- the training wrap, under which the score of a
        training answer is the training loss's own quantity.  Rows whose prompts differ in length are assembled one at a time.

        `candidates`: a list of strings shared by the batch, or one list per sample, tokenised as the training targets are --
        tok(c + end_sym, add_special_tokens=False), truncated to max_txt_len.  `candidate_ids` gives integer ids instead (a list
        of 1-D tensors / lists shared by the batch, or one such list per sample).  With neither, the two answers the model is
        trained on: [datasets.ABNORMAL_DESCRIBE, datasets.NORMAL_DESCRIBE].

        Returns {"answer_logprobs": [B, C] float64, the sum of each candidate's token log-probs (their mean with
        normalize="mean"; with per-sample lists of different sizes C is the largest and the missing entries are -inf),
        "answer_token_logprobs": per sample a list of f32 [n] tensors (LlamaHIP.score_continuations), "best": [B] int64, the
        arg-max with ties to the lower index, "candidate_ids": the ids scored, "ve_anomaly_maps": as generate() returns it}.
        `last_score_stats` holds the engine's counters."""
        if normalize not in ("sum", "mean"):
            raise ValueError(f"normalize must be 'sum' or 'mean', got {normalize!r}")
        self.finish_update()
        stage = 1 if self.arch == "myriad" else 0
        image = samples["image"].to(self._dev, F32)
        maps = None
        if self.arch == "myriad":
            key = "oneshot_anomaly_maps" if self.k_shot > 0 else "anomaly_maps"
            maps = self._maps_for(samples, key, image)
        B = image.shape[0]
        cand_ids = self._candidate_ids(B, candidates, candidate_ids)
        before, after = self._prompt_ids_rows(samples, B, stage)
        parts = self.encode_img(image, maps, stage, False)
        first = 1 if not bos else 0                                      # generate() wraps without BOS (myriad.py:446-449)
        if len({(int(b.shape[0]), int(a.shape[0])) for b, a in zip(before, after)}) == 1:
            emb, _, _, _ = self._assemble(parts, torch.stack(list(before)), torch.stack(list(after)), None, None)
            prompts = [emb[i, first:].contiguous() for i in range(B)]
        else:
            prompts = []
            for i in range(B):
                emb, _, _, _ = self._assemble([p[i:i + 1] for p in parts], before[i][None], after[i][None], None, None)
                prompts.append(emb[0, first:].contiguous())
        self.llama.decode_lora_version = self.store.version
        token_lp = self.llama.score_continuations(prompts, cand_ids)
        self.last_score_stats = self.llama.last_score_stats
        C = max(len(cs) for cs in cand_ids)
        lp = torch.full((B, C), float("-inf"), dtype=torch.float64)
        for i, row in enumerate(token_lp):
            for c, t in enumerate(row):
                total = t.double().sum()
                lp[i, c] = total / t.numel() if normalize == "mean" else total
        return {"answer_logprobs": lp, "answer_token_logprobs": token_lp, "best": lp.argmax(1), "candidate_ids": cand_ids,
                "ve_anomaly_maps": maps}

    def _candidate_ids(self, B: int, candidates, candidate_ids):
        """score_answers' candidates as ids: per sample a list of 1-D int64 tensors."""
        if candidates is not None and candidate_ids is not None:
            raise ValueError("pass candidates or candidate_ids, not both")
        if candidate_ids is not None:
            rows = list(candidate_ids)
            shared = not rows or torch.is_tensor(rows[0]) or not rows[0] or not hasattr(rows[0][0], "__len__")
            rows = [rows] * B if shared else rows
            if len(rows) != B:
                raise ValueError(f"candidate_ids: one list per sample, got {len(rows)} for a batch of {B}")
            return [[torch.as_tensor(c, dtype=torch.long).reshape(-1) for c in cs] for cs in rows]
        if candidates is None:
            from . import datasets
            candidates = [datasets.ABNORMAL_DESCRIBE, datasets.NORMAL_DESCRIBE]
        rows = list(candidates)
        rows = [rows] * B if not rows or isinstance(rows[0], str) else [list(r) for r in rows]
        if len(rows) != B:
            raise ValueError(f"candidates: one list per sample, got {len(rows)} for a batch of {B}")
        tok = self.llama_tokenizer
        if tok is None:
            raise RuntimeError("no tokenizer: pass integer ids (candidate_ids)")
        memo = {}
        for cs in rows:
            for c in cs:
                if c not in memo:                                        # as the training targets are (myriad.py:395-405)
                    ids = tok(c + self.end_sym, add_special_tokens=False).input_ids[:self.max_txt_len]
                    memo[c] = torch.tensor(ids, dtype=torch.long)
        return [[memo[c] for c in cs] for cs in rows]

    def _prompt_ids_rows(self, samples, B: int, stage: int):
        """_tokenize for an inference batch, one row at a time: lists of B 1-D id tensors whose lengths may differ."""
        if "before_ids" in samples:
            return [samples["before_ids"][i] for i in range(B)], [samples["after_ids"][i] for i in range(B)]
        tok = self.llama_tokenizer
        if tok is None:
            raise RuntimeError("no tokenizer: pass integer ids (before_ids/after_ids) in samples")
        key = {0: "question", 1: "question2", 2: "question3"}[stage] if self.arch == "myriad" else "question"
        bs, as_ = [], []
        for q in samples[key]:
            pb, pa = ("###Human: " + q + " ###Assistant: ").split("<ImageHere>")
            bs.append(tok(pb, return_tensors="pt", add_special_tokens=False).input_ids[0])
            as_.append(tok(pa, return_tensors="pt", add_special_tokens=False).input_ids[0])
        return bs, as_

    def generate_stream(self, batches, slots: int = 8, prefill_batch: int = 1, refill_min: int = 1, seeds=None, **generate_kwargs):
        """generate() for a whole run: `batches` (an iterable of generate()'s sample dicts, e.g. a DataLoader) streams through
        `slots` decode slots (LlamaHIP.slot_decoder).  Each batch is encoded as generate() encodes it (image, maps, encode_img at
        the batch's own size), each of its rows is tokenised and assembled on its own -- questions of different lengths are fine,
        `before_ids` / `after_ids` may be lists of 1-D tensors -- and decodes with its own position and its own stop rule: a row
        ends on EOS, on a stop sequence at the end of ITS ids or at max_new_tokens, and its slot takes the next row at once.

        Yields {"index", "token_ids": [L] int64 (CPU), "ve_anomaly_map"} per sample in input order (index counts samples
        over all batches), so a sampled run is reproducible per `generator`.  Takes generate()'s keyword arguments.  num_beams > 1
        is refused (NotImplementedError) unless `self.llama.slot_beams` (MYRIAD_SLOT_BEAMS=1, off by default) is on: then every
        sample is a beam search in its own group of num_beams slots (SlotDecoder.run; `slots` a multiple of num_beams), with
        length_penalty, early_stopping and num_return_sequences as in generate(); "token_ids" is what generate() returns in that
        sample's rows ([L] for one returned sequence, else [nrs, L], padded with EOS) and "sequences_scores" [nrs] comes with it;
        do_sample, repetition_penalty != 1 and seeds are refused there unless `self.llama.beam_sampling` is on as well: then they
        are beam sampling and the penalty per sample, sample i drawing from the i-th seed.  repetition_penalty != 1 needs the device sampling switch, as in
        generate(), and so does min_length > 1 here (SlotDecoder.run itself takes it on every path).  With that switch on, a
        sampled run draws every token on the device and each sample from its own stream: sample i takes the i-th seed drawn from `generator` (or the i-th of `seeds`, an iterable of ints), so its answer does not
        depend on the slot count, the refill settings or its neighbours (SlotDecoder.run).  min_length is a per-sample EOS ban.
        An unknown argument is a TypeError.  `last_generate_stats` holds the engine's counters (steps, prefills, graph_replays,
        graph_captures, live_row_steps, occupancy, prefill_passes, packed_rows, host_sampled_rows, device_sampled_rows) once the
        stream is exhausted.  `prefill_batch` = P > 1 prefills up to P waiting samples in one packed pass whenever slots are free
        and `refill_min` = k holds a refill back until k slots are free (SlotDecoder.run); both default to 1, the one-sample refill.
        output_scores / watch_ids as in generate(): each yielded dict gains "token_logprobs" [L] and "watch_logprobs" [L, W].
        draft=<drafter>, draft_k=K (generate()'s; slots * K <= 64; refused with NotImplementedError unless `self.llama.slot_draft`,
        MYRIAD_SLOT_DRAFT=1, off by default, is on): draft-and-verify decoding in the slots
        (SlotDecoder.run): the same token_ids as the call without them, in fewer passes over the decoder weights when the drafter
        guesses well.  `last_generate_stats` then also holds draft_k, draft_off, verify_steps, plain_steps, draft_proposed,
        draft_accepted, emitted, verify_graph_replays and plain_graph_replays.  Refused (NotImplementedError) with beams, and --
        unless `self.llama.draft_sampling` (MYRIAD_DRAFT_SAMPLING=1, off by default) is on -- with device sampling,
        repetition_penalty != 1, min_length > 1 and output_scores.  The caller teaches the drafter."""
        self.finish_update()
        a = self._generate_args(generate_kwargs)
        if a["draft"] is not None and not getattr(self.llama, "slot_draft", False):
            raise NotImplementedError("generate_stream(draft=...): draft decoding in the decode slots needs its switch "
                                      "(MYRIAD_SLOT_DRAFT=1 or model.llama.slot_draft = True)")
        draft_kw = {} if a["draft"] is None else dict(draft=a["draft"], draft_k=a["draft_k"])      # without: today's arguments
        nb, beam_kw = a["num_beams"], {}
        if nb > 1:
            if not getattr(self.llama, "slot_beams", False):
                raise NotImplementedError(f"generate_stream(num_beams={nb}): beam search in the decode slots needs its switch "
                                          "(MYRIAD_SLOT_BEAMS=1 or model.llama.slot_beams = True)")
            beam_sampling = bool(getattr(self.llama, "beam_sampling", False))
            if (a["do_sample"] or a["rep_pen"] != 1.0 or seeds is not None) and not beam_sampling:
                raise NotImplementedError(f"generate_stream(num_beams={nb}): do_sample, repetition_penalty != 1 and seeds are not "
                                          "implemented with beams in the decode slots")
            if nb > ops.BEAM_MAX or int(slots) % nb:
                raise ValueError(f"generate_stream(slots={slots}, num_beams={nb}): the slots divide into groups of num_beams <= "
                                 f"{ops.BEAM_MAX} rows")
            beam_kw = dict(num_beams=nb, **{k: a["beam_kw"][k] for k in ("length_penalty", "early_stopping", "num_return_sequences")})
            if beam_sampling:                                          # switch off: SlotDecoder.run is called with today's arguments
                beam_kw.update(do_sample=a["do_sample"], temperature=a["temperature"], top_k=a["top_k"], top_p=a["top_p"],
                               repetition_penalty=a["rep_pen"], generator=a["generator"], seeds=seeds)
        max_new = a["max_new"]
        if max_new is None:
            raise NotImplementedError("generate_stream(max_length=...): pass max_new_tokens, the prompts differ in length")
        if a["min_length"] > 1 and not self.llama.device_sampling:
            # the slot engine takes the per-row ban on every path (SlotDecoder.run); this entry keeps its earlier refusal
            # unless the device sampling switch is on, the same condition as the penalty's
            raise NotImplementedError(f"generate_stream(min_length={a['min_length']}) needs the device sampling switch "
                                      "(MYRIAD_DEVICE_SAMPLING=1 or model.llama.device_sampling = True)")
        stage = 1 if self.arch == "myriad" else 0
        side = []                                                      # per sample, in input order: its anomaly map

        def rows():
            for samples in batches:
                image = samples["image"].to(self._dev, F32)
                maps = None
                if self.arch == "myriad":
                    key = "oneshot_anomaly_maps" if self.k_shot > 0 else "anomaly_maps"
                    maps = self._maps_for(samples, key, image)
                B = image.shape[0]
                before, after = self._prompt_ids_rows(samples, B, stage)
                parts = self.encode_img(image, maps, stage, False)
                for i in range(B):
                    emb, _, _, _ = self._assemble([p[i:i + 1] for p in parts], before[i][None], after[i][None], None, None)
                    side.append(None if maps is None else maps[i])
                    yield emb[0, 1:].contiguous()                       # generate() wraps without BOS (myriad.py:446-449)

        self.llama.decode_lora_version = self.store.version
        # one engine (its caches and its captured step) per slot count, kept across calls; a slot holds slot_capacity positions
        # (prompt + generated: a few hundred in an evaluation run), a longer request is a ValueError that names the attribute
        key = (int(slots), min(int(self.slot_capacity), self.llama.cos.shape[0]))
        if self._slot_decoder is None or self._slot_decoder[0] != key:
            self._slot_decoder = None
            self._slot_decoder = (key, self.llama.slot_decoder(*key))
        dec = self._slot_decoder[1]

        def beam_stream():                                             # per sample what generate() returns in its rows
            for index, ids, scores, _ in dec.run(rows(), max_new_tokens=max_new, stop_ids=a["stops"], eos_id=a["eos_id"],
                                                 min_length=a["min_length"], ordered=True, prefill_batch=prefill_batch,
                                                 refill_min=refill_min, **beam_kw):
                self.last_generate_stats = dec.last_stats
                one = beam_kw["num_return_sequences"] == 1
                yield {"index": index, "token_ids": ids[0] if one else ids, "sequences_scores": scores,
                       "ve_anomaly_map": side[index]}
                side[index] = None
            self.last_generate_stats = dec.last_stats

        if nb > 1:
            return beam_stream()

        def stream():
            for index, ids, _, *sc in dec.run(rows(), max_new_tokens=max_new, stop_ids=a["stops"], eos_id=a["eos_id"],
                                              min_length=a["min_length"], do_sample=a["do_sample"], top_p=a["top_p"],
                                              temperature=a["temperature"], top_k=a["top_k"], generator=a["generator"], ordered=True,
                                              prefill_batch=prefill_batch, refill_min=refill_min, repetition_penalty=a["rep_pen"],
                                              seeds=seeds, return_scores=a["output_scores"], watch_ids=a["watch_ids"], **draft_kw):
                self.last_generate_stats = dec.last_stats
                yield {"index": index, "token_ids": ids, "ve_anomaly_map": side[index], **(sc[0] if sc else {})}
                side[index] = None
            self.last_generate_stats = dec.last_stats

        return stream()


class StoppingCriteriaSub:
    """`StoppingCriteriaSub` (conversation.py:96-107) for callers that build the criterion themselves: holds `stops`, and
    `__call__(input_ids, scores)` is the reference's row-0 suffix test.  `generate()` reads `.stops`."""

    def __init__(self, stops=(), encounters=1):
        self.stops = list(stops)

    def __call__(self, input_ids, scores=None):
        for stop in self.stops:
            stop = torch.as_tensor(stop).to(input_ids.device)
            if torch.all((stop == input_ids[0][-len(stop):])).item():
                return True
        return False


class MiniGPT4HIP(MyriadHIP):
    """`MiniGPT4` (reference mini_gpt4.py:14-307): ViT -> ln_vision -> Q-Former(32 queries) -> llama_proj -> LLaMA."""
    arch = "mini_gpt4"


registry.register_model("myriad")(MyriadHIP)
registry.register_model("mini_gpt4")(MiniGPT4HIP)
Myriad = MyriadHIP
MiniGPT4 = MiniGPT4HIP
