"""Streaming localisation metrics for anomaly maps: pixel AUROC / AP / F1-max and AUPRO (`ALEvaluator.eval_seg`,
scripts/eval_protocol/eval_align.py:281-343) at the end of an evaluation pass, without keeping a single map.

    sm = SegMetrics("cuda:0")
    for batch in loader:
        out = model.generate(batch, ...)
        sm.update(out["ve_anomaly_maps"], batch["gt_mask"])       # two launches on the current stream, no host sync
    print(sm.compute())                                           # one device -> host copy, then numpy in fp64

The state is a [3, 2^20] int64 histogram over a 20-bit key of the score (csrc/seg_metrics.hip) and four counters.  Rows 0 / 1
count the normal / anomalous pixels per key; row 2 receives floor(2^40 / area of its ground-truth region) per anomalous pixel,
which makes PRO a suffix sum as well: the mean over regions of tp_r(th) / area_r is the row's sum above th over n_regions 2^40,
off by at most 2^-24.  All adds are integer atomics, so the state does not depend on batching or arrival order, and the states of
the ranks of a sharded evaluation simply add (`state` / `merge` / `save` / `load`).

What compute() returns are the reference's formulas applied to the maps TRUNCATED to the 20-bit key (sign, exponent, 11 mantissa
bits; a bin stands for its smallest member, so a non-negative bf16 map is scored exactly and a negative score moves to the most
negative fp32 value of its bin).  For AUROC the effect is bounded: the value for the unquantised fp32 scores lies within
`auroc_px_tie_bound` of `auroc_px`.  For AP, F1-max and AUPRO no bound is claimed.  eval_protocol.seg_metrics_from_hist has the
arithmetic."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import _lib
from . import eval_protocol as EP
from . import ops

N_BINS = 1 << EP.SEG_KEY_BITS
MAX_PIXELS = 65536


class SegMetrics:
    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.hist = torch.zeros((3, N_BINS), dtype=torch.int64, device=self.device)
        self.counters = torch.zeros((4,), dtype=torch.int64, device=self.device)   # pixels, anomalous, regions, non-finite

    def update(self, maps: torch.Tensor, masks: torch.Tensor, aggregate: bool = True) -> None:
        """maps [B, H, W] or [B, 1, H, W] f32 / bf16 scores on the device; masks of the same shape, uint8 / bool, nonzero =
        anomalous (a host tensor is uploaded).  H * W <= 65536."""
        if not isinstance(maps, torch.Tensor) or not isinstance(masks, torch.Tensor):
            raise ValueError("SegMetrics.update: maps and masks must be tensors")
        if maps.dim() == 4 and maps.shape[1] == 1:
            maps = maps[:, 0]
        if masks.dim() == 4 and masks.shape[1] == 1:
            masks = masks[:, 0]
        if maps.dim() != 3 or masks.dim() != 3:
            raise ValueError(f"SegMetrics.update: need [B, H, W] or [B, 1, H, W], got maps {tuple(maps.shape)} masks "
                             f"{tuple(masks.shape)}")
        if tuple(maps.shape) != tuple(masks.shape):
            raise ValueError(f"SegMetrics.update: maps {tuple(maps.shape)} and masks {tuple(masks.shape)} differ in shape")
        if maps.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"SegMetrics.update: maps must be float32 or bfloat16, got {maps.dtype}")
        if masks.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"SegMetrics.update: masks must be uint8 or bool, got {masks.dtype}")
        B, H, W = maps.shape
        if B < 1 or H < 1 or W < 1:
            raise ValueError(f"SegMetrics.update: empty batch {tuple(maps.shape)}")
        if H * W > MAX_PIXELS:
            raise ValueError(f"SegMetrics.update: {H} x {W} maps: the component labelling keeps one image in LDS, "
                             f"H * W <= {MAX_PIXELS}")
        if self.device.type != "cuda" or maps.device != self.hist.device:
            raise _lib.MyriadHipError(f"SegMetrics.update runs on the GPU only (no CPU / eager fallback): accumulator on "
                                          f"{self.hist.device}, maps on {maps.device}")
        masks = masks.to(self.hist.device, non_blocking=True).contiguous()
        maps = maps.contiguous()
        labels, area, _ = ops.mask_components(masks)
        ops.seg_hist_update(self.hist, self.counters, maps, masks, labels, area, aggregate=aggregate)

    def state(self) -> Dict[str, np.ndarray]:
        """{"hist", "counters"} as numpy int64 (one device -> host copy)."""
        flat = torch.cat([self.hist.view(-1), self.counters]).cpu().numpy()
        return {"hist": flat[:3 * N_BINS].reshape(3, N_BINS).copy(), "counters": flat[3 * N_BINS:].copy()}

    def merge(self, state) -> "SegMetrics":
        """Add another accumulator's state (a `state()` dict or a SegMetrics)."""
        if isinstance(state, SegMetrics):
            state = state.state()
        hist, counters = np.asarray(state["hist"]), np.asarray(state["counters"])
        if hist.shape != (3, N_BINS) or counters.shape != (4,) or hist.dtype != np.int64 or counters.dtype != np.int64:
            raise ValueError(f"SegMetrics.merge: need int64 hist {(3, N_BINS)} and counters (4,), got {hist.dtype} {hist.shape} "
                             f"{counters.dtype} {counters.shape}")
        self.hist += torch.from_numpy(np.ascontiguousarray(hist)).to(self.device)
        self.counters += torch.from_numpy(np.ascontiguousarray(counters)).to(self.device)
        return self

    def save(self, path: str) -> None:
        with open(path, "wb") as f:                      # a file object: numpy appends no suffix
            np.savez_compressed(f, **self.state())

    @classmethod
    def load(cls, path: str, device="cpu") -> "SegMetrics":
        with np.load(path) as z:
            return cls(device).merge({"hist": z["hist"], "counters": z["counters"]})

    def compute(self, max_step: int = 200, expect_fpr: float = 0.3) -> dict:
        """{"auroc_px", "ap_px", "f1_px", "aupro", "auroc_px_tie_bound", "n_pixels", "n_anomalous", "n_regions"}; ValueError
        where a score was NaN / infinite, a class is missing or n_regions >= 2^22."""
        s = self.state()
        return EP.seg_metrics_from_state(s["hist"], s["counters"], max_step, expect_fpr)
