#!/usr/bin/env python3
"""Time the streaming localisation metrics (myriad_amd/seg_metrics.py) against the host protocol on the same data.

    python tools/seg_metrics_bench.py [--n 256] [--bs 8] [--size 224] [--rounds 5] [--skip-host]

N synthetic maps of size x size in batches of bs, two score distributions: `noise` (every pixel its own fp32 score: equal keys
are rare inside a wave) and `flat` (a constant background with scores on and around the defects, as a sharp expert map has it:
whole waves on one bin).  Per distribution and per atomic shape (aggregate = 1: equal keys of a wave add once; 0: one atomic
per lane) the HIP-event time of one SegMetrics.update, taken over a pass through all batches, as the median of `rounds` passes
with the two shapes alternating inside each round; the two kernels alone the same way; the wall time of compute(); and the wall
time of the host protocol -- sklearn's roc_auc_score / average_precision_score / precision_recall_curve where importable, else
the numpy sort of tests/seg_metrics_ref.py, plus that file's PRO loop (200 thresholds over every map; the reference's own loop
needs skimage).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_data(n, size, kind, seed=0):
    import numpy as np
    from tests import seg_metrics_ref as R
    masks, maps = R.make_case(n, size, size, seed=seed)
    masks[-1, size // 3:size // 2, size // 4:size // 2] = 1
    if kind == "flat":
        rng = np.random.RandomState(seed + 1)
        maps = np.where(masks != 0, 0.2 + 0.8 * rng.rand(*maps.shape), 0.05).astype(np.float32)
        halo = rng.rand(*maps.shape) < 0.02
        maps[halo] = rng.rand(int(halo.sum())).astype(np.float32)
    return masks, maps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    from myriad_amd import ops
    from myriad_amd.seg_metrics import SegMetrics
    from tests import seg_metrics_ref as R
    assert torch.cuda.is_available(), "this benchmark measures the GPU path; there is no fallback"
    dev = "cuda"
    n_batches = args.n // args.bs
    out = {"n": args.n, "bs": args.bs, "size": args.size, "rounds": args.rounds}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / n_batches       # us per batch

    for kind in ("noise", "flat"):
        masks, maps = make_data(args.n, args.size, kind)
        maps_b = [torch.from_numpy(maps[i:i + args.bs]).to(dev) for i in range(0, args.n, args.bs)]
        masks_b = [torch.from_numpy(masks[i:i + args.bs]).to(dev) for i in range(0, args.n, args.bs)]
        comps = [ops.mask_components(m) for m in masks_b]
        accs = {1: SegMetrics(dev), 0: SegMetrics(dev)}

        def run_update(agg):
            for mp, mk in zip(maps_b, masks_b):
                accs[agg].update(mp, mk, aggregate=bool(agg))

        def run_hist(agg):
            for mp, mk, (lab, area, _) in zip(maps_b, masks_b, comps):
                ops.seg_hist_update(accs[agg].hist, accs[agg].counters, mp, mk, lab, area, aggregate=bool(agg))

        def run_components():
            for mk in masks_b:
                ops.mask_components(mk)

        for agg in (1, 0):                               # warm-up: code objects, the allocator's blocks
            run_update(agg)
            run_hist(agg)
        run_components()
        torch.cuda.synchronize()
        t = {"update_agg1": [], "update_agg0": [], "hist_agg1": [], "hist_agg0": [], "components": []}
        for _ in range(args.rounds):                     # the variants alternate inside a round
            for agg in (1, 0):
                t[f"update_agg{agg}"].append(timed(lambda: run_update(agg)))
            for agg in (1, 0):
                t[f"hist_agg{agg}"].append(timed(lambda: run_hist(agg)))
            t["components"].append(timed(run_components))
        res = {k + "_us": round(statistics.median(v), 2) for k, v in t.items()}
        res.update({k + "_us_min_max": [round(min(v), 2), round(max(v), 2)] for k, v in t.items()})
        assert torch.equal(accs[1].hist, accs[0].hist) and torch.equal(accs[1].counters, accs[0].counters)

        one = SegMetrics(dev)                            # one clean pass: what an evaluation holds at its end
        for mp, mk in zip(maps_b, masks_b):
            one.update(mp, mk)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = one.compute()
        res["compute_s"] = round(time.perf_counter() - t0, 4)
        res["metrics"] = got
        if not args.skip_host:
            gt, s = masks.ravel(), maps.ravel()
            t0 = time.perf_counter()
            try:
                from sklearn.metrics import average_precision_score, precision_recall_curve, roc_auc_score
                auroc, apx = roc_auc_score(gt, s), average_precision_score(gt, s)
                p, r, _ = precision_recall_curve(gt, s)
                with np.errstate(divide="ignore", invalid="ignore"):
                    f1 = 2 * p * r / (p + r)
                f1 = float(np.max(f1[np.isfinite(f1)]))
                res["host_impl"] = "sklearn + numpy PRO loop"
            except ImportError:
                auroc, apx, f1 = R.auroc(gt, s), R.average_precision(gt, s), R.f1_max(gt, s)
                res["host_impl"] = "numpy"
            res["host_sort_metrics_s"] = round(time.perf_counter() - t0, 3)
            t0 = time.perf_counter()
            pro = R.pro_score(masks, maps)
            res["host_pro_s"] = round(time.perf_counter() - t0, 3)
            res["host_total_s"] = round(res["host_sort_metrics_s"] + res["host_pro_s"], 3)
            res["diff_to_host"] = {"auroc_px": abs(got["auroc_px"] - auroc), "ap_px": abs(got["ap_px"] - apx),
                                   "f1_px": abs(got["f1_px"] - f1), "aupro": abs(got["aupro"] - pro)}
        out[kind] = res
        print(f"# {kind}: {json.dumps(res)}", flush=True)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
