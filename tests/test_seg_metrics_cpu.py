"""Localisation metrics without a GPU: the numpy reference of tests/seg_metrics_ref.py against sklearn / scipy, the device-free
finalisation (eval_protocol.seg_metrics_from_hist) against sklearn and the reference PRO loop, and the host logic of SegMetrics,
the datasets' `with_gt_mask` and eval_aqa.py --seg-metrics.

Tolerances: AUROC / AP / F1 are sums of at most 2^20 fp64 terms of magnitude <= 1, each rounded to 2^-53: 1e-9 leaves three orders
of room (observed 0 on the 6 x 40 x 56 case).  AUPRO: each threshold's PRO is within 2^-24 = 6e-8 of the exact mean (the
floor of 2^40 / area), the normalised FPR axis spans 1, so the area is within 6e-8 plus rounding: 1e-7 (observed 1.7e-11)."""
import json
import os

import numpy as np
import pytest
import torch

from myriad_amd import _lib
from myriad_amd import datasets as D
from myriad_amd import eval_protocol as EP
from myriad_amd.seg_metrics import N_BINS, SegMetrics
from tests import seg_metrics_ref as R

SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 0.50001, 0.5001, -0.5, -0.50001, 1e-45, -1e-45, 1.17549435e-38, 3.4028235e38,
                     -3.4028235e38, 2.0, 1.9999999, 255.0, -1e-3], dtype=np.float32)


@pytest.fixture(scope="module")
def exact_case():
    masks, maps = R.make_case(6, 40, 56, seed=1, exact=True)
    hist, counters = R.hist_state(maps, masks)
    return masks, maps, hist, counters


@pytest.fixture(scope="module")
def generic_case():
    masks, maps = R.make_case(6, 40, 56, seed=2, exact=False)
    hist, counters = R.hist_state(maps, masks)
    return masks, maps, hist, counters


def _acc(hist, counters):
    return SegMetrics("cpu").merge({"hist": hist, "counters": counters})


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_metrics_equal_sklearn(generic_case):
    skm = pytest.importorskip("sklearn.metrics")
    masks, maps, _, _ = generic_case
    for scores in (maps, np.round(maps * 8) / 8):        # the second has heavy ties
        gt, s = masks.ravel(), scores.ravel()
        assert abs(R.auroc(gt, s) - skm.roc_auc_score(gt, s)) <= 1e-12
        assert abs(R.average_precision(gt, s) - skm.average_precision_score(gt, s)) <= 1e-12
        p, r, _ = skm.precision_recall_curve(gt, s)
        with np.errstate(divide="ignore", invalid="ignore"):
            f1 = 2 * p * r / (p + r)
        assert abs(R.f1_max(gt, s) - np.max(f1[np.isfinite(f1)])) <= 1e-12


def test_reference_labeller_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(0)
    cases = [rng.rand(33, 65) < p for p in (0.05, 0.3, 0.5, 0.7)] + [np.ones((5, 7), bool), np.zeros((5, 7), bool),
                                                                      np.eye(16, dtype=bool), R.make_case(1, 40, 56, 3)[0][0] != 0]
    for m in cases:
        lab, area, n = R.label8(m)
        ref, n_ref = ndi.label(m, structure=np.ones((3, 3)))
        assert n == n_ref
        want_lab = np.full(m.shape, -1, dtype=np.int64)
        want_area = np.zeros(m.shape, dtype=np.int64)
        for r in range(1, n_ref + 1):
            idx = np.nonzero((ref == r).ravel())[0]
            want_lab.ravel()[idx] = idx[0]
            want_area.ravel()[idx[0]] = len(idx)
        assert np.array_equal(lab, want_lab) and np.array_equal(area, want_area)


def test_key_and_bin_value():
    keys = EP.seg_key(SPECIALS)
    assert np.array_equal(keys, R.key_of(SPECIALS))
    assert keys[0] == keys[1]                            # -0 is +0
    assert 0 <= keys.min() and keys.max() < N_BINS
    order = np.argsort(SPECIALS, kind="stable")
    assert np.all(np.diff(keys[order]) >= 0)             # the key never reverses an order
    some = np.concatenate([keys, [1, N_BINS - 2, 1 << 19, (1 << 19) - 1]])
    assert np.array_equal(EP.seg_bin_value(some).view(np.uint32), R.bin_value(some).view(np.uint32))
    vals = EP.seg_bin_value(keys)
    assert np.array_equal(EP.seg_key(vals), keys)        # a bin's value lies in the bin ...
    canon = np.where(SPECIALS == 0, np.float32(0), SPECIALS)
    assert np.all(vals <= canon)                         # ... and is its smallest member
    inner = keys > int(EP.seg_key(np.array([-3.4028235e38], dtype=np.float32))[0])          # the float below -FLT_MAX's bin is -inf
    assert np.all(EP.seg_key(np.nextafter(vals[inner], np.float32(-np.inf))) == keys[inner] - 1)
    # a bf16 score is keyed exactly: distinct bf16 values, distinct keys, value = the score
    bf = torch.arange(-(1 << 15), 1 << 15, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float().numpy()
    bf = bf[np.isfinite(bf) & (bf >= 0)]
    assert np.array_equal(EP.seg_bin_value(EP.seg_key(bf)), np.where(bf == 0, np.float32(0), bf))


# ------------------------------------------------------------------------------------------------ finalisation
def test_finalisation_of_key_exact_scores_equals_sklearn_and_the_pro_loop(exact_case):
    skm = pytest.importorskip("sklearn.metrics")
    masks, maps, hist, counters = exact_case
    res = EP.seg_metrics_from_hist(hist[0], hist[1], hist[2], int(counters[2]))
    gt, s = masks.ravel(), maps.ravel()
    p, r, _ = skm.precision_recall_curve(gt, s)
    with np.errstate(divide="ignore", invalid="ignore"):
        f1 = 2 * p * r / (p + r)
    errs = {"auroc_px": abs(res["auroc_px"] - skm.roc_auc_score(gt, s)), "ap_px": abs(res["ap_px"] - skm.average_precision_score(gt, s)),
            "f1_px": abs(res["f1_px"] - np.max(f1[np.isfinite(f1)]))}
    pro_err = abs(res["aupro"] - R.pro_score(masks, maps))
    print("errors against sklearn", errs, "aupro against the loop", pro_err)
    assert all(e <= 1e-9 for e in errs.values()), errs
    assert pro_err <= 1e-7
    assert abs(res["auroc_px"] - R.auroc(gt, s)) <= 1e-9 and abs(res["ap_px"] - R.average_precision(gt, s)) <= 1e-9
    assert (res["n_pixels"], res["n_anomalous"], res["n_regions"]) == (masks.size, int(masks.sum()), int(counters[2]))
    assert res["auroc_px_tie_bound"] >= 0.0
    # other curve parameters take the same path
    for max_step, fpr in ((50, 0.3), (200, 0.05), (7, 1.0)):
        got = EP.seg_metrics_from_hist(hist[0], hist[1], hist[2], int(counters[2]), max_step, fpr)["aupro"]
        assert abs(got - R.pro_score(masks, maps, max_step, fpr)) <= 1e-7


def test_generic_fp32_scores_stay_inside_the_tie_bound(generic_case):
    skm = pytest.importorskip("sklearn.metrics")
    masks, maps, hist, counters = generic_case
    res = EP.seg_metrics_from_hist(hist[0], hist[1], hist[2], int(counters[2]))
    err = abs(res["auroc_px"] - skm.roc_auc_score(masks.ravel(), maps.ravel()))
    print("auroc error", err, "tie bound", res["auroc_px_tie_bound"])
    assert err <= res["auroc_px_tie_bound"] < 1e-3       # inside the bound, and a bound that says something
    # the four numbers are the reference's formulas on the truncated maps
    trunc = R.snap(maps)
    assert abs(res["auroc_px"] - R.auroc(masks.ravel(), trunc.ravel())) <= 1e-9
    assert abs(res["ap_px"] - R.average_precision(masks.ravel(), trunc.ravel())) <= 1e-9
    assert abs(res["f1_px"] - R.f1_max(masks.ravel(), trunc.ravel())) <= 1e-9
    assert abs(res["aupro"] - R.pro_score(masks, trunc)) <= 1e-7


def test_pro_edge_returns_nan_like_the_reference():
    """Every kept point at one FPR: the reference's min-max normalisation divides 0 by 0."""
    neg, pos, w = (np.zeros(N_BINS, dtype=np.int64) for _ in range(3))
    lo, hi = (int(k) for k in EP.seg_key(np.array([0.25, 0.75], dtype=np.float32)))
    neg[lo], pos[hi], w[hi] = 10, 4, 4 * ((1 << 40) // 4)
    with np.errstate(all="ignore"):
        res = EP.seg_metrics_from_hist(neg, pos, w, 1)
    assert res["auroc_px"] == 1.0 and res["ap_px"] == 1.0 and res["f1_px"] == 1.0 and np.isnan(res["aupro"])


# ------------------------------------------------------------------------------------------------ SegMetrics on the host
def test_merge_is_associative_and_commutative_and_save_load_round_trips(exact_case, tmp_path):
    masks, maps, hist, counters = exact_case
    parts = [R.hist_state(maps[i:i + 2], masks[i:i + 2]) for i in (0, 2, 4)]
    a, b, c = ({"hist": h, "counters": k} for h, k in parts)
    whole = _acc(hist, counters).state()

    def same(x, y):
        return np.array_equal(x["hist"], y["hist"]) and np.array_equal(x["counters"], y["counters"])

    ab_c = SegMetrics("cpu").merge(SegMetrics("cpu").merge(a).merge(b)).merge(c).state()
    a_bc = SegMetrics("cpu").merge(a).merge(SegMetrics("cpu").merge(b).merge(c)).state()
    cba = SegMetrics("cpu").merge(c).merge(b).merge(a).state()
    assert same(ab_c, whole) and same(a_bc, whole) and same(cba, whole)
    path = str(tmp_path / "state.npz")
    _acc(hist, counters).save(path)
    assert os.path.exists(path) and os.path.getsize(path) < (1 << 20)
    back = SegMetrics.load(path)
    assert same(back.state(), whole) and back.compute() == _acc(hist, counters).compute()
    # the shards of a sharded evaluation, merged by the helper next to merge_shards
    paths = []
    for k, p in enumerate((a, b, c)):
        paths.append(str(tmp_path / f"res.seg.rank{k}.npz"))
        SegMetrics("cpu").merge(p).save(paths[-1])
    out = str(tmp_path / "res.seg.json")
    assert EP.merge_seg_shards(paths[::-1], out) == _acc(hist, counters).compute() == json.load(open(out))
    with pytest.raises(ValueError):
        SegMetrics("cpu").merge({"hist": hist[:2], "counters": counters})
    with pytest.raises(ValueError):
        SegMetrics("cpu").merge({"hist": hist.astype(np.int32), "counters": counters})


def test_update_refuses_bad_arguments_before_any_launch():
    sm = SegMetrics("cpu")
    f32, u8 = torch.zeros(2, 8, 8), torch.zeros(2, 8, 8, dtype=torch.uint8)
    for maps, masks in ((f32, u8[:1]), (f32, torch.zeros(2, 8, 9, dtype=torch.uint8)), (f32[0], u8[0]), (f32[:, None, None], u8),
                        (f32.double(), u8), (f32.half(), u8), (f32, u8.float()), (f32, u8.long()), (f32[:0], u8[:0]),
                        (torch.zeros(2, 2, 8, 8), torch.zeros(2, 2, 8, 8, dtype=torch.uint8)),
                        (torch.zeros(1, 257, 256), torch.zeros(1, 257, 256, dtype=torch.uint8)),
                        (f32.numpy(), u8)):
        with pytest.raises(ValueError):
            sm.update(maps, masks)
    with pytest.raises(ValueError, match="65536"):
        sm.update(torch.zeros(1, 1, 257, 256), torch.zeros(1, 1, 257, 256, dtype=torch.bool))
    with pytest.raises(_lib.MyriadHipError, match="no CPU"):     # valid arguments, but no device: never an eager fallback
        sm.update(f32, u8)
    assert int(sm.state()["counters"].sum()) == 0


def test_compute_refuses_states_it_cannot_score(exact_case):
    _, _, hist, counters = exact_case
    bad = counters.copy()
    bad[3] = 17
    with pytest.raises(ValueError, match="17"):
        _acc(hist, bad).compute()
    with pytest.raises(ValueError, match="0 anomalous"):
        _acc(np.stack([hist[0], hist[1] * 0, hist[2] * 0]), np.array([counters[0] - counters[1], 0, 0, 0])).compute()
    with pytest.raises(ValueError, match="0 normal"):
        _acc(np.stack([hist[0] * 0, hist[1], hist[2]]), np.array([counters[1], counters[1], counters[2], 0])).compute()
    with pytest.raises(ValueError, match="anomalous"):
        SegMetrics("cpu").compute()
    many = counters.copy()
    many[2] = 1 << 22
    with pytest.raises(ValueError, match="2\\^22"):
        _acc(hist, many).compute()
    many[2] = (1 << 22) - 1
    assert np.isfinite(_acc(hist, many).compute()["aupro"])
    with pytest.raises(ValueError):
        EP.seg_metrics_from_hist(hist[0][:-1], hist[1][:-1], hist[2][:-1], 3)


# ------------------------------------------------------------------------------------------------ datasets
def test_synthetic_dataset_gt_mask():
    plain = D.SyntheticAnomalyDataset(n=6, seed=3, train=False, image_size=32)
    with_mask = D.build_datasets({"synthetic": {"num_samples": 6, "seed": 3, "image_size": 32, "with_gt_mask": True}}, "test")["synthetic"]
    assert "gt_mask" not in plain[1] and "gt_mask" not in D.build_datasets({"synthetic": {"num_samples": 2}}, "test")["synthetic"][1]
    for i in range(6):
        a, b = plain[i], with_mask[i]
        assert set(b) == set(a) | {"gt_mask"}
        assert all(torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k] for k in a)     # nothing else moves
        m = b["gt_mask"]
        assert m.shape == (1, 32, 32) and m.dtype == torch.uint8 and set(m.unique().tolist()) <= {0, 1}
        assert bool(m.any()) == b["is_anomaly"]          # zeros for a good sample, a defect for an anomalous one
        assert torch.equal(m, with_mask[i]["gt_mask"])   # seeded
    assert not torch.equal(with_mask[1]["gt_mask"], with_mask[3]["gt_mask"])
    batch = D.collate([with_mask[i] for i in range(4)])
    assert batch["gt_mask"].shape == (4, 1, 32, 32) and batch["gt_mask"].dtype == torch.uint8


def test_anomaly_detection_dataset_gt_mask(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    root = tmp_path / "data"
    rel = {"bad": "mvtec/bottle/test/broken/000.jpg", "good": "mvtec/bottle/test/good/001.jpg", "lost": "mvtec/bottle/test/broken/002.jpg"}
    rng = np.random.RandomState(0)
    for p in rel.values():
        os.makedirs(root / os.path.dirname(p), exist_ok=True)
        Image.fromarray(rng.randint(0, 255, (48, 64, 3), dtype=np.uint8)).save(root / p)
    gt = np.zeros((48, 64), dtype=np.uint8)
    gt[10:30, 20:50] = 7                                  # any value > 0 is anomalous
    gt_path = root / "mvtec/bottle/ground_truth/test/broken/000.png"
    os.makedirs(gt_path.parent)
    Image.fromarray(gt).save(gt_path)
    with open(root / "ann.jsonl", "w") as f:
        for k in ("bad", "good", "lost"):
            f.write(json.dumps({"img_path": rel[k], "caption": "", "is_anomaly": "0" if k == "good" else "1"}) + "\n")
    assert D.AnomalyDetectionDataset.gt_mask_path(str(root / rel["bad"])) == str(gt_path)
    ds = D.AnomalyDetectionDataset(str(root), ["ann.jsonl"], img_size=24, crop_size=24, stage="test", with_gt_mask=True)
    assert "gt_mask" not in D.AnomalyDetectionDataset(str(root), ["ann.jsonl"], img_size=24, crop_size=24, stage="test")[0]
    bad, good = ds[0], ds[1]
    assert bad["gt_mask"].shape == good["gt_mask"].shape == (1, 24, 24) and bad["gt_mask"].dtype == torch.uint8
    assert not bool(good["gt_mask"].any())
    # resized and cropped like the image (48 x 64 -> 24 x 32 -> the centre 24 x 24), nearest sampling
    want = np.asarray(Image.fromarray((gt > 0).astype(np.uint8) * 255).resize((32, 24), Image.NEAREST).crop((4, 0, 28, 24))) > 0
    assert np.array_equal(bad["gt_mask"][0].numpy() != 0, want) and want.any() and not want.all()
    assert set(bad["gt_mask"].unique().tolist()) == {0, 1}
    with pytest.raises(FileNotFoundError, match="ground_truth/test/broken/002.png"):
        ds[2]


# ------------------------------------------------------------------------------------------------ the entry point
def test_eval_entry_point_seg_arguments(tmp_path):
    import eval_aqa
    a = eval_aqa.parse_args(["--cfg-path", "x.yaml"])
    assert a.seg_metrics is False
    a = eval_aqa.parse_args(["--cfg-path", "x.yaml", "--seg-metrics", "--seg-max-step", "50", "--seg-expect-fpr", "0.1"])
    assert (a.seg_metrics, a.seg_max_step, a.seg_expect_fpr) == (True, 50, 0.1)
    for bad in (["--seg-max-step", "50"], ["--seg-expect-fpr", "0.1"], ["--seg-metrics", "--seg-max-step", "0"],
                ["--seg-metrics", "--seg-expect-fpr", "0"], ["--seg-metrics", "--seg-expect-fpr", "1.5"]):
        with pytest.raises(SystemExit):
            eval_aqa.parse_args(["--cfg-path", "x.yaml", *bad])
    assert eval_aqa.seg_paths("out/res.jsonl") == ("out/res.seg.json", None)
    assert eval_aqa.seg_paths("out/res.jsonl", world=4, rank=2) == (None, "out/res.seg.rank2.npz")
    assert eval_aqa.seg_paths("out/res.rank2.jsonl", world=4, rank=2) == (None, "out/res.seg.rank2.npz")
    sm = SegMetrics("cpu")
    with pytest.raises(KeyError, match="gt_mask"):
        eval_aqa.seg_gt({"image": torch.zeros(1, 3, 8, 8)})
    gt = torch.zeros(1, 1, 8, 8, dtype=torch.uint8)
    assert eval_aqa.seg_gt({"gt_mask": gt}) is gt
    with pytest.raises(KeyError, match="ve_anomaly_maps"):
        eval_aqa.seg_update(sm, None, gt, "cpu")
