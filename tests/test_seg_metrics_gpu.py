"""Localisation metrics on the GPU (csrc/seg_metrics.hip, myriad_amd/seg_metrics.py): mask_components and seg_hist_update bit for
bit against the numpy reference of tests/seg_metrics_ref.py, SegMetrics.compute() end to end at the tolerances derived in
tests/test_seg_metrics_cpu.py, and eval_aqa.py --seg-metrics."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from myriad_amd.seg_metrics import N_BINS, SegMetrics  # noqa: E402
from tests import seg_metrics_ref as R  # noqa: E402

DEV = "cuda"
BORDER, SENTINEL = 64, -77777
SHAPES = [(5, 7), (16, 16), (33, 65), (224, 224), (256, 256)]


def patterns(H, W):
    rng = np.random.RandomState(H * 1000 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    p = {"empty": np.zeros((H, W), bool), "full": np.ones((H, W), bool)}
    p["corners"] = np.zeros((H, W), bool)
    p["corners"][[0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]] = True
    p["diagonal"] = yy == xx                                             # one region under 8-connectivity
    p["row_end_and_next_row_start"] = np.zeros((H, W), bool)             # linear neighbours, not pixel neighbours: two regions
    p["row_end_and_next_row_start"][[H // 2 - 1, H // 2], [W - 1, 0]] = True
    p["lattice"] = (yy % 2 == 0) & (xx % 2 == 0)                         # the most regions an image can hold
    serp = (yy % 2 == 0)                                                 # one pixel wide through the whole image
    serp |= (yy % 4 == 1) & (xx == W - 1)
    serp |= (yy % 4 == 3) & (xx == 0)
    p["serpentine"] = serp
    p["checkerboard"] = (yy + xx) % 2 == 0                               # one region through diagonals
    p["blobs"] = R.make_case(1, H, W, seed=H + W)[0][0] != 0
    p["noise"] = rng.rand(H, W) < 0.4                                    # near the percolation threshold: ragged regions
    return p


def bordered(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * BORDER,), SENTINEL, dtype=torch.int32, device=DEV)
    return buf, buf[BORDER:BORDER + n].view(shape)


def run_components(masks_np):
    B, H, W = masks_np.shape
    bufs = [bordered(s) for s in ((B, H, W), (B, H, W), (B,))]
    out = ops.mask_components(torch.from_numpy(masks_np).to(DEV), out=tuple(v for _, v in bufs))
    for (buf, _), name in zip(bufs, ("labels", "area", "n_regions")):
        assert bool((buf[:BORDER] == SENTINEL).all()) and bool((buf[-BORDER:] == SENTINEL).all()), f"{name}: border written"
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("H,W", SHAPES)
def test_mask_components_equals_the_numpy_labeller(H, W):
    pats = patterns(H, W)
    names = list(pats)
    want = {k: R.label8(pats[k]) for k in names}
    assert want["diagonal"][2] == 1 and want["row_end_and_next_row_start"][2] == 2 and want["serpentine"][2] == 1
    assert want["checkerboard"][2] == 1 and want["lattice"][2] == ((H + 1) // 2) * ((W + 1) // 2)
    assert want["full"][1][0, 0] == H * W and want["corners"][2] == (4 if min(H, W) > 2 else 1)
    groups, i = [], 0
    for b in (1, 2, 3, 3, 1):                             # B = 1 .. 3, uint8 and bool
        groups.append(names[i:i + b])
        i += b
    assert i == len(names)
    for g, group in enumerate(groups):
        m = np.stack([pats[k] for k in group])
        labels, area, n = run_components(m if g % 2 else m.astype(np.uint8) * (1 + g))     # any nonzero byte is anomalous
        for j, k in enumerate(group):
            assert n[j] == want[k][2], (k, n[j], want[k][2])
            assert np.array_equal(labels[j], want[k][0]), k
            assert np.array_equal(area[j], want[k][1]), k
            assert np.all(labels[j][~pats[k]] == -1)


def test_mask_components_extreme_aspect_and_refusals():
    for H, W in ((4, 16384), (16384, 4), (1, 300), (300, 1), (2, 2), (1, 1)):
        m = np.random.RandomState(H + W).rand(1, H, W) < 0.5
        labels, area, n = run_components(m)
        want = R.label8(m[0])
        assert n[0] == want[2] and np.array_equal(labels[0], want[0]) and np.array_equal(area[0], want[1])
    for H, W in ((257, 256), (1, 65537), (1, 65536)):     # too many pixels; too many 2 x 2 blocks for the LDS
        with pytest.raises(_lib.MyriadHipError, match="LDS"):
            ops.mask_components(torch.zeros(1, H, W, dtype=torch.uint8, device=DEV))
    big = torch.zeros(1, 257, 256, dtype=torch.uint8, device=DEV)                # the C entry refuses by itself as well
    outs = [torch.full(s, SENTINEL, dtype=torch.int32, device=DEV) for s in ((1, 257, 256), (1, 257, 256), (1,))]
    assert ops._L().mh_mask_components(big.data_ptr(), *(t.data_ptr() for t in outs), 1, 257, 256, ops._s()) == -1
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in outs)
    with pytest.raises(_lib.MyriadHipError):
        ops.mask_components(torch.zeros(1, 8, 8, dtype=torch.float32, device=DEV))
    with pytest.raises(_lib.MyriadHipError):
        ops.mask_components(torch.zeros(2, 8, 8, dtype=torch.uint8, device=DEV)[:, :, ::2])


# ------------------------------------------------------------------------------------------------ seg_hist_update
def special_case(flat):
    """3 x 33 x 65 (26 workgroups, rows off every vector grid): generic scores with every special value planted on anomalous and on
    normal pixels; flat: two values only, a whole wave on one bin."""
    masks, maps = R.make_case(3, 33, 65, seed=11)
    masks[2, 3:9, 50:65] = 1                              # the 'good' image gets a region too: areas differ inside a wave
    if flat:
        maps = np.where(np.random.RandomState(5).rand(*maps.shape) < 0.9, np.float32(0.25), np.float32(0.5)).astype(np.float32)
    fmax, tiny = np.float32(3.4028235e38), np.float32(1e-45)
    specials = [np.float32(-0.0), np.float32(0.0), np.float32(-1.5), np.float32(-1.5000001), fmax, -fmax, tiny, -tiny,
                np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(1)), np.float32("nan"), np.float32("inf"),
                np.float32("-inf"), -np.float32("nan")]
    flat_idx = np.random.RandomState(7).permutation(maps.size)
    pos_idx, neg_idx = flat_idx[masks.ravel()[flat_idx] != 0], flat_idx[masks.ravel()[flat_idx] == 0]
    for j, v in enumerate(specials):
        maps.ravel()[pos_idx[j]] = v
        maps.ravel()[neg_idx[j]] = v
        maps.ravel()[neg_idx[j + len(specials)]] = v      # twice among the normal pixels: two lanes, one bin
    return masks, maps


def fresh():
    return torch.zeros((3, N_BINS), dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)


def accumulate(maps_t, masks_t, order, aggregate):
    hist, counters = fresh()
    for idx in order:
        idx = list(idx)
        mk = masks_t[idx].contiguous()
        labels, area, _ = ops.mask_components(mk)
        ops.seg_hist_update(hist, counters, maps_t[idx].contiguous(), mk, labels, area, aggregate=aggregate)
    return hist, counters


@pytest.mark.parametrize("aggregate", [True, False])
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_seg_hist_update_equals_the_numpy_histograms(dtype, flat, aggregate):
    masks, maps = special_case(flat)
    maps_t = torch.from_numpy(maps).to(DEV).to(dtype)
    masks_t = torch.from_numpy(masks).to(DEV)
    ref_hist, ref_counters = R.hist_state(maps_t.float().cpu().numpy(), masks)
    assert ref_counters[3] >= 8 and ref_counters[2] >= 3
    hist, counters = accumulate(maps_t, masks_t, [(0, 1, 2)], aggregate)
    assert np.array_equal(counters.cpu().numpy(), ref_counters), (counters, ref_counters)
    got = hist.cpu().numpy()
    for row in range(3):
        assert np.array_equal(got[row], ref_hist[row]), f"row {row}: {int((got[row] != ref_hist[row]).sum())} bins differ"
    assert int(got[0].sum() + got[1].sum()) == masks.size - ref_counters[3]            # a non-finite score is in no row
    for order in ([(0,), (1,), (2,)], [(2,), (0,), (1,)], [(1, 2), (0,)], [(2, 1, 0)]):
        h2, c2 = accumulate(maps_t, masks_t, order, aggregate)
        assert torch.equal(h2, hist) and torch.equal(c2, counters), order
    again = accumulate(maps_t, masks_t, [(0, 1, 2)], not aggregate)                   # the other atomic shape: the same sums
    assert torch.equal(again[0], hist) and torch.equal(again[1], counters)


def test_seg_hist_update_refuses_bad_arguments():
    hist, counters = fresh()
    mk = torch.zeros(1, 8, 8, dtype=torch.uint8, device=DEV)
    labels, area, _ = ops.mask_components(mk)
    maps = torch.zeros(1, 8, 8, device=DEV)
    for bad in (dict(hist=hist[:2]), dict(hist=hist.int()), dict(counters=counters[:3]), dict(maps=maps.half()),
                dict(maps=torch.zeros(1, 8, 9, device=DEV)), dict(labels=labels.long()), dict(area=area[:, :4]),
                dict(masks=mk.float()), dict(maps=maps.cpu())):
        kw = dict(hist=hist, counters=counters, maps=maps, masks=mk, labels=labels, area=area)
        kw.update(bad)
        with pytest.raises(_lib.MyriadHipError):
            ops.seg_hist_update(**kw)
    assert int(hist.sum()) == 0 and int(counters.sum()) == 0


# ------------------------------------------------------------------------------------------------ SegMetrics end to end
def check_against_reference(res, masks, maps_scored):
    gt, s = masks.ravel(), maps_scored.ravel()
    errs = {"auroc_px": abs(res["auroc_px"] - R.auroc(gt, s)), "ap_px": abs(res["ap_px"] - R.average_precision(gt, s)),
            "f1_px": abs(res["f1_px"] - R.f1_max(gt, s)), "aupro": abs(res["aupro"] - R.pro_score(masks, maps_scored))}
    print("errors against the numpy reference", errs)
    assert errs["auroc_px"] <= 1e-9 and errs["ap_px"] <= 1e-9 and errs["f1_px"] <= 1e-9 and errs["aupro"] <= 1e-7, errs


def test_compute_end_to_end_on_key_exact_scores():
    masks, maps = R.make_case(6, 40, 56, seed=1, exact=True)
    maps_t, masks_t = torch.from_numpy(maps).to(DEV), torch.from_numpy(masks).to(DEV)
    one = SegMetrics(DEV)
    one.update(maps_t[:, None], masks_t[:, None])         # [B, 1, H, W]
    res = one.compute()
    check_against_reference(res, masks, maps)
    labelled = R.label8_batch(masks)[2].sum()
    assert (res["n_pixels"], res["n_anomalous"], res["n_regions"]) == (masks.size, int(masks.sum()), int(labelled))
    # two accumulators merged = one; host masks and bool masks are taken as well
    a, b = SegMetrics(DEV), SegMetrics(DEV)
    a.update(maps_t[:4], masks_t[:4].bool())
    b.update(maps_t[4:, None], torch.from_numpy(masks[4:, None]))
    merged = SegMetrics(DEV).merge(b).merge(a.state())
    sa, sb = merged.state(), one.state()
    assert np.array_equal(sa["hist"], sb["hist"]) and np.array_equal(sa["counters"], sb["counters"])
    assert merged.compute() == res
    ref_hist, ref_counters = R.hist_state(maps, masks)
    assert np.array_equal(sb["hist"], ref_hist) and np.array_equal(sb["counters"], ref_counters)
    for max_step, fpr in ((50, 0.3), (200, 0.05)):
        assert abs(one.compute(max_step, fpr)["aupro"] - R.pro_score(masks, maps, max_step, fpr)) <= 1e-7


def test_compute_end_to_end_on_fp32_maps_at_full_size():
    masks, maps = R.make_case(2, 224, 224, seed=4)
    masks[1, 100:120, 30:90] = 1
    sm = SegMetrics(DEV)
    sm.update(torch.from_numpy(maps).to(DEV), torch.from_numpy(masks).to(DEV))
    res = sm.compute()
    check_against_reference(res, masks, R.snap(maps))     # the reference's formulas on the truncated maps
    err = abs(res["auroc_px"] - R.auroc(masks.ravel(), maps.ravel()))
    print("auroc against the unquantised scores", err, "tie bound", res["auroc_px_tie_bound"])
    assert err <= res["auroc_px_tie_bound"] < 1e-3
    bf = torch.from_numpy(maps).to(DEV).bfloat16()        # bf16: distinct scores keep distinct keys; a bin stands for its smallest
    sb = SegMetrics(DEV)                                  # member, which for a negative score lies below the score
    sb.update(bf, torch.from_numpy(masks).to(DEV))
    check_against_reference(sb.compute(), masks, R.snap(bf.float().cpu().numpy()))
    sp = SegMetrics(DEV)                                  # a non-negative bf16 map is scored exactly as it is
    sp.update(bf.abs(), torch.from_numpy(masks).to(DEV))
    check_against_reference(sp.compute(), masks, bf.abs().float().cpu().numpy())


def test_update_errors_and_non_finite_scores_on_the_device():
    sm = SegMetrics(DEV)
    maps, masks = torch.rand(2, 16, 16, device=DEV), torch.zeros(2, 16, 16, dtype=torch.uint8, device=DEV)
    masks[0, 2:5, 2:5] = 1
    with pytest.raises(ValueError):
        sm.update(maps, masks[:1])
    with pytest.raises(ValueError, match="65536"):
        sm.update(torch.zeros(1, 257, 256, device=DEV), torch.zeros(1, 257, 256, dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.MyriadHipError):
        sm.update(maps.cpu(), masks)
    assert int(sm.state()["counters"].sum()) == 0
    maps[1, 0, 0], maps[0, 3, 3] = float("nan"), float("inf")
    sm.update(maps, masks)
    assert sm.state()["counters"].tolist() == [512, 9, 1, 2]
    with pytest.raises(ValueError, match="2 of 512"):
        sm.compute()


# ------------------------------------------------------------------------------------------------ the entry point
def test_eval_entry_point_writes_the_seg_metrics(tmp_path, monkeypatch):
    import eval_aqa
    from myriad_amd.myriad import MyriadHIP
    from tests import disk_fixture
    fx = disk_fixture.build(str(tmp_path / "ref_files"))
    seen = []
    gen = MyriadHIP.generate

    def spy_generate(self, samples, **kw):
        out = gen(self, samples, **kw)
        seen.append((out["ve_anomaly_maps"].detach().clone(), samples["gt_mask"].clone()))
        return out

    monkeypatch.setattr(MyriadHIP, "generate", spy_generate)
    res = str(tmp_path / "res.jsonl")
    path, records = eval_aqa.main(["--cfg-path", fx["eval_yaml"], "--dataset", "synthetic", "--bs", "2", "--limit", "2",
                                   "--seg-metrics", "--out", res])
    assert len(records) == 4 and len(seen) == 2
    want = SegMetrics(DEV)
    for maps, gt in seen:
        assert gt.shape[0] == 2 and gt.dtype == torch.uint8
        want.update(maps.to(DEV), gt)
    got = json.load(open(str(tmp_path / "res.seg.json")))
    assert got == want.compute() and got["n_pixels"] == 4 * seen[0][1][0].numel() and got["n_regions"] >= 2
    # the slot loop feeds the same maps one by one: the same integers, so the same file; a rank of a sharded run saves its state
    eval_aqa.main(["--cfg-path", fx["eval_yaml"], "--dataset", "synthetic", "--bs", "2", "--limit", "2", "--slots", "2",
                   "--seg-metrics", "--out", str(tmp_path / "slots.jsonl")])
    assert json.load(open(str(tmp_path / "slots.seg.json"))) == got
