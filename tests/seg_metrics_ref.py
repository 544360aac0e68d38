"""Numpy-only reference for the localisation metrics (myriad_amd/seg_metrics.py, csrc/seg_metrics.hip), written from the
definitions: exact pixel AUROC / AP / F1-max by sorting, the PRO loop of `cal_pro_score` with a small union-find labeller, the
20-bit key, the smallest value of a bin, and the histograms / counters SegMetrics accumulates."""
import numpy as np

KEY_BITS = 20
N_BINS = 1 << KEY_BITS


# ------------------------------------------------------------------------------------------------ key
def key_of(scores) -> np.ndarray:
    """-0 -> +0; negative: every bit flipped, else the sign bit set; the top 20 bits."""
    x = np.asarray(scores, dtype=np.float32).copy()
    x[x == 0] = 0.0                                      # -0.0 == 0
    u = x.view(np.uint32).astype(np.uint64)
    neg = (u >> np.uint64(31)) == 1
    t = np.where(neg, np.uint64(0xFFFFFFFF) - u, u + np.uint64(0x80000000))
    return (t >> np.uint64(12)).astype(np.int64)


def bin_value(keys) -> np.ndarray:
    """The smallest fp32 value whose key is `keys`."""
    t = np.asarray(keys, dtype=np.uint64) << np.uint64(12)
    nonneg = t >= np.uint64(0x80000000)
    u = np.where(nonneg, t - np.uint64(0x80000000), np.uint64(0xFFFFFFFF) - t)
    return u.astype(np.uint32).view(np.float32)


def snap(scores) -> np.ndarray:
    """Scores moved to the value their bin stands for (key-representable)."""
    return bin_value(key_of(scores)).reshape(np.shape(scores))


# ------------------------------------------------------------------------------------------------ connected components
def label8(mask):
    """8-connected components of a 2-D mask -> (labels int32: -1 on background, else the smallest linear index of the component;
    area int32: the pixel count at that index, 0 elsewhere; number of regions).  Runs of a row are the union-find's elements; a run
    touches the runs of the row above that overlap it widened by one pixel on each side."""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    parent, runs = [], []

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    prev = []
    for y in range(H):
        d = np.diff(np.concatenate([[0], mask[y].astype(np.int8), [0]]))
        cur, j = [], 0
        for x0, x1 in zip(np.nonzero(d == 1)[0].tolist(), np.nonzero(d == -1)[0].tolist()):
            rid = len(parent)
            parent.append(rid)
            runs.append((y, x0, x1))
            while j < len(prev) and prev[j][1] < x0:    # prev run [p0, p1) ends left of x0 - 1
                j += 1
            k = j
            while k < len(prev) and prev[k][0] <= x1:   # starts at or before x1 (one past this run's last pixel)
                a, b = find(rid), find(prev[k][2])
                if a != b:
                    parent[max(a, b)] = min(a, b)       # run ids ascend in raster order of their first pixel
                k += 1
            j = max(j, k - 1)
            cur.append((x0, x1, rid))
        prev = cur
    labels = np.full((H, W), -1, dtype=np.int32)
    area = np.zeros((H, W), dtype=np.int32)
    n = 0
    for rid, (y, x0, x1) in enumerate(runs):
        r = find(rid)
        ry, rx0, _ = runs[r]
        labels[y, x0:x1] = ry * W + rx0
        area[ry, rx0] += x1 - x0
        n += r == rid
    return labels, area, int(n)


def label8_batch(masks):
    out = [label8(m) for m in masks]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32))


# ------------------------------------------------------------------------------------------------ exact metrics
def _curve(gt, score):
    """Cumulative (tp, fp) at every distinct score, descending."""
    gt = np.asarray(gt).ravel() != 0
    score = np.asarray(score, dtype=np.float64).ravel()
    order = np.argsort(-score, kind="mergesort")
    s, g = score[order], gt[order]
    last = np.nonzero(np.concatenate([s[1:] != s[:-1], [True]]))[0]
    tps = np.cumsum(g)[last].astype(np.float64)
    fps = (last + 1) - tps
    return tps, fps, int(g.sum()), int((~g).sum())


def auroc(gt, score) -> float:
    tps, fps, P, N = _curve(gt, score)
    tpr, fpr = np.concatenate([[0.0], tps / P]), np.concatenate([[0.0], fps / N])
    return float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0))


def average_precision(gt, score) -> float:
    tps, fps, P, _ = _curve(gt, score)
    recall = np.concatenate([[0.0], tps / P])
    return float(np.sum(np.diff(recall) * (tps / (tps + fps))))


def f1_max(gt, score) -> float:
    tps, fps, P, _ = _curve(gt, score)
    p, r = tps / (tps + fps), tps / P
    with np.errstate(divide="ignore", invalid="ignore"):
        f1 = 2 * p * r / (p + r)
    return float(np.max(f1[np.isfinite(f1)]))


def sk_auc(x, y) -> float:
    """The trapezoid area with sklearn.metrics.auc's direction rule."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    dx = np.diff(x)
    direction = 1.0
    if np.any(dx < 0):
        assert np.all(dx <= 0), "x is neither increasing nor decreasing"
        direction = -1.0
    return float(direction * np.sum(dx * (y[1:] + y[:-1]) / 2.0))


def pro_score(masks, amaps, max_step=200, expect_fpr=0.3) -> float:
    """`cal_pro_score`: per threshold the mean over ground-truth regions of (pixels above the threshold) / area, against the
    false-positive rate; the points with fpr < expect_fpr, fpr min-max normalised, trapezoid area."""
    masks = np.asarray(masks) != 0
    amaps = np.asarray(amaps, dtype=np.float32)
    region = np.full(masks.shape, -1, dtype=np.int64)   # region ids counted through the whole set
    n = 0
    for b, m in enumerate(masks):
        lab, _, _ = label8(m)
        roots, inv = np.unique(lab[lab >= 0], return_inverse=True)
        region[b][lab >= 0] = n + inv
        n += len(roots)
    fg = region >= 0
    areas = np.bincount(region[fg], minlength=n).astype(np.float64)
    n_normal = int((~masks).sum())
    min_th, max_th = amaps.min(), amaps.max()
    delta = (max_th - min_th) / max_step
    pros, fprs = [], []
    for th in np.arange(min_th, max_th, delta):
        binary = amaps > th
        tp = np.bincount(region[fg & binary], minlength=n).astype(np.float64)
        pros.append(np.mean(tp / areas))
        fprs.append(np.logical_and(~masks, binary).sum() / n_normal)
    pros, fprs = np.array(pros), np.array(fprs)
    keep = fprs < expect_fpr
    fprs = fprs[keep]
    fprs = (fprs - fprs.min()) / (fprs.max() - fprs.min())
    return sk_auc(fprs, pros[keep])


# ------------------------------------------------------------------------------------------------ the accumulated state
def hist_state(maps, masks):
    """(hist [3, 2^20] int64, counters [4] int64) of maps / masks [B, H, W]: what SegMetrics holds after update(maps, masks)."""
    maps = np.asarray(maps, dtype=np.float32)
    masks = np.asarray(masks) != 0
    hist = np.zeros((3, N_BINS), dtype=np.int64)
    counters = np.zeros(4, dtype=np.int64)
    for amap, m in zip(maps, masks):
        lab, area, n = label8(m)
        finite = np.isfinite(amap)
        key = key_of(amap)
        counters += np.array([m.size, int(m.sum()), n, int((~finite).sum())], dtype=np.int64)
        np.add.at(hist[0], key[finite & ~m], 1)
        np.add.at(hist[1], key[finite & m], 1)
        sel = finite & m
        a = area.ravel()[lab[sel]].astype(np.int64)
        np.add.at(hist[2], key[sel], (1 << 40) // a)
    return hist, counters


# ------------------------------------------------------------------------------------------------ test data
def make_case(B, H, W, seed, exact=False):
    """(masks [B, H, W] uint8, maps [B, H, W] fp32): a few elliptic defects per image (the last image stays good), scores =
    noise, higher on the defects, negative values among them.  exact: scores moved to their bin's value."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.zeros((B, H, W), dtype=np.uint8)
    for b in range(B - 1 if B > 1 else B):
        for _ in range(rng.randint(1, 4)):
            cy, cx = rng.randint(0, H), rng.randint(0, W)
            ry, rx = rng.randint(1, max(2, H // 4)), rng.randint(1, max(2, W // 4))
            masks[b] |= (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0).astype(np.uint8)
    maps = (rng.randn(B, H, W) * 0.35 + 0.1 + 0.5 * masks * rng.rand(B, H, W)).astype(np.float32)
    return masks, (snap(maps) if exact else maps)
