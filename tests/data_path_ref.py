"""Helpers of the data-path edge tests (tests/test_data_path_edges_cpu.py, tests/test_data_path_edges_gpu.py): the image
front-end (csrc/image.hip, K17) and the self-supervised augmentation kernels (csrc/selfsup.hip, K18).

  * `label_ref`            the label lines of `myriad_amd.self_sup.apply_numpy` restated in float64 with scipy's median filters
                           (the label stage is not separately callable on the host); pinned bit for bit to apply_numpy by the CPU
                           module on every golden case.
  * `label_cases`          hand-made (dest, out, union) arrays of section 3: dense / sparse differences, constructed median and
                           vote windows, threshold blocks, a union mask with holes.
  * `emu_label`, `emu_blend`, `emu_front_end`   plain numpy emulations of the kernels' index arithmetic, with named mutants: the
                           CPU module shows that the cases tell every mutant from the kernel.
  * `blend_scenarios`      hand-built PatchOps on [3, 37, 53] noise crops.
  * `poisson_cases`, `poisson_u`   the Poisson cases and their pre-truncation solutions by scipy's DST and by dense sine products.
No test lives here."""
import numpy as np

from myriad_amd import self_sup as P
from oracle import image_ref as IR

MH_OK, MH_ERR_ARG = 0, -1
LOGISTIC_PARAMS = ((1 / 6, 20), (1, 3), (1 / 12, 24))        # patch_ex's default and the two extremes of the MVTec table
LABEL_TOLS = (0, 1, 85)
_DISK = [(dy, dx) for dy in range(-5, 6) for dx in range(-5, 6) if dx * dx + dy * dy <= 25]      # 81 taps, the kernel's order


# ------------------------------------------------------------------------------------------------ label: the reference
def union_ref(shape_hw, ops):
    """The union mask apply_numpy keeps internally: mask[a1:b1, a2:b2] = patch_mask, an assignment, in operation order."""
    m = np.zeros(shape_hw, np.uint8)
    for op in ops:
        y0, x0, h, w = op.dst_box
        m[y0:y0 + h, x0:x0 + w] = op.mask
    return m


def label_ref(dest, out, union, mode, tol, factor, k, x0):
    """apply_numpy's label lines on one image: dest / out [H, W, 3] uint8, union [H, W] uint8 -> float64 [H, W].
    mode 0 binary, 1 continuous, 2 intensity, 3 logistic-intensity."""
    import scipy.ndimage as ndi
    mask = union[..., None]
    diff = np.abs(mask.astype(np.int32) * dest - mask.astype(np.int32) * out).sum(-1, keepdims=True)
    lm = np.uint8(diff > 3 * tol)
    lm[..., 0] = ndi.median_filter(lm[..., 0], size=5, mode="nearest")
    if mode == 0:
        label = lm
    elif mode == 1:
        label = lm * factor
    else:
        y, x = np.mgrid[-5:6, -5:6]
        label = (lm.astype(np.int32) * np.abs(dest.astype(np.int32) - out)).sum(-1, keepdims=True) / 3.0
        label[..., 0] = ndi.median_filter(label[..., 0], footprint=(x * x + y * y <= 25), mode="nearest")
        if mode == 3:
            label = lm / (1 + np.exp(-k * (label - x0)))
    return np.asarray(label, np.float64)[..., 0]


def check_label(got, ref, mode):
    """The derived tolerance of the label kernel: it evaluates the reference's float64 expression and rounds once to float32, so
    modes 0-2 equal np.float32(ref) bit for bit; mode 3 may differ by half a float32 ulp plus a last-bit difference of exp:
    |got - ref| <= 2^-24 |ref| + 2^-50, and exactly 0 where the reference is 0 (lm = 0).  Returns max err / bound."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape
    if mode < 3:
        assert np.array_equal(got.view(np.uint32), np.float32(ref).view(np.uint32)), f"mode {mode}: label differs from float32(ref)"
        return 0.0
    zero = ref == 0                                            # the logistic is never 0 where lm = 1
    assert np.array_equal(got[zero].view(np.uint32), np.zeros(int(zero.sum()), np.uint32)), "mode 3: non-zero label where lm = 0"
    err = np.abs(got.astype(np.float64) - ref)
    bound = 2.0 ** -24 * np.abs(ref) + 2.0 ** -50
    assert not (~(err <= bound)).any(), f"mode 3: err / bound = {np.nanmax(err / bound)}"
    return float((err / bound).max())


# ------------------------------------------------------------------------------------------------ label: window counts
def channel_sums(dest, out):
    return np.abs(dest.astype(np.int32) - out.astype(np.int32)).sum(-1)


def vote_count(dest, out, union, tol, y, x):
    """Pixels over threshold among the 25 taps of the replicated-border 5 x 5 window at (y, x) of one image."""
    over = np.where(union != 0, channel_sums(dest, out), 0) > 3 * tol
    return int(np.pad(over, 2, mode="edge")[y:y + 5, x:x + 5].sum())


def disk_nonzeros(dest, out, union, tol, y, x):
    """Non-zero values among the 81 taps of the replicated-border radius-5 disk at (y, x) of lm * sum_c |dest - out|."""
    lm = label_ref(dest, out, union, 0, tol, 1.0, 0.0, 0.0)
    v = np.pad(lm.astype(np.int64) * channel_sums(dest, out), 5, mode="edge")
    return int(sum(v[y + 5 + dy, x + 5 + dx] != 0 for dy, dx in _DISK))


def _set_sum(out, dest, y, x, s):
    """out[y, x] such that sum_c |dest - out| == s (0 <= s <= 765), spread over the channels, on a dest of 0 / 255 only."""
    for c in range(3):
        d = min(s, 255)
        out[y, x, c] = dest[y, x, c] + d if dest[y, x, c] == 0 else dest[y, x, c] - d
        s -= d


def _median_window(H, W, cy, cx, target, seed, tol=1):
    """An image whose radius-5 disk at (cy, cx) holds exactly `target` non-zero values.  Start: a checkerboard of changed
    (sum > 3 tol, distinct values) and unchanged pixels -- an unchanged pixel has 13 of 25 unchanged neighbours, so lm is 1 on
    the changed colour only -- then unchanged pixels of the window are changed one at a time until the count is reached."""
    r = np.random.RandomState(seed)
    dest = np.zeros((H, W, 3), np.uint8)
    out = dest.copy()
    union = np.ones((H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    vals = r.permutation(H * W).reshape(H, W) % 700 + 3 * tol + 1 + 10
    for parity in (0, 1):                  # the colour that leaves the window short of the target (at a corner the replicated
        out = dest.copy()                  # corner pixel alone counts 26 times)
        for y, x in zip(*np.nonzero((yy + xx) % 2 == (cy + cx + parity) % 2)):
            _set_sum(out, dest, y, x, int(vals[y, x]))
        n = disk_nonzeros(dest, out, union, tol, cy, cx)
        if n <= target:
            break
    for dy, dx in _DISK:
        if n == target:
            break
        y, x = cy + dy, cx + dx
        if not (0 <= y < H and 0 <= x < W) or channel_sums(dest, out)[y, x] != 0:
            continue
        _set_sum(out, dest, y, x, int(vals[y, x]))
        m = disk_nonzeros(dest, out, union, tol, cy, cx)
        if m > target:
            _set_sum(out, dest, y, x, 0)
        else:
            n = m
    assert n == target, (cy, cx, target, n)
    return dest, out, union


def _vote_window(H, W, pix, seed):
    """Only the pixels `pix` are changed (sum well over every threshold used): the 5 x 5 count at the window centre is what
    the caller arranges."""
    r = np.random.RandomState(seed)
    dest = r.randint(0, 2, (H, W, 3)).astype(np.uint8) * 255
    out = dest.copy()
    for y, x in pix:
        _set_sum(out, dest, y, x, 300 + int(r.randint(0, 400)))
    return dest, out, np.ones((H, W), np.uint8)


# the constructed windows: (kind, count, (cy, cx) as a function of (H, W)); the corner is (0, 0) or the bottom-right pixel
def _vote_pixels(H, W, where, count):
    if where == "interior":
        cy, cx = H // 2, W // 2
        cells = [(cy + dy, cx + dx) for dy in range(-2, 3) for dx in range(-2, 3)]
        return (cy, cx), cells[:count]
    if where == "corner00":        # replicated taps: (0,0) counts 9 times, (0,1) (0,2) (1,0) (2,0) 3 times, the other four once
        return (0, 0), ([(0, 0), (0, 1)] if count == 12 else [(0, 0), (1, 1), (1, 2), (2, 1), (2, 2)])
    cy, cx = H - 1, W - 1          # the mirror image at the bottom-right corner
    return (cy, cx), ([(cy, cx), (cy - 1, cx)] if count == 12 else [(cy, cx), (cy - 1, cx - 1), (cy - 1, cx - 2), (cy - 2, cx - 1), (cy - 2, cx - 2)])


CONSTRUCTED = []          # (case name, image index, (cy, cx), kind, expected count, tol) -- asserted by the CPU module


def _stack(images):
    return tuple(np.stack([im[i] for im in images]) for i in range(3))


def label_cases():
    """[(name, dest [B,H,W,3] u8, out, union [B,H,W] u8)] of section 3.  Deterministic; built once per process."""
    if _CACHE.get("label") is not None:
        return _CACHE["label"]
    del CONSTRUCTED[:]
    cases = []
    for si, (B, H, W) in enumerate([(2, 37, 53), (1, 53, 37), (1, 3, 53), (1, 53, 4), (1, 1, 1)]):
        tag = f"{B}x{H}x{W}"
        r = np.random.RandomState(100 + si)
        dest = r.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
        full = np.ones((B, H, W), np.uint8)
        # dense noise differences under a full union mask: > 40 non-zeros per window, the selection sort
        cases.append((f"dense_wide_{tag}", dest, r.randint(0, 256, (B, H, W, 3)).astype(np.uint8), full))
        # small differences: channel sums 0..6, many ties, sums of exactly 3 tol and 3 tol + 1 for tol 0 and 1
        small = np.clip(dest.astype(np.int32) + r.randint(-2, 3, dest.shape) * (r.rand(*dest.shape) < 0.8), 0, 255).astype(np.uint8)
        cases.append((f"dense_ties_{tag}", dest, small, full))
        # sparse: a few changed blocks and isolated pixels, most windows hold <= 40 non-zeros
        out = dest.copy()
        for _ in range(3):
            y0, x0 = r.randint(0, max(H - 5, 1)), r.randint(0, max(W - 5, 1))
            out[:, y0:y0 + 6, x0:x0 + 7] = r.randint(0, 256, out[:, y0:y0 + 6, x0:x0 + 7].shape)
        iso = r.rand(B, H, W) < 0.03
        out[iso] = 255 - out[iso]
        cases.append((f"sparse_{tag}", dest, out, full))
        # a union mask with holes: out != dest inside the holes, which lie inside the blurred mask (the unmasked sum is what the
        # intensity needs there) and in a block the union leaves out altogether (the masked sum is what the vote needs there)
        out = r.randint(0, 256, dest.shape).astype(np.uint8)
        out[out == dest] ^= 1
        union = np.zeros((B, H, W), np.uint8)
        union[:, : max(H * 2 // 3, 1), : max(W * 2 // 3, 1)] = 1
        union[:, 3::5, 2::4] = 0
        union[:, 4::5, 2::4] = 0
        c0 = max(W * 2 // 3, 1)
        out[:, : H // 2, c0:] = dest[:, : H // 2, c0:]                                                  # top right: unchanged
        cases.append((f"union_holes_{tag}", dest, out, union))
    for (H, W) in ((37, 53), (53, 37)):
        tag = f"{H}x{W}"
        # thresholds: 7 x 7 blocks whose channel sums are exactly 3 tol and 3 tol + 1 for tol = 0, 1, 85
        dest = np.random.RandomState(7).randint(0, 2, (H, W, 3)).astype(np.uint8) * 255
        out = dest.copy()
        sums = [0, 1, 3, 4, 255, 256]
        per_row = 3 if W > H else 2
        for n, s in enumerate(sums):
            y0, x0 = 2 + 11 * (n // per_row), 2 + 17 * (n % per_row)      # gaps of >= 4: no vote bridges two blocks
            for y in range(y0, y0 + 7):
                for x in range(x0, x0 + 7):
                    _set_sum(out, dest, y, x, s)
        cases.append((f"thresholds_{tag}", dest[None], out[None], np.ones((1, H, W), np.uint8)))
        # constructed windows, interior and corner, each its own image so that no window disturbs another
        for kind, counts in (("median", (40, 41)), ("vote", (12, 13))):
            imgs, recs = [], []
            for count in counts:
                for where in ("interior", "corner00", "cornerBR"):
                    if kind == "median":
                        cy, cx = {"interior": (H // 2, W // 2), "corner00": (0, 0), "cornerBR": (H - 1, W - 1)}[where]
                        imgs.append(_median_window(H, W, cy, cx, count, seed=count))
                    else:
                        (cy, cx), pix = _vote_pixels(H, W, where, count)
                        imgs.append(_vote_window(H, W, pix, seed=count))
                    recs.append((len(imgs) - 1, (cy, cx), kind, count, 1))
            name = f"{kind}_windows_{tag}"
            cases.append((name,) + _stack(imgs))
            CONSTRUCTED.extend((name,) + rec for rec in recs)
    _CACHE["label"] = cases
    return cases


_CACHE = {}


def label_refs(name, dest, out, union, mode, tol, k=0.0, x0=0.0):
    """label_ref per image of a case, cached (the CPU and the GPU module, and every mutant, share one reference)."""
    key = (name, mode, tol, k, x0)
    if key not in _CACHE:
        B = dest.shape[0]
        _CACHE[key] = np.stack([label_ref(dest[b], out[b], union[b], mode, tol, label_factor(b), k, x0) for b in range(B)])
    return _CACHE[key]


def label_factor(b):
    return (0.3, 0.95, 0.05, 0.5, 0.7, 0.61)[b % 6]


def label_runs():
    """(mode, tol, k, x0) of every call made on every label case: modes 0-3 at tol 0, 1, 85; mode 3 with three parameter pairs."""
    runs = [(m, t, 0.0, 0.0) for m in (0, 1, 2) for t in LABEL_TOLS]
    runs += [(3, t, k, x0) for t in LABEL_TOLS for (k, x0) in LOGISTIC_PARAMS]
    return runs


# ------------------------------------------------------------------------------------------------ label: the emulation
LABEL_MUTANTS = ["hw_swap", "clamp_h2", "majority_gt13", "threshold_ge", "median_pos39", "median_pos41", "nz_gt41",
                 "value_masked", "vote_unmasked"]


def emu_label(dest, out, union, mode, tol, factor, k, x0, mutant=None):
    """csrc/selfsup.hip label_sum / label_mask / label_value in numpy over the flat pixel index, [B, H, W] at once."""
    B, H, W = union.shape
    s = channel_sums(dest, out).reshape(-1)
    lo, hi = np.where(union.reshape(-1) != 0, s, 0), s                       # the two halves of `sums`
    Hi, Wi = (W, H) if mutant == "hw_swap" else (H, W)
    i = np.arange(B * H * W)
    x, y, base = i % Wi, (i // Wi) % Hi, (i // (Wi * Hi)) * (Wi * Hi)
    ymax = max(Hi - 2, 0) if mutant == "clamp_h2" else Hi - 1

    def tap(a, dy, dx):
        return a[base + np.clip(y + dy, 0, ymax) * Wi + np.clip(x + dx, 0, Wi - 1)]

    vs = hi if mutant == "vote_unmasked" else lo
    tol3 = 3 * tol
    cnt = sum(((tap(vs, dy, dx) >= tol3) if mutant == "threshold_ge" else (tap(vs, dy, dx) > tol3)).astype(np.int32)
              for dy in range(-2, 3) for dx in range(-2, 3))
    lm = ((cnt > 13) if mutant == "majority_gt13" else (cnt >= 13)).astype(np.int64)
    if mode == 0:
        return lm.astype(np.float32).reshape(B, H, W)
    if mode == 1:
        f = np.repeat(np.asarray(factor, np.float64), H * W)
        return (lm.astype(np.float64) * f).astype(np.float32).reshape(B, H, W)
    val = (lo if mutant == "value_masked" else hi) * lm
    v = np.sort(np.stack([tap(val, dy, dx) for dy, dx in _DISK]), axis=0)
    nz = (v != 0).sum(0)
    pos = {"median_pos39": 39, "median_pos41": 41}.get(mutant, 40)
    med = np.where(nz > (41 if mutant == "nz_gt41" else 40), v[pos], 0).astype(np.float64) / 3.0
    if mode == 2:
        return med.astype(np.float32).reshape(B, H, W)
    return (lm.astype(np.float64) / (1.0 + np.exp(-k * (med - x0)))).astype(np.float32).reshape(B, H, W)


def label_case_passes(case, mutant=None):
    """True when the emulation meets every run of one case (the check the GPU module applies to the kernel)."""
    name, dest, out, union = case
    B = dest.shape[0]
    f = [label_factor(b) for b in range(B)]
    try:
        for mode, tol, k, x0 in label_runs():
            got = emu_label(dest, out, union, mode, tol, f, k, x0, mutant)
            check_label(got, label_refs(name, dest, out, union, mode, tol, k, x0), mode)
    except AssertionError:
        return False
    return True


# ------------------------------------------------------------------------------------------------ blend
BLEND_SHAPE = (3, 37, 53)


def _mask(r, h, w, kind):
    if kind == "full":
        return np.ones((h, w), np.uint8)
    return (r.rand(h, w) < 0.7).astype(np.uint8)                             # holes


def integer_pairs(f=0.3):
    """(x, s) byte pairs for the 'uniform' blend at factor f, mask 1: `exact` -- x - f x + f s is an integer in exact decimal
    arithmetic and the float64 evaluation in the reference's order lands on it; `under` -- it lands just under it (the floor
    is one less than the exact value's)."""
    assert f == 0.3
    x, s = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    exact10 = 10 * x - 3 * x + 3 * s                                         # ten times the exact value for f = 3 / 10
    v = x.astype(np.float64)
    v = v - (f * 1) * x
    v = v + (f * 1) * s
    integer = exact10 % 10 == 0
    exact = integer & (v == exact10 // 10)
    under = integer & (np.floor(v) == exact10 // 10 - 1)
    return np.argwhere(exact), np.argwhere(under)


def blend_scenarios():
    """[(name, dest [3,37,53,3], src, plans)] with plans[b] = (ops, factor): hand-built PatchOps on images 0 and 2, none on 1."""
    if _CACHE.get("blend") is not None:
        return _CACHE["blend"]
    B, H, W = BLEND_SHAPE
    r = np.random.RandomState(2024)
    dest = r.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    src = r.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    out = []

    def op(mode, dst, sy=None, sx=None, kind="holes", f=1.0, src_size=None):
        y0, x0, h, w = dst
        sh, sw = src_size if src_size is not None else (h, w)
        sy = int(r.randint(0, H - sh + 1)) if sy is None else sy
        sx = int(r.randint(0, W - sw + 1)) if sx is None else sx
        return P.PatchOp((sy, sx), dst, _mask(r, h, w, kind), f, mode, src_size=src_size)

    borders = [(0, 10, 5, 7), (32, 10, 5, 7), (10, 0, 6, 4), (10, 49, 6, 4)]
    corners = [(0, 0, 4, 5), (0, 48, 4, 5), (33, 0, 4, 5), (33, 48, 4, 5)]
    out.append(("borders", dest, src, [([op("swap", b) for b in borders], 1.0), ([], 1.0),
                                       ([op("uniform", b, f=0.3) for b in borders], 0.3)]))
    out.append(("corners", dest, src, [([op("uniform", c, f=0.3) for c in corners], 0.3), ([], 1.0),
                                       ([op("swap", c) for c in corners], 1.0)]))
    thin = [(5, 6, 1, 1), (0, 0, 1, 1), (36, 52, 1, 1), (7, 3, 1, 40), (36, 0, 1, 53), (2, 20, 30, 1), (0, 52, 37, 1)]
    out.append(("thin", dest, src, [([op("swap", t, kind="full") for t in thin], 1.0), ([], 1.0),
                                    ([op("uniform", t, kind="full", f=0.3) for t in thin], 0.3)]))
    whole = (0, 0, H, W)
    out.append(("whole_image", dest, src, [([op("swap", whole, 0, 0)], 1.0), ([], 1.0), ([op("uniform", whole, 0, 0, f=0.3)], 0.3)]))
    a, b2 = (8, 12, 15, 20), (14, 22, 16, 21)                                  # two overlapping boxes, both orders
    out.append(("overlap", dest, src, [([op("swap", a), op("uniform", b2, f=0.3)], 0.3), ([], 1.0),
                                       ([op("uniform", a, f=0.3), op("swap", b2)], 0.3)]))
    out.append(("factors_0_1", dest, src, [([op("uniform", a, f=0.0), op("uniform", (30, 40, 7, 13), f=0.0)], 0.0), ([], 1.0),
                                           ([op("uniform", b2, f=1.0), op("uniform", (0, 0, 9, 9), f=1.0)], 1.0)]))
    # pooled source (mode & 4: the patch is resampled) next to a direct one; up-scaled, down-scaled and the 2 x 2 area path
    pooled0 = [op("swap", (3, 5, 20, 30), src_size=(11, 17)), op("swap", (25, 30, 5, 6), src_size=(10, 12)), op("swap", (31, 38, 6, 12)), op("uniform", (12, 30, 9, 14), f=0.3, src_size=(18, 28))]
    pooled2 = [op("uniform", (0, 0, 37, 53), f=0.3, src_size=(5, 9)), op("swap", (30, 2, 7, 50), src_size=(20, 11)), op("uniform", (4, 4, 5, 5), f=0.3)]
    out.append(("pooled", dest, src, [(pooled0, 0.3), ([], 1.0), (pooled2, 0.3)]))
    # f = 0.3 on byte pairs whose blend is an integer: landing on it and just under it (image 0), noise on image 2
    exact, under = integer_pairs(0.3)
    pairs = np.resize(np.concatenate([under, exact]), (H * W * 3, 2))
    d2, s2 = dest.copy(), src.copy()
    d2[0] = pairs[:, 0].astype(np.uint8).reshape(H, W, 3)
    s2[0] = pairs[:, 1].astype(np.uint8).reshape(H, W, 3)
    out.append(("integer_landing", d2, s2, [([op("uniform", whole, 0, 0, kind="full", f=0.3)], 0.3), ([], 1.0),
                                            ([op("uniform", whole, 0, 0, f=0.3)], 0.3)]))
    _CACHE["blend"] = out
    return out


def emu_blend(dest, src, plans, mutant=None):
    """patch_blend_kernel's index arithmetic on flat arrays, operations in order -> (out [B,H,W,3], union [B,H,W])."""
    B, H, W, _ = dest.shape
    Hi, Wi = (W, H) if mutant == "hw_swap" else (H, W)
    o = dest.reshape(-1, 3).copy()
    sflat = src.reshape(-1, 3)
    union = np.zeros(B * H * W, np.uint8)
    for b, (ops, _f) in enumerate(plans):
        for op in ops:
            (sy, sx), (y0, x0, h, w) = op.src_box, op.dst_box
            py, px = np.mgrid[0:h, 0:w]
            d = ((b * Hi + y0 + py) * Wi + x0 + px).reshape(-1)
            if op.resized:
                sv = P.resize_linear_u8(src[b, sy:sy + op.src_size[0], sx:sx + op.src_size[1]], (w, h)).reshape(-1, 3)
            else:
                sv = sflat[((b * Hi + sy + py) * Wi + sx + px).reshape(-1)]
            m = op.mask.reshape(-1)
            union[d] = m
            xv = o[d]
            if op.mode == "swap":
                o[d] = np.where(m[:, None] != 0, sv, xv)
            else:
                fm = (op.factor * m.astype(np.float64))[:, None]
                v = xv.astype(np.float64)
                v = v - fm * xv
                v = v + fm * sv
                o[d] = np.floor(v).astype(np.uint8)
    return o.reshape(dest.shape), union.reshape(B, H, W)


def blend_ref(dest, src, plans):
    """apply_numpy per image -> (out, union, binary label)."""
    outs, unions = [], []
    for b, (ops, f) in enumerate(plans):
        o, _, _ = P.apply_numpy(dest[b], src[b], ops, f, "binary")
        outs.append(o)
        unions.append(union_ref(dest.shape[1:3], ops))
    return np.stack(outs), np.stack(unions)


# ------------------------------------------------------------------------------------------------ front-end
FRONT_SIZE = 16
FRONT_SIZES = [(16, 16), (5, 7), (1, 1), (17, 16), (16, 17), (33, 16), (35, 16), (64, 1000), (1000, 3)]


def noise_image(H, W, seed=0):
    return np.random.RandomState(H * 1009 + W + seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


def front_ref(img, size, mode):
    return (IR.train_image if mode == "train" else IR.eval_image)(img, size)


def emu_front_end(img, size, mode, rounding="half_even"):
    """csrc/image.hip's two passes with the plan of image_frontend._plan: pass 1 only for the crop's columns and the rows its
    output rows tap, pass 2 for the crop window -> uint8 [size, size, 3].  `rounding`: how the crop offset (rh - size) / 2 is
    made an integer -- 'half_even' (torchvision's round), or the mutants 'floor' / 'ceil'."""
    import math
    from myriad_amd import image_frontend as F
    H, W, _ = img.shape
    S = size
    rnd = {"half_even": lambda v: int(round(v)), "floor": math.floor, "ceil": math.ceil}[rounding]
    if mode == "train":
        rh, rw = F.resized_size(H, W, S)
        top, left = rnd((rh - S) / 2.0), rnd((rw - S) / 2.0)
    else:
        rh, rw, top, left = S, S, 0, 0
    kh, bh = F.resample_tables(W, rw)
    kv, bv = F.resample_tables(H, rh)
    y0 = int(bv[top, 0])
    rows = int(bv[top + S - 1, 0] + bv[top + S - 1, 1]) - y0
    half = 1 << (F.PRECISION_BITS - 1)
    q = img.astype(np.int64)
    tmp = np.empty((rows, S, 3), np.int64)
    for x in range(S):
        first, n = bh[left + x]
        tmp[:, x] = np.clip((half + np.tensordot(q[y0:y0 + rows, first:first + n], kh[left + x, :n].astype(np.int64), axes=(1, 0))) >> F.PRECISION_BITS, 0, 255)
    out = np.empty((S, S, 3), np.uint8)
    for y in range(S):
        first, n = bv[top + y]
        out[y] = np.clip((half + np.tensordot(kv[top + y, :n].astype(np.int64), tmp[first - y0:first - y0 + n], axes=(0, 0))) >> F.PRECISION_BITS, 0, 255)
    return out


# ------------------------------------------------------------------------------------------------ Poisson clone
POISSON_SHAPE = (2, 41, 59)


def _ellipse_with_hole(h, w):
    y, x = np.mgrid[0:h, 0:w]
    ry, rx = (h - 1) / 2.0, (w - 1) / 2.0
    e = ((y - ry) / (ry + 0.25)) ** 2 + ((x - rx) / (rx + 0.25)) ** 2
    return (((e <= 1.0) & (e > 0.08)) * 255).astype(np.uint8)


def poisson_cases():
    """[(name, dest [2,41,59,3] u8, image, steps)], steps = [(patch [hp,wp,3], pms [hp,wp], roi, mixed)] applied in sequence.
    roi = (y0s, x0s, dy0, dx0, h, w) as clone_roi returns it."""
    if _CACHE.get("poisson") is not None:
        return _CACHE["poisson"]
    B, H, W = POISSON_SHAPE
    # name, image, [(patch (hp, wp), roi-in-patch (y0s, x0s, h, w), destination (dy0, dx0), mask)]
    spec = [("3x3", 0, [((3, 3), (0, 0, 3, 3), (19, 30), "full")]),
            ("3x38_top_left", 1, [((3, 38), (0, 0, 3, 38), (0, 0), "full")]),
            ("23x5_bottom_right", 1, [((23, 5), (0, 0, 23, 5), (H - 23, W - 5), "full")]),
            ("18x34", 0, [((18, 34), (0, 0, 18, 34), (5, 7), "full")]),
            ("19x35_bottom_right", 1, [((19, 35), (0, 0, 19, 35), (H - 19, W - 35), "full")]),
            ("41x59_whole", 0, [((41, 59), (0, 0, 41, 59), (0, 0), "full")]),
            ("ellipse_hole", 1, [((21, 31), (0, 0, 21, 31), (3, 4), "ellipse")]),
            ("box_inside_patch", 0, [((30, 40), (4, 6, 20, 27), (10, 20), "full")]),
            ("two_overlapping", 1, [((18, 34), (0, 0, 18, 34), (2, 3), "full"), ((19, 35), (0, 0, 19, 35), (10, 15), "ellipse")])]
    cases = []
    for ci, (name, image, steps) in enumerate(spec):
        for mixed in (False, True):
            r = np.random.RandomState(POISSON_SEEDS.get((name, mixed), 500 + 2 * ci + int(mixed)))
            dest = r.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
            built = []
            for (hp, wp), (y0s, x0s, h, w), (dy0, dx0), kind in steps:
                patch = r.randint(0, 256, (hp, wp, 3)).astype(np.uint8)
                pms = np.zeros((hp, wp), np.uint8)
                pms[y0s:y0s + h, x0s:x0s + w] = _ellipse_with_hole(h, w) if kind == "ellipse" else 255
                ys, xs = np.nonzero(pms)                                      # the ROI is the mask's bounding box
                assert (ys.min(), ys.max() + 1, xs.min(), xs.max() + 1) == (y0s, y0s + h, x0s, x0s + w)
                built.append((patch, pms, (y0s, x0s, dy0, dx0, h, w), mixed))
            cases.append((name + ("_mixed" if mixed else "_normal"), dest, image, built))
    _CACHE["poisson"] = cases
    return cases


POISSON_SEEDS = {}        # (case, mixed) -> seed, for a case whose default seed put a solution within 1e-9 of an integer


def poisson_u(out, patch, pms, roi, mixed):
    """The pre-truncation solution of poisson_clone_numpy (its lines, restated) computed two ways: scipy's DST-I, and the
    dense sine products of `dst_tables` in the device's order.  -> (u_fft, u_dense), each [h-2, w-2, 3] float64."""
    import scipy.fft as sfft
    y0, x0, dy0, dx0, h, w = roi
    D = out[dy0:dy0 + h, dx0:dx0 + w].astype(np.float64)
    Pm = np.where(pms[y0:y0 + h, x0:x0 + w, None] != 0, patch[y0:y0 + h, x0:x0 + w], 0).astype(np.float64)
    me = P.eroded_mask(pms, roi).astype(np.float64)[..., None]
    mf, mi = me / 255.0, (255.0 - me) / 255.0
    dgx, pgx = D[:, 1:] - D[:, :-1], Pm[:, 1:] - Pm[:, :-1]
    dgy, pgy = D[1:] - D[:-1], Pm[1:] - Pm[:-1]
    if mixed:
        keep = np.abs(pgx[:-1] - pgy[:, :-1]) > np.abs(dgx[:-1] - dgy[:, :-1])
        pgx, pgy = pgx.copy(), pgy.copy()
        pgx[:-1] = np.where(keep, pgx[:-1], dgx[:-1])
        pgy[:, :-1] = np.where(keep, pgy[:, :-1], dgy[:, :-1])
    gx = dgx * mi[:, :-1] + pgx * mf[:, :-1]
    gy = dgy * mi[:-1] + pgy * mf[:-1]
    lap = (gx[1:-1, 1:] - gx[1:-1, :-1]) + (gy[1:, 1:-1] - gy[:-1, 1:-1])
    ring = D.copy()
    ring[1:-1, 1:-1] = 0
    rhs = lap - (ring[1:-1, :-2] + ring[1:-1, 2:] + ring[:-2, 1:-1] + ring[2:, 1:-1])
    nh, nw = h - 2, w - 2
    Sh, cy = P.dst_tables(nh)
    Sw, cx = P.dst_tables(nw)
    den = cy[:, None, None] + cx[None, :, None] - 4.0
    u_fft = sfft.idstn(sfft.dstn(rhs, type=1, axes=(0, 1)) / den, type=1, axes=(0, 1))
    u_dense = np.empty_like(rhs)
    for c in range(3):              # t = Sh r;  r = (t Sw) / den;  t = Sh r;  u = (t Sw) 4 / ((nh + 1)(nw + 1))
        t = Sh @ rhs[..., c]
        q = (t @ Sw) / den[..., 0]
        t = Sh @ q
        u_dense[..., c] = (t @ Sw) * (4.0 / ((nh + 1.0) * (nw + 1.0)))
    return u_fft, u_dense


def truncate(u):
    return np.floor(np.clip(u, 0.0, 255.0) + P.TRUNC_EPS).astype(np.uint8)


def poisson_apply_ref(dest, image, steps):
    """poisson_clone_numpy over the steps of one case -> the [2,41,59,3] result (only `image` changes)."""
    out = dest.copy()
    for patch, pms, roi, mixed in steps:
        P.poisson_clone_numpy(out[image], patch, pms, roi, mixed=mixed)
    return out
