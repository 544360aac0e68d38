"""The image front-end (csrc/image.hip, K17) and the self-supervised augmentation kernels (csrc/selfsup.hip, K18) per pixel at
their edges, on crops of a few thousand pixels, into poisoned buffers, with their refusal paths.

References: oracle/image_ref.py (pinned to Pillow) for the front-end; `apply_numpy`, `resize_linear_u8`, `poisson_clone_numpy`
(pinned to the oracle and the reference's goldens) for blend, resize and clone; `label_ref` of tests/data_path_ref.py for the
label stage (pinned bit for bit to apply_numpy by tests/test_data_path_edges_cpu.py, which also shows that the cases tell the
kernels from their named mutants).

Tolerances, derived: everything uint8 and the front-end's float32 are bit-exact.  The label kernel evaluates the reference's
float64 expression and rounds once to float32: modes 0-2 equal float32(ref) bit for bit; mode 3 (one exp) is held to
|got - ref| <= 2^-24 |ref| + 2^-50 and is exactly 0 where lm = 0.  Largest mode-3 err / bound seen on the MI355X: 0.8896
(dense_ties, every shape; all label cases, tol 0 / 1 / 85, three logistic parameter pairs) -- the float32 rounding itself.

Found by these cases and fixed with them: the 'uniform' blend's two products were fused into the adds that follow them (the
build contracts floating point), one rounding where numpy has two; at factor 0.3 that lands x - 0.3 x + 0.3 s on an integer
where the reference lands just under it, a whole grey level after floor().  `thin` (one byte of 5883) and `integer_landing`
(74 bytes) are its regression cases; the smooth golden images never reached it.

Poisson: bit equality on every pixel.  The device solves with dense sine products, the host with scipy's DST, and both
truncate floor(clip(u) + 1e-6); the CPU module asserts for every case here that the two solutions agree to 1e-10, that no
unclipped pixel is within 1e-9 of an integer, and that both truncate alike.  CPU-measured per case (NORMAL / MIXED):

    case                  dense vs FFT          nearest integer
    3x3                   0 / 0                 2.5e-01 / 1.0e-06 (an exact-integer solution sits at the 1e-6 offset)
    3x38_top_left         7.1e-13 / 8.2e-13     4.5e-03 / 3.2e-04
    23x5_bottom_right     5.9e-13 / 5.0e-13     1.2e-03 / 3.5e-03
    18x34                 1.1e-12 / 1.1e-12     6.8e-04 / 7.5e-04
    19x35_bottom_right    1.1e-12 / 9.2e-13     1.5e-05 / 5.8e-04
    41x59_whole           3.5e-12 / 2.4e-12     1.5e-05 / 5.1e-05
    ellipse_hole          1.5e-12 / 1.3e-12     2.3e-04 / 1.0e-04
    box_inside_patch      1.3e-12 / 9.1e-13     2.1e-05 / 7.4e-05
    two_overlapping       1.2e-12 / 1.2e-12     1.1e-04 / 5.1e-04
"""
import numpy as np
import pytest
import torch

from myriad_amd import self_sup as P
from tests import data_path_ref as R

pytestmark = pytest.mark.gpu

OK, ERR = R.MH_OK, R.MH_ERR_ARG
S = R.FRONT_SIZE
NAN_BITS = 0x7FC0BEEF                # a quiet NaN with a payload
BYTE = 0xA5


def _lib():
    from myriad_amd import _lib as L, ops as Ops
    return L.load(), Ops._s()


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_buf(*shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def is_poison(t):
    torch.cuda.synchronize()
    if t.dtype == torch.uint8:
        return bool((t == BYTE).all())
    if t.dtype == torch.float64:
        return bool(torch.isnan(t).all())
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def byte_buf(*shape):
    return torch.full(shape, BYTE, dtype=torch.uint8, device="cuda")


# ================================================================================================ 1. front-end
def _front_end(size, mode):
    from myriad_amd.image_frontend import ImageFrontEndHIP
    fe = ImageFrontEndHIP("cuda", size=size, mode=mode)
    fe._tmp = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")          # large enough for every size below: never reallocated
    return fe


def _run_one(fe, img_dev, size):
    """_one into the middle slab of poisoned [3, ...] buffers; the neighbours must stay untouched."""
    buf, ubuf = nan_buf(3, 3, size, size), byte_buf(3, size, size, 3)
    fe._one(img_dev, buf[1], ubuf[1])
    assert is_poison(buf[0]) and is_poison(buf[2]) and is_poison(ubuf[0]) and is_poison(ubuf[2])
    return ubuf[1].cpu().numpy(), buf[1].cpu().numpy()


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("H,W,size", [(h, w, S) for h, w in R.FRONT_SIZES] + [(100, 150, 224)])
def test_front_end_sizes_scratch_and_strides(H, W, size, mode):
    img = R.noise_image(H, W)
    ref_u8, ref_f = R.front_ref(img, size, mode)
    fe = _front_end(size, mode)
    tmp_ptr = fe._tmp.data_ptr()
    results = []
    for fill in (0x00, 0xFF):                       # a byte poison can equal a legitimate value: both fills give the same output
        fe._tmp.fill_(fill)
        results.append(_run_one(fe, cu(img), size))
        assert fe._tmp.data_ptr() == tmp_ptr
    for u8, f in results:
        assert np.array_equal(u8, ref_u8), (H, W, mode)
        assert np.array_equal(f.view(np.uint32), ref_f.view(np.uint32)), (H, W, mode)
    # a view of a wider poisoned image: stride(0) > 3 W goes to the kernel as row_stride
    big = byte_buf(H, W + 11, 3)
    big[:, 5:5 + W] = cu(img)
    view = big[:, 5:5 + W]
    assert view.stride(0) > 3 * W and view.stride(1) == 3
    u8, f = _run_one(fe, view, size)
    assert np.array_equal(u8, ref_u8) and np.array_equal(f.view(np.uint32), ref_f.view(np.uint32))
    # stride(1) != 3: the .contiguous() branch
    wide = byte_buf(H, 2 * W, 3)
    wide[:, ::2] = cu(img)
    view = wide[:, ::2]
    assert view.stride(1) != 3
    u8, f = _run_one(fe, view, size)
    assert np.array_equal(u8, ref_u8) and np.array_equal(f.view(np.uint32), ref_f.view(np.uint32))


def _direct_args(fe, img_dev, H, W, out, u8):
    kh, bh, ksh, kv, bv, ksv, top, left, y0, rows = fe._plan(H, W)
    return dict(img=img_dev.data_ptr(), H=H, W=W, row_stride=3 * W, kh=kh.data_ptr(), bh=bh.data_ptr(), ksz_h=ksh, kv=kv.data_ptr(),
                bv=bv.data_ptr(), ksz_v=ksv, crop_y0=top, crop_x0=left, out_h=fe.size, out_w=fe.size, y0=y0, rows=rows,
                tmp=fe._tmp.data_ptr(), lut=fe.lut.data_ptr(), out=None if out is None else out.data_ptr(),
                u8_out=None if u8 is None else u8.data_ptr())


def _resize_call(a):
    lib, s = _lib()
    return lib.mh_image_resize_crop_norm(a["img"], a["H"], a["W"], a["row_stride"], a["kh"], a["bh"], a["ksz_h"], a["kv"], a["bv"],
                                         a["ksz_v"], a["crop_y0"], a["crop_x0"], a["out_h"], a["out_w"], a["y0"], a["rows"], a["tmp"],
                                         a["lut"], a["out"], a["u8_out"], s)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_front_end_single_output_calls(mode):
    H, W = 35, 16
    img = R.noise_image(H, W)
    ref_u8, ref_f = R.front_ref(img, S, mode)
    fe = _front_end(S, mode)
    d = cu(img)
    out, u8 = nan_buf(3, 3, S, S), byte_buf(3, S, S, 3)
    assert _resize_call(_direct_args(fe, d, H, W, out[1], u8[1])) == OK
    both_f, both_u = out[1].cpu().numpy(), u8[1].cpu().numpy()
    assert np.array_equal(both_u, ref_u8) and np.array_equal(both_f.view(np.uint32), ref_f.view(np.uint32))
    u8b = byte_buf(3, S, S, 3)
    a = _direct_args(fe, d, H, W, None, u8b[1])
    a["lut"] = None                                                             # u8-only needs no table
    assert _resize_call(a) == OK
    assert np.array_equal(u8b[1].cpu().numpy(), both_u) and is_poison(u8b[0]) and is_poison(u8b[2])
    outb = nan_buf(3, 3, S, S)
    assert _resize_call(_direct_args(fe, d, H, W, outb[1], None)) == OK
    assert np.array_equal(outb[1].cpu().numpy().view(np.uint32), both_f.view(np.uint32)) and is_poison(outb[0]) and is_poison(outb[2])


def test_front_end_refusals_leave_the_outputs_untouched():
    H, W = 33, 16
    fe = _front_end(S, "train")
    d = cu(R.noise_image(H, W))
    out, u8 = nan_buf(3, S, S), byte_buf(S, S, 3)
    good = _direct_args(fe, d, H, W, out, u8)
    bad = [dict(img=None), dict(kh=None), dict(bh=None), dict(kv=None), dict(bv=None), dict(tmp=None), dict(out=None, u8_out=None),
           dict(lut=None), dict(H=0), dict(W=0), dict(H=-1), dict(out_h=0), dict(out_w=0), dict(out_h=-3), dict(crop_y0=-1),
           dict(crop_x0=-1), dict(ksz_h=0), dict(ksz_v=0), dict(y0=-1), dict(rows=0), dict(rows=-2),
           dict(y0=good["y0"] + 1, rows=H - good["y0"]),                        # y0 + rows = H + 1
           dict(y0=H, rows=1), dict(row_stride=3 * W - 1), dict(row_stride=0), dict(row_stride=-3 * W)]
    for change in bad:
        assert _resize_call(dict(good, **change)) == ERR, change
    assert is_poison(out) and is_poison(u8)
    assert _resize_call(dict(good, rows=H - good["y0"])) == OK                  # y0 + rows = H itself is legal (more rows than tapped)
    assert np.array_equal(u8.cpu().numpy(), R.front_ref(R.noise_image(H, W), S, "train")[0])
    lib, s = _lib()
    o2, src = nan_buf(3 * 7 + 5), byte_buf(7, 3)
    for args in ((None, 7, fe.lut.data_ptr(), o2.data_ptr()), (src.data_ptr(), 7, None, o2.data_ptr()), (src.data_ptr(), 7, fe.lut.data_ptr(), None)):
        assert lib.mh_image_u8_normalize(*args, s) == ERR
    for n in (0, -5):                                                          # nothing to do: OK, nothing written
        assert lib.mh_image_u8_normalize(src.data_ptr(), n, fe.lut.data_ptr(), o2.data_ptr(), s) == OK
    assert is_poison(o2)


@pytest.mark.parametrize("n_pix", [1, 255, 256, 257, 65536 * 256 + 3])
def test_u8_normalize_every_value_every_channel(n_pix):
    """n_pix at, below and above one block, and past the 65536-block grid cap (the grid-stride loop's second sweep)."""
    lib, s = _lib()
    lut = cu(R.IR.normalize_lut())
    i = torch.arange(n_pix, dtype=torch.int64, device="cuda")
    u8 = torch.stack([((i * 7 + 91 * c) % 256).to(torch.uint8) for c in range(3)], 1).contiguous()          # [n_pix, 3]
    del i
    if n_pix >= 256:
        assert all(int(torch.unique(u8[:, c]).numel()) == 256 for c in range(3))
    guard = 64
    out = nan_buf(3 * n_pix + guard)
    assert lib.mh_image_u8_normalize(u8.data_ptr(), n_pix, lut.data_ptr(), out.data_ptr(), s) == OK
    torch.cuda.synchronize()
    for c in range(3):
        want = lut[c][u8[:, c].long()]
        assert torch.equal(out[c * n_pix:(c + 1) * n_pix].view(torch.int32), want.view(torch.int32)), c
        del want
    assert is_poison(out[3 * n_pix:])


# ================================================================================================ 2. blend
@pytest.mark.parametrize("sc", R.blend_scenarios(), ids=[s[0] for s in R.blend_scenarios()])
def test_blend_matches_apply_numpy(sc):
    name, dest, src, plans = sc
    want, want_union = R.blend_ref(dest, src, plans)
    ex = P.PatchExHIP("cuda")
    out, label, union = ex(cu(dest), cu(src), plans, label_mode="binary")
    out, label, union = out.cpu().numpy(), label.cpu().numpy(), union.cpu().numpy()
    for b in range(dest.shape[0]):
        assert np.array_equal(out[b], want[b]), (name, b, int((out[b] != want[b]).sum()))
        assert np.array_equal(union[b], want_union[b]), (name, b)
        R.check_label(label[b], R.label_ref(dest[b], want[b], want_union[b], 0, 1, plans[b][1], 0, 0), 0)
    assert np.array_equal(out[1], dest[1]) and not union[1].any() and not label[1].any()


# ================================================================================================ 3. label
MODE3_WORST = [0.0]


def _label_call(dest, out, union, sums, lm, label, factor, B, H, W, mode, tol, k, x0):
    lib, s = _lib()
    p = lambda t: None if t is None else t.data_ptr()
    return lib.mh_patch_label(p(dest), p(out), p(union), p(sums), p(lm), p(label), p(factor), B, H, W, mode, tol, float(k), float(x0), s)


@pytest.mark.parametrize("case", R.label_cases(), ids=[c[0] for c in R.label_cases()])
def test_label_matches_label_ref(case):
    name, dest, out, union = case
    B, H, W = union.shape
    n = B * H * W
    d, o, u = cu(dest), cu(out), cu(union)
    factor = cu(np.array([R.label_factor(b) for b in range(B)], np.float64))
    worst = 0.0
    for mode, tol, k, x0 in R.label_runs():
        sums = torch.full((n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        lm = byte_buf(n + 16)
        label = nan_buf(n + 16)
        assert _label_call(d, o, u, sums, lm, label, factor, B, H, W, mode, tol, k, x0) == OK
        got = label[:n].cpu().numpy().reshape(B, H, W)
        assert is_poison(label[n:]) and is_poison(lm[n:]) and bool((sums[n:] == 0x5A5A5A5A).all())
        worst = max(worst, R.check_label(got, R.label_refs(name, dest, out, union, mode, tol, k, x0), mode))
    MODE3_WORST[0] = max(MODE3_WORST[0], worst)
    print(f"{name}: mode-3 err / bound {worst:.4f} (largest so far {MODE3_WORST[0]:.4f})")


def test_label_entry_refusals():
    name, dest, out, union = R.label_cases()[0]
    B, H, W = union.shape
    n = B * H * W
    d, o, u = cu(dest), cu(out), cu(union)
    factor = cu(np.full(B, 0.5))
    sums, lm, label = torch.zeros(n, dtype=torch.int32, device="cuda"), byte_buf(n), nan_buf(n)
    good = [d, o, u, sums, lm, label, factor, B, H, W, 0, 1, 1 / 6, 20.0]
    for i in range(6):                                                          # each null pointer
        a = list(good)
        a[i] = None
        assert _label_call(*a) == ERR, i
    a = list(good)
    a[6], a[10] = None, 1                                                       # continuous without its factors
    assert _label_call(*a) == ERR
    for mode in (4, -1):
        a = list(good)
        a[10] = mode
        assert _label_call(*a) == ERR
    for Bz in (0, -1):                                                          # no images: OK, nothing written
        a = list(good)
        a[7] = Bz
        assert _label_call(*a) == OK
    assert is_poison(label) and is_poison(lm) and not bool(sums.any())
    a = list(good)
    a[6] = None                                                                 # the other modes need no factors
    assert _label_call(*a) == OK
    R.check_label(label.cpu().numpy().reshape(B, H, W), R.label_refs(name, dest, out, union, 0, 1), 0)


# ================================================================================================ 4. resize
RESIZE_SRC_SHAPE = (2, 37, 53)
RESIZE_CASES = [((27, 41, 10, 12), (6, 5)),         # the exact 2 x 2 halving on a box that ends at the bottom-right corner
                ((35, 51, 2, 2), (1, 1)),           # ... down to one pixel, the corner's last four
                ((36, 3, 1, 40), (17, 5)),          # sh = 1
                ((2, 52, 30, 1), (4, 9)),           # sw = 1, the last column
                ((5, 6, 9, 11), (1, 1)),            # a 1 x 1 output on the linear path
                ((0, 0, 37, 53), (20, 11)),         # the whole non-square image down
                ((3, 4, 11, 17), (30, 20)),         # up
                ((30, 0, 7, 53), (53, 7))]          # identity at the bottom rows


def _resize(src_dev, image, box, wh, tabs=True, out=None, H=37, W=53, null=()):
    lib, s = _lib()
    (sy, sx, sh, sw), (w, h) = box, wh
    keep, ptrs = None, [None] * 4
    if tabs and w > 0 and h > 0:
        xi, xw = P.linear_resize_tables(sw, w)
        yi, yw = P.linear_resize_tables(sh, h)
        keep = cu(np.concatenate([xi, xw.reshape(-1), yi, yw.reshape(-1)]).astype(np.int32))
        tp = keep.data_ptr()
        ptrs = [tp, tp + 4 * w, tp + 4 * 3 * w, tp + 4 * (3 * w + h)]
    for i in null:
        ptrs[i] = None
    rc = lib.mh_patch_resize_u8(None if src_dev is None else src_dev.data_ptr(), image, H, W, sy, sx, sh, sw, *ptrs,
                                None if out is None else out.data_ptr(), h, w, s)
    torch.cuda.synchronize()
    return rc


def test_resize_non_square_source_and_guards():
    img = np.random.RandomState(31).randint(0, 256, RESIZE_SRC_SHAPE + (3,)).astype(np.uint8)
    d = cu(img)
    for box, (w, h) in RESIZE_CASES:
        sy, sx, sh, sw = box
        buf = byte_buf(64 + h * w * 3 + 64)
        assert _resize(d, 1, box, (w, h), out=buf[64:]) == OK
        want = P.resize_linear_u8(img[1, sy:sy + sh, sx:sx + sw], (w, h))
        assert np.array_equal(buf[64:64 + h * w * 3].cpu().numpy().reshape(h, w, 3), want), (box, w, h)
        assert is_poison(buf[:64]) and is_poison(buf[64 + h * w * 3:])
    # the 2 x 2 halving takes no tables
    buf = byte_buf(5 * 6 * 3)
    assert _resize(d, 1, (27, 41, 10, 12), (6, 5), tabs=False, out=buf) == OK
    assert np.array_equal(buf.cpu().numpy().reshape(5, 6, 3), P.resize_linear_u8(img[1, 27:37, 41:53], (6, 5)))


def test_resize_refusals_leave_the_output_untouched():
    d = cu(np.random.RandomState(32).randint(0, 256, RESIZE_SRC_SHAPE + (3,)).astype(np.uint8))
    out = byte_buf(20 * 30 * 3)
    for box in ((28, 0, 10, 12), (0, 42, 10, 12), (-1, 0, 10, 12), (0, -1, 10, 12), (0, 0, 38, 53), (0, 0, 37, 54), (36, 52, 2, 2),
                (0, 0, 0, 12), (0, 0, 10, 0), (0, 0, -4, 12)):
        assert _resize(d, 1, box, (7, 9), tabs=box[2] > 0 and box[3] > 0, out=out) == ERR, box      # the box leaves the image
    assert _resize(d, 1, (27, 41, 10, 12), (6, 5), out=out, H=36) == ERR                             # ... by one row of a smaller image
    for i in range(4):                                                                             # a null table outside the area path
        assert _resize(d, 1, (3, 4, 11, 17), (30, 20), out=out, null=(i,)) == ERR, i
    assert _resize(None, 1, (3, 4, 11, 17), (30, 20), out=out) == ERR
    assert _resize(d, 1, (3, 4, 11, 17), (30, 20), out=None) == ERR
    for wh in ((30, 0), (0, 20), (30, -1), (-2, 20)):                                               # nothing to write: OK
        assert _resize(d, 1, (3, 4, 11, 17), wh, tabs=False, out=out) == OK, wh
    assert is_poison(out)


# ================================================================================================ 5. Poisson clone
def _poisson_call(ex, buf_img, image, H, W, patch, pms, roi, mixed, ws=None, change=None, null=()):
    lib, s = _lib()
    y0s, x0s, dy0, dx0, h, w = roi
    hp, wp = pms.shape
    keep = [cu(patch), cu(pms)]
    Sh = cy = Sw = cx = er = None
    if h >= 3 and w >= 3:
        er = cu(P.eroded_mask(pms, roi))
        Sh, cy = ex._dst_tables(h - 2)
        Sw, cx = ex._dst_tables(w - 2)
    n_ws = int(lib.mh_patch_poisson_ws_doubles(h, w))
    if ws is None:
        ws = torch.full((n_ws + 16,), float("nan"), dtype=torch.float64, device="cuda")
    a = dict(y0s=y0s, x0s=x0s, dy0=dy0, dx0=dx0, h=h, w=w, hp=hp, wp=wp, H=H, W=W)
    a.update(change or {})
    p = lambda t: None if t is None else t.data_ptr()
    ptr = dict(out=p(buf_img), patch=p(keep[0]), pms=p(keep[1]), er=p(er), Sh=p(Sh), cy=p(cy), Sw=p(Sw), cx=p(cx), ws=p(ws))
    for k in null:
        ptr[k] = None
    rc = lib.mh_patch_poisson_u8(ptr["out"], image, a["H"], a["W"], ptr["patch"], a["hp"], a["wp"], ptr["pms"], ptr["er"], a["y0s"],
                                 a["x0s"], a["dy0"], a["dx0"], a["h"], a["w"], ptr["Sh"], ptr["cy"], ptr["Sw"], ptr["cx"], ptr["ws"],
                                 1 if mixed else 0, s)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[n_ws:]).all())                                   # nothing past the stated workspace
    return rc


@pytest.mark.parametrize("case", R.poisson_cases(), ids=[c[0] for c in R.poisson_cases()])
def test_poisson_clone_matches_the_host_on_every_pixel(case):
    name, dest, image, steps = case
    B, H, W = R.POISSON_SHAPE
    want = R.poisson_apply_ref(dest, image, steps)
    assert not np.array_equal(want[image], dest[image]) and np.array_equal(want[1 - image], dest[1 - image])
    ex = P.PatchExHIP("cuda")
    buf = byte_buf(B + 2, H, W, 3)                                              # the two images between poisoned neighbours
    buf[1:1 + B] = cu(dest)
    for patch, pms, roi, mixed in steps:
        assert _poisson_call(ex, buf[1], image, H, W, patch, pms, roi, mixed) == OK
    got = buf[1:1 + B].cpu().numpy()
    assert np.array_equal(got[1 - image], dest[1 - image]), name                # the other image stays untouched
    diff = got[image] != want[image]
    assert not diff.any(), (name, int(diff.sum()), np.argwhere(diff)[:5].tolist())
    assert is_poison(buf[0]) and is_poison(buf[B + 1])


def test_poisson_through_patch_ex_two_overlapping_clones():
    """The same sequence through PatchExHIP (resample into the pool, clone, union mask, label) on a non-square crop."""
    name, dest, image, steps = [c for c in R.poisson_cases() if c[0] == "two_overlapping_normal"][0]
    _, H, W = R.POISSON_SHAPE
    r = np.random.RandomState(77)
    src = r.randint(0, 256, (H, W, 3)).astype(np.uint8)
    ops = []
    for n, (patch, pms, roi, mixed) in enumerate(steps):
        hp, wp = pms.shape
        sy, sx = (3, 5) if n == 0 else (22, 22)                                # the two source boxes do not overlap
        src[sy:sy + hp, sx:sx + wp] = patch
        mask = (pms != 0).astype(np.uint8)
        ops.append(P.PatchOp((sy, sx), (roi[2], roi[3], hp, wp), mask, 1.0, "mixed_clone" if mixed else "normal_clone", pms=pms, roi=roi))
    want, label, _ = P.apply_numpy(dest[image], src, ops, 1.0, "logistic-intensity", 1, (1 / 6, 20))
    assert np.array_equal(want, R.poisson_apply_ref(dest, image, steps)[image])
    ex = P.PatchExHIP("cuda")
    out, lab, union = ex(cu(dest[image][None]), cu(src[None]), [(ops, 1.0)], label_mode="logistic-intensity")
    assert np.array_equal(out[0].cpu().numpy(), want)
    wu = R.union_ref((H, W), ops)
    assert np.array_equal(union[0].cpu().numpy(), wu)
    R.check_label(lab[0].cpu().numpy(), R.label_ref(dest[image], want, wu, 3, 1, 1.0, 1 / 6, 20), 3)


def test_poisson_refusals_leave_the_image_untouched():
    B, H, W = R.POISSON_SHAPE
    r = np.random.RandomState(78)
    dest = r.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    patch = r.randint(0, 256, (12, 14, 3)).astype(np.uint8)
    pms = np.full((12, 14), 255, np.uint8)
    ex = P.PatchExHIP("cuda")
    buf = cu(dest)
    roi = (1, 2, 5, 6, 10, 11)                                                  # 10 x 11 at (1, 2) of the patch, (5, 6) of the image
    bad = [dict(y0s=3), dict(x0s=4), dict(y0s=-1), dict(x0s=-1), dict(hp=10), dict(wp=12),        # the ROI leaves the patch
           dict(dy0=H - 9), dict(dx0=W - 10), dict(dy0=-1), dict(dx0=-1), dict(H=14), dict(W=16)]  # ... or the image
    for change in bad:
        assert _poisson_call(ex, buf, 1, H, W, patch, pms, roi, False, change=change) == ERR, change
    for k in ("out", "patch", "pms", "er", "Sh", "cy", "Sw", "cx", "ws"):
        assert _poisson_call(ex, buf, 1, H, W, patch, pms, roi, False, null=(k,)) == ERR, k
    for hw in (dict(h=2), dict(w=2), dict(h=0), dict(w=-1)):                    # no interior: OK, nothing to solve
        assert _poisson_call(ex, buf, 1, H, W, patch, pms, roi, False, change=hw) == OK, hw
    assert torch.equal(buf, cu(dest))
    assert _lib()[0].mh_patch_poisson_ws_doubles(2, 9) == 0 and _lib()[0].mh_patch_poisson_ws_doubles(5, 9) == 6 * 3 * 7
