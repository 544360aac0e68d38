"""VisionExpertHIP.compact_references / add_references(coreset=) / bank_stats on the GPU: what the coreset does to the banked
one-shot head.  Banks come from the committed golden expert case d1280_1blk_k2 and from synthetic banks written into the expert;
selections are held to tests/coreset_ref.py, the head to the bounds of tests/bank_ref.py."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import ops  # noqa: E402
from myriad_amd.expert_bank import BankIndex  # noqa: E402
from myriad_amd.vision_expert import VisionExpertHIP  # noqa: E402
from tests import bank_ref as br  # noqa: E402
from tests import coreset_ref as cr  # noqa: E402
from tests.test_expert_oracle import load_case  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def golden():
    g, cfg, sd, images, refs, text = load_case("d1280_1blk_k2")
    return cfg, VisionExpertHIP(sd, cfg["heads"], cfg["layers"], DEV), images.to(DEV), refs, text


def clear(ex):
    for n in list(ex.bank_classes()):
        ex.drop_references(n)


def write_bank(ex, classes):
    """A synthetic bank: classes = {name: [one [rows, D] bf16 tensor per tap]} in bank order."""
    ex._bank_index, ex._bank_text, ex._bank_meta = BankIndex(), {}, {}
    for name, taps in classes.items():
        ex._bank_index.append(name, taps[0].shape[0])
    T = len(next(iter(classes.values())))
    ex._bank = [torch.cat([taps[t].to(DEV) for taps in classes.values()]).contiguous() for t in range(T)]


def class_rows(ex, name):
    off, rows = ex._bank_index.lookup(name)
    return [t[off:off + rows].clone() for t in ex._bank]


def head(ex, qt, names):
    """_one_shot_banked_from_taps keeping the similarity: (normalised queries per tap, ranges, sim, simmask, amap)."""
    B, N, D = qt[0].shape
    L = N - 1
    ranges = [ex._bank_index.lookup(n) for n in names]
    part = torch.empty((len(qt), B, max(ops.bank_sim_chunks(r) for _, r in ranges), L), dtype=F32, device=DEV)
    dr, qns = None, []
    for i, (q, bank) in enumerate(zip(qt, ex._bank)):
        qn, _ = ops.l2norm_rows(q.reshape(B * N, D), eps=1e-8)
        qns.append(qn)
        _, dr = ops.bank_sim_max(qn, bank, ranges, L, 1, N, out=part[i], dev_ranges=dr)
    sim, simmask, amap = ops.bank_sim_finish(part, dr[1], ex.out_size)
    return qns, ranges, sim, simmask, amap


def check_keep_fewer(ex, qt, names, name, keep, **kw):
    """Compact `name`; sim never rises, and falls by at most cover_radius plus the head's two rounding bounds."""
    N = qt[0].shape[1]
    qns, ranges_f, sim_f, mask_f, _ = head(ex, qt, names)
    bank_f = [t.clone() for t in ex._bank]
    info = ex.compact_references(name, keep, **kw)
    _, ranges_c, sim_c, mask_c, _ = head(ex, qt, names)
    assert bool((sim_c <= sim_f).all()) and bool((mask_c >= mask_f).all())           # a max over a subset, monotone sums
    S = ex.out_size
    vf, ef = br.head_ref_bound(qns, bank_f, ranges_f, N - 1, S, q_row0=1, q_sample_rows=N)["sim"]
    vc, ec = br.head_ref_bound(qns, ex._bank, ranges_c, N - 1, S, q_row0=1, q_sample_rows=N)["sim"]
    drop = sim_f.double() - sim_c.double()
    assert bool((drop <= info["cover_radius"] + ef.to(drop.device) + ec.to(drop.device)).all()), (
        f"sim fell by {float(drop.max()):.4g}, cover_radius {info['cover_radius']:.4g}")
    print(f"keep {keep}: rows {info['rows_before']} -> {info['rows_after']}, largest drop of sim {float(drop.max()):.4f}, "
          f"cover_radius {info['cover_radius']:.4f}")
    return info


# ---------------------------------------------------------------------------------------------------- the golden bank
def test_keep_everything_then_fewer_on_the_golden_bank(golden):
    cfg, ex, images, refs, text = golden
    B, k = cfg["B"], cfg["k"]
    clear(ex)
    ex.add_references("c0", refs[:k], text_feats=text[0])
    rows = ex.bank_stats("c0")["rows"]
    assert ex.bank_stats("c0") == dict(rows=k * 256, rows_registered=k * 256, cover_radius=None)
    names = ["c0"] * B
    before = class_rows(ex, "c0")
    omap, omask = ex.one_shot_banked(images, names)
    info = ex.compact_references("c0", rows)                                         # keep everything: a permutation
    assert info["rows_before"] == info["rows_after"] == rows and info["exact"] is True and info["cover_radius"] == 0.0
    assert sorted(info["sel"]) == list(range(rows)) and info["sel"][0] == 0
    sel = torch.tensor(info["sel"], device=DEV)
    assert all(torch.equal(a, b[sel]) for a, b in zip(class_rows(ex, "c0"), before))
    omap2, omask2 = ex.one_shot_banked(images, names)
    assert torch.equal(omap2, omap) and torch.equal(omask2, omask)                   # a max does not see row order
    # keep fewer: the guarantee, then nesting (the kept rows are in selection order: a smaller keep is their prefix)
    _, qt = ex.trunk.forward(images)
    info = check_keep_fewer(ex, qt, names, "c0", 0.125)
    assert info["rows_after"] == math.ceil(0.125 * rows) and info["sel"] == list(range(info["rows_after"]))
    kept = class_rows(ex, "c0")
    stats = ex.bank_stats("c0")
    assert stats == dict(rows=info["rows_after"], rows_registered=rows, cover_radius=info["cover_radius"])
    host = [t.cpu() for t in before]
    full = ops.coreset_select(before, info["rows_after"])
    cr.replay_check(host, full.sel, full.radius2, start=0, mind=full.mind, cover2=full.cover2, what="golden bank")
    assert info["cover_radius"] == math.sqrt(max(float(full.cover2), 0.0))
    again = ex.compact_references("c0", 16)
    assert again["sel"] == list(range(16)) and again["rows_before"] == info["rows_after"]
    assert all(torch.equal(a, b[:16]) for a, b in zip(class_rows(ex, "c0"), kept))
    with pytest.raises(KeyError, match="zipper"):
        ex.compact_references("zipper", 4)
    with pytest.raises(KeyError, match="zipper"):
        ex.bank_stats("zipper")
    for bad in (0, 17, 0.0, 1.5, "half"):
        with pytest.raises(ValueError):
            ex.compact_references("c0", bad)
    for kw in (dict(start=16), dict(start=-1), dict(proj_dim=12), dict(proj_dim=0), dict(proj_dim=cfg["D"] + 8)):
        with pytest.raises(ValueError):
            ex.compact_references("c0", 4, **kw)
    assert ex.bank_stats("c0")["rows"] == 16                                         # a refused call changes nothing


def test_compacting_the_middle_class_of_three(golden):
    cfg, ex, images, refs, text = golden
    B, k = cfg["B"], cfg["k"]
    clear(ex)
    ex.add_references("left", refs[:k], text_feats=text[0])
    ex.add_references("mid", refs[-k:], text_feats=text[-1])
    ex.add_references("right", refs[:1], text_feats=text[0])
    outer = ["left", "right"] * B
    outer = outer[:B]
    rows_l, rows_r = class_rows(ex, "left"), class_rows(ex, "right")
    omap, omask = ex.one_shot_banked(images, outer)
    info = ex.compact_references("mid", 0.25)
    assert info["rows_after"] == k * 64 and ex.bank_classes() == ["left", "mid", "right"]
    assert ex._bank_index.lookup("right") == (k * 256 + k * 64, 256) and all(t.shape[0] == k * 320 + 256 for t in ex._bank)
    assert all(torch.equal(a, b) for a, b in zip(class_rows(ex, "left"), rows_l))
    assert all(torch.equal(a, b) for a, b in zip(class_rows(ex, "right"), rows_r))
    omap2, omask2 = ex.one_shot_banked(images, outer)
    assert torch.equal(omap2, omap) and torch.equal(omask2, omask)
    (zmap, _), (fmap, fmask) = ex.forward_banked(images, ["mid"] * B)                # the text pair survived the compaction
    mmap, mmask = ex.one_shot_banked(images, ["mid"] * B)
    assert torch.equal(fmap, mmap) and torch.equal(fmask, mmask) and bool(torch.isfinite(zmap).all())
    ex.drop_references("mid")
    assert ex.bank_classes() == ["left", "right"] and ex._bank_index.lookup("right") == (k * 256, 256)
    omap3, _ = ex.one_shot_banked(images, outer)
    assert torch.equal(omap3, omap)
    ex.add_references("mid", refs[-k:], text_feats=text[-1])                         # registered again: whole, never compacted
    assert ex.bank_stats("mid") == dict(rows=k * 256, rows_registered=k * 256, cover_radius=None)


def test_add_references_with_coreset_equals_add_then_compact(golden):
    cfg, ex, images, refs, text = golden
    k = cfg["k"]
    clear(ex)
    ex.add_references("c0", refs[:k], text_feats=text[0], coreset=0.25)
    one, stats = class_rows(ex, "c0"), ex.bank_stats("c0")
    assert stats["rows"] == k * 64 and stats["rows_registered"] == k * 256 and stats["cover_radius"] > 0
    ex.add_references("c0", refs[:k], text_feats=text[0])
    info = ex.compact_references("c0", 0.25)
    assert all(torch.equal(a, b) for a, b in zip(class_rows(ex, "c0"), one))
    assert ex.bank_stats("c0") == stats and info["cover_radius"] == stats["cover_radius"]
    # a value out of range is refused before the bank is touched: the registered class stays, a new name is not registered
    for bad in (1.5, 0, k * 256 + 1, "half"):
        with pytest.raises(ValueError):
            ex.add_references("c0", refs[:k], text_feats=text[0], coreset=bad)
        with pytest.raises(ValueError):
            ex.add_references("c9", refs[:k], coreset=bad)
    assert ex.bank_classes() == ["c0"] and ex.bank_stats("c0") == stats
    assert all(torch.equal(a, b) for a, b in zip(class_rows(ex, "c0"), one))


# -------------------------------------------------------------------------------------------------- synthetic banks
def synthetic_queries(B, N, D, T, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, N, D, generator=g).to(DEV) for _ in range(T)]


def test_coverage_of_unequal_clusters(golden):
    """Six clusters of 900 / 40 / 30 / 20 / 7 / 3 rows, the big one first: keep = 6 returns one row of every cluster where a
    truncation to six rows holds cluster 0 alone (tests/test_coreset_cpu.py checks the same case on the fp64 rule)."""
    _, ex, _, _, _ = golden
    taps, label = cr.sized_clusters(cr.COVER_SIZES, 96, 2, seed=5)
    write_bank(ex, {"parts": taps})
    info = ex.compact_references("parts", 6)
    assert sorted(int(label[s]) for s in info["sel"]) == [0, 1, 2, 3, 4, 5] and set(label[:6].tolist()) == {0}
    res = ops.coreset_select([t.to(DEV) for t in taps], 6)
    assert res.sel.tolist() == info["sel"] and info["cover_radius"] == math.sqrt(float(res.cover2))
    cr.replay_check(taps, res.sel, res.radius2, start=0, mind=res.mind, cover2=res.cover2, what="coverage")
    assert info["sel"] == cr.COVER_SEL                                               # no near tie here: the radii are far apart
    g = cr.gamma(96, 2)                                                              # the recorded fp64 values, within gamma
    want = torch.tensor(cr.COVER_RADIUS2, dtype=torch.float64)
    assert bool(((res.radius2[1:].cpu().double() - want).abs() <= g * want + 1e-9).all())
    assert abs(float(res.cover2) - cr.COVER_COVER2) <= g * cr.COVER_COVER2 + 1e-9
    sel = torch.tensor(info["sel"])
    assert all(torch.equal(a.cpu(), t[sel]) for a, t in zip(class_rows(ex, "parts"), taps))


def test_keep_fewer_on_a_synthetic_bank_of_three_classes(golden):
    _, ex, _, _, _ = golden
    D, T, N, B = 96, 2, 17, 3
    classes = {"a": cr.unit_case(300, D, T, seed=1, clusters=7, spread=0.3), "b": cr.unit_case(515, D, T, seed=2),
               "c": cr.unit_case(65, D, T, seed=3, clusters=3, spread=0.5)}
    write_bank(ex, classes)
    qt = synthetic_queries(B, N, D, T, seed=4)
    names = ["b", "a", "b"]
    rows_a, rows_c = class_rows(ex, "a"), class_rows(ex, "c")
    _, _, sim_a, _, _ = head(ex, qt[:], ["a", "c", "a"])
    info = check_keep_fewer(ex, qt, names, "b", 0.1, start=514)
    assert info["rows_after"] == 52 and info["sel"][0] == 514 and ex._bank_index.lookup("c") == (352, 65)
    assert all(torch.equal(x, y) for x, y in zip(class_rows(ex, "a"), rows_a))
    assert all(torch.equal(x, y) for x, y in zip(class_rows(ex, "c"), rows_c))
    _, _, sim_a2, _, _ = head(ex, qt, ["a", "c", "a"])
    assert torch.equal(sim_a2, sim_a)                                                # the other classes' map bits
    check_keep_fewer(ex, qt, ["a", "a", "c"], "a", 7)
    check_keep_fewer(ex, qt, ["c", "c", "c"], "c", 1)                                # one centre: the radius of the class


def test_projection_selects_on_the_documented_products(golden):
    _, ex, _, _, _ = golden
    D, T, P, seed = 128, 2, 32, 9                                                    # ops.gemm takes K % 64 == 0
    classes = {"x": cr.unit_case(70, D, T, seed=5), "y": cr.unit_case(400, D, T, seed=6, clusters=11, spread=0.4),
               "z": cr.unit_case(3, D, T, seed=7)}
    write_bank(ex, classes)
    before = class_rows(ex, "y")
    proj = []
    for t in range(T):
        G = (torch.randn(P, D, generator=torch.Generator("cpu").manual_seed(seed + t)) / math.sqrt(P)).to(BF16)
        proj.append(ops.gemm(before[t], G.to(DEV)))
    want = ops.coreset_select(proj, 40, start=2)
    info = ex.compact_references("y", 0.1, proj_dim=P, seed=seed, start=2)
    assert info["exact"] is False and info["rows_after"] == 40 and info["sel"] == want.sel.tolist()
    assert info["cover_radius"] == math.sqrt(max(float(want.cover2), 0.0))
    cr.replay_check([p.cpu() for p in proj], want.sel, want.radius2, start=2, mind=want.mind, cover2=want.cover2, what="projected")
    sel = torch.tensor(info["sel"], device=DEV)
    assert all(torch.equal(a, b[sel]) for a, b in zip(class_rows(ex, "y"), before))     # the rows kept are original rows
    assert all(torch.equal(a.cpu(), c) for a, c in zip(class_rows(ex, "x"), classes["x"]))
    assert all(torch.equal(a.cpu(), c) for a, c in zip(class_rows(ex, "z"), classes["z"]))
    other = ex.compact_references("x", 10, proj_dim=P, seed=seed + 1)                # another seed: another projection
    assert other["exact"] is False and len(set(other["sel"])) == 10
    # the projection is an ops.gemm product: a tap width that is no multiple of 64 is refused, the bank stays as it was
    narrow = {"w": cr.unit_case(50, 96, T, seed=8)}
    write_bank(ex, narrow)
    with pytest.raises(ValueError, match="multiple of 64"):
        ex.compact_references("w", 10, proj_dim=P)
    assert ex.bank_stats("w")["rows"] == 50 and all(torch.equal(a.cpu(), c) for a, c in zip(class_rows(ex, "w"), narrow["w"]))
    assert ex.compact_references("w", 10)["rows_after"] == 10                        # without a projection D = 96 is fine
