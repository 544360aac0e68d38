"""The vision expert's reference bank on the GPU (csrc/expert_bank.hip, VisionExpertHIP.add_references / one_shot_banked /
forward_banked, MyriadHIP's `ref_bank`): every output element against the fp64 restatement of tests/bank_ref.py, whose bounds
come from the rounding rules of tests/fp64_bounds.py (bf16 MFMA product with fp32 accumulation, the tap mean, 1 - x, the
bilinear resize) and are shown to reject the plausible kernel mistakes by tests/test_expert_bank_cpu.py; outputs start as poison
inside poisoned borders.  End to end the tolerances are those tests/test_expert_gpu.py states for the same quantities."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from myriad_amd.vision_expert import VisionExpertHIP  # noqa: E402
from tests import bank_ref as br  # noqa: E402
from tests import fp64_bounds as fb  # noqa: E402
from tests import golden_utils as gu  # noqa: E402
from tests.test_expert_oracle import load_case  # noqa: E402

DEV = "cuda"
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
BORDER = 64
COUNTS = [1, 1025, 15, 16, 17, 255, 256, 257, 1024, 4097]      # one class each, in this order: 1 row beside 1025 rows


def unit_rows(n, D, seed, centre=None, spread=1.0):
    """[n, D] unit rows rounded to bf16 (device); `centre`: rows scattered around that direction."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, D, generator=g, dtype=torch.float64) * spread
    if centre is not None:
        x = x + centre[None]
    return (x / x.norm(dim=-1, keepdim=True)).to(BF16).to(DEV)


def ranges_of(counts, gap=0, lead=0):
    out, off = [], lead
    for r in counts:
        out.append((off, r))
        off += r + gap
    return out, off


def bordered(shape, dtype=F32):
    """A poisoned flat buffer and the view of `shape` BORDER elements inside it."""
    n = 1
    for s in shape:
        n *= s
    buf = fb.poisoned((n + 2 * BORDER,), dtype, DEV)
    return buf, buf[BORDER:BORDER + n].view(shape)


def assert_borders(buf, what):
    fb.assert_untouched(buf[:BORDER], what + " (before)")
    fb.assert_untouched(buf[-BORDER:], what + " (behind)")


def test_chunk_rows_is_what_the_cpu_tests_assume():
    from tests.test_expert_bank_cpu import CHUNK
    assert ops._L().mh_bank_sim_chunk_rows() == CHUNK and ops.bank_sim_chunks(1) == 1 and ops.bank_sim_chunks(CHUNK + 1) == 2


# ------------------------------------------------------------------------------------------------ bank_sim_max per element
@pytest.mark.parametrize("L", [1, 15, 16, 17, 256])
@pytest.mark.parametrize("D", [32, 96, 1280])
def test_bank_sim_max_per_element(D, L):
    """One launch, ten samples of ten classes with every row count of the list (mixed counts, 1 beside 1025), class-token row
    skipped through the first-row offset and the per-sample stride; every chunk slot against its own fp64 value."""
    B, N = len(COUNTS), L + 1
    ranges, total = ranges_of(COUNTS)
    q = unit_rows(B * N, D, seed=D + L)
    bank = unit_rows(total, D, seed=D + L + 1)
    chunk = ops._L().mh_bank_sim_chunk_rows()
    max_chunks = ops.bank_sim_chunks(max(COUNTS))
    buf, part = bordered((B, max_chunks, L))
    out, _ = ops.bank_sim_max(q, bank, ranges, L, 1, N, out=part)
    assert out.data_ptr() == part.data_ptr()
    ref = br.chunk_max_ref_bound(q, bank, ranges, L, chunk, 1, N)
    worst = 0.0
    for b, (m, e) in enumerate(ref):
        n = m.shape[0]
        assert n == ops.bank_sim_chunks(COUNTS[b])
        worst = max(worst, fb.assert_within(part[b, :n], m, e, f"bank_sim_max D={D} L={L} rows={COUNTS[b]}"))
        fb.assert_untouched(part[b, n:], f"chunk slots past the last chunk of rows={COUNTS[b]}")
    assert_borders(buf, "bank_sim_max part")
    print(f"bank_sim_max D={D} L={L}: worst err/bound {worst:.3f}")


# --------------------------------------------------------------------------------------------- the whole head per element
def head_case(D, L, T, counts, seed):
    B, N = len(counts), L + 1
    ranges, total = ranges_of(counts)
    q_taps = [unit_rows(B * N, D, seed=seed + 2 * t) for t in range(T)]
    bank_taps = [unit_rows(total, D, seed=seed + 2 * t + 1) for t in range(T)]
    return q_taps, bank_taps, ranges, N


def run_head(q_taps, bank_taps, ranges, L, N, S):
    T, B = len(q_taps), len(ranges)
    part = torch.empty((T, B, max(ops.bank_sim_chunks(r) for _, r in ranges), L), dtype=F32, device=DEV)
    dr = None
    for t in range(T):
        _, dr = ops.bank_sim_max(q_taps[t], bank_taps[t], ranges, L, 1, N, out=part[t], dev_ranges=dr)
    return part, dr, ops.bank_sim_finish(part, dr[1], S)


@pytest.mark.parametrize("D,L,T,S", [(96, 1, 1, 7), (96, 16, 4, 24), (32, 256, 1, 224), (1280, 256, 4, 224)])
def test_head_per_element(D, L, T, S, monkeypatch):
    counts = [1, 1025, 17, 256, 257] if D == 1280 else COUNTS
    q_taps, bank_taps, ranges, N = head_case(D, L, T, counts, seed=7 * D + L)
    ref = br.head_ref_bound(q_taps, bank_taps, ranges, L, S, q_row0=1, q_sample_rows=N)
    with fb.poisoned_allocations(monkeypatch):
        part, dr, (sim, simmask, amap) = run_head(q_taps, bank_taps, ranges, L, N, S)
    worst = br.check_head(sim, simmask, amap, ref, f"head D={D} L={L} T={T}")
    print(f"head D={D} L={L} T={T}: worst err/bound {worst:.3f}")
    # the finish kernel again, into bordered outputs: same bits, nothing outside
    B, h = len(ranges), int(round(L ** 0.5))
    bufs = [bordered(s) for s in ((B, h, h), (B, h, h), (B, S, S))]
    _lib.check(ops._L().mh_bank_sim_finish(ops._p(part), ops._p(dr[1]), *(ops._p(v) for _, v in bufs), T, B, part.shape[2], h, S,
                                           1.0 / T, ops._s()), "mh_bank_sim_finish")
    for (buf, v), want, name in zip(bufs, (sim, simmask, amap), ("sim", "simmask", "amap")):
        assert torch.equal(v, want), name
        assert_borders(buf, f"bank_sim_finish {name}")


@pytest.mark.parametrize("T", [1, 4])
def test_finish_is_bit_equal_to_bilinear_ac(T):
    """Given the sim it wrote, both maps carry the bits of ops.bilinear_ac(sim, ., ., one_minus=True): 16 -> 224 and 16 -> 16."""
    q_taps, bank_taps, ranges, N = head_case(96, 256, T, [300, 1, 129], seed=50 + T)
    _, _, (sim, simmask, amap) = run_head(q_taps, bank_taps, ranges, 256, N, 224)
    assert torch.equal(amap, ops.bilinear_ac(sim, 224, 224, one_minus=True))
    assert torch.equal(simmask, ops.bilinear_ac(sim, 16, 16, one_minus=True))
    assert sim.shape == (3, 16, 16) and bool(torch.isfinite(sim).all())


# ------------------------------------------------------------------------------------------------------- neighbour trap
def test_neighbour_class_trap():
    """A sample's own rows are its negated queries (every cosine < 0: the queries share a direction) and the rows stored right
    before and right after its range are copies of its queries (cosine 1).  An overrun at either end, the next class's rows or
    zero padding of the last tile then fails by O(1).  Row counts off the tile and the chunk grid."""
    D, L, T, S = 96, 16, 1, 24
    N = L + 1
    counts = [1, 15, 17, 16, 3]
    B = len(counts)
    g = torch.Generator().manual_seed(3)
    centre = torch.randn(D, generator=g, dtype=torch.float64)
    centre = 3.0 * centre / centre.norm()
    q = unit_rows(B * N, D, seed=4, centre=centre, spread=0.1)
    ranges, total = ranges_of(counts, gap=L, lead=L)
    bank = torch.empty((total, D), dtype=BF16, device=DEV)
    for b, (off, r) in enumerate(ranges):
        patches = q[b * N + 1:(b + 1) * N]
        bank[off - L:off] = patches                                      # the class in front: copies of the queries
        bank[off:off + r] = -patches[torch.arange(r) % L]
        bank[off + r:off + r + L] = patches                              # the class behind
    ref = br.head_ref_bound([q], [bank], ranges, L, S, q_row0=1, q_sample_rows=N)
    assert float(ref["sim"][0].max()) < -0.5
    _, _, (sim, simmask, amap) = run_head([q], [bank], ranges, L, N, S)
    br.check_head(sim, simmask, amap, ref, "neighbour trap")
    assert float(sim.max()) < -0.5 and float(simmask.min()) > 1.5 and float(amap.min()) > 1.5


# --------------------------------------------------------------------------------------- independence and repeated classes
def test_a_sample_does_not_depend_on_its_batch_or_on_the_rest_of_the_bank():
    D, L, T, S = 96, 256, 4, 224
    N = L + 1
    rows = {"x": 385, "y": 1, "z": 200}
    qs = {n: [unit_rows(N, D, seed=100 + 10 * i + t) for t in range(T)] for i, n in enumerate("xyz")}
    cls = {n: [unit_rows(rows[n], D, seed=200 + 10 * i + t) for t in range(T)] for i, n in enumerate("xyz")}

    def run(batch, layout):
        ranges_all, _ = ranges_of([rows[n] for n in layout])
        where = dict(zip(layout, ranges_all))
        q_taps = [torch.cat([qs[n][t] for n in batch]) for t in range(T)]
        bank_taps = [torch.cat([cls[n][t] for n in layout]) for t in range(T)]
        _, _, out = run_head(q_taps, bank_taps, [where[n] for n in batch], L, N, S)
        return out

    alone = [o[0] for o in run("x", "x")]
    for batch, layout, row in (("xyz", "xyz", 0), ("yzx", "xyz", 2), ("x", "yxz", 0), ("zyx", "zxy", 2), ("xx", "yxz", 0),
                               ("xx", "yxz", 1), ("yxx", "xzy", 2)):
        got = [o[row] for o in run(batch, layout)]
        for a, b_, name in zip(alone, got, ("sim", "simmask", "amap")):
            assert torch.equal(a, b_), (batch, layout, name)


# ------------------------------------------------------------------------------------------------------------- refusals
def test_launcher_refusals_leave_the_outputs_untouched():
    D, L, N, B = 64, 16, 17, 2
    q, bank = unit_rows(B * N, D, seed=1), unit_rows(40, D, seed=2)
    off = torch.tensor([0, 20], dtype=I32, device=DEV)
    rows = torch.tensor([20, 20], dtype=I32, device=DEV)
    buf, part = bordered((B, 1, L))
    lib, p, s = ops._L(), ops._p, ops._s
    good = dict(q=p(q), q_row0=1, qsr=N, bank=p(bank), off=p(off), rows=p(rows), part=p(part), B=B, L=L, D=D, mc=1)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mh_bank_sim_max(a["q"], a["q_row0"], a["qsr"], a["bank"], a["off"], a["rows"], a["part"], a["B"], a["L"], a["D"],
                                   a["mc"], s())

    for kw in (dict(D=48), dict(D=16), dict(D=0), dict(L=0), dict(B=0), dict(mc=0), dict(q=None), dict(bank=None), dict(off=None),
               dict(rows=None), dict(part=None), dict(qsr=L)):
        with pytest.raises(_lib.MyriadHipError, match="MH_ERR_ARG"):
            _lib.check(call(**kw), f"mh_bank_sim_max {kw}")
    torch.cuda.synchronize()
    fb.assert_untouched(buf, "refused bank_sim_max")
    outs = [bordered(sh) for sh in ((B, 4, 4), (B, 4, 4), (B, 8, 8))]
    pp = fb.poisoned((1, B, 1, L), F32, DEV)
    fgood = dict(part=p(pp), rows=p(rows), sim=p(outs[0][1]), mask=p(outs[1][1]), amap=p(outs[2][1]), T=1, B=B, mc=1, h=4, S=8)

    def fcall(**kw):
        a = dict(fgood, **kw)
        return lib.mh_bank_sim_finish(a["part"], a["rows"], a["sim"], a["mask"], a["amap"], a["T"], a["B"], a["mc"], a["h"], a["S"],
                                      1.0, s())

    for kw in (dict(T=0), dict(B=0), dict(mc=0), dict(h=0), dict(S=0), dict(part=None), dict(rows=None), dict(sim=None),
               dict(mask=None), dict(amap=None)):
        with pytest.raises(_lib.MyriadHipError, match="MH_ERR_ARG"):
            _lib.check(fcall(**kw), f"mh_bank_sim_finish {kw}")
    torch.cuda.synchronize()
    for b_, _ in outs:
        fb.assert_untouched(b_, "refused bank_sim_finish")
    # the wrappers refuse what the launcher cannot see: a class without rows, a range outside the bank, mismatched widths
    for ranges in ([(0, 0), (0, 20)], [(0, 20), (30, 20)], [(-1, 5), (0, 20)]):
        with pytest.raises(_lib.MyriadHipError):
            ops.bank_sim_max(q, bank, ranges, L, 1, N, out=part)
    with pytest.raises(_lib.MyriadHipError):
        ops.bank_sim_max(q, unit_rows(40, 96, seed=3), [(0, 20), (20, 20)], L, 1, N, out=part)
    with pytest.raises(_lib.MyriadHipError):
        ops.bank_sim_max(unit_rows(B * N, 48, seed=4), unit_rows(40, 48, seed=5), [(0, 20), (20, 20)], L, 1, N, out=part)   # D % 32
    torch.cuda.synchronize()
    fb.assert_untouched(buf, "refused ops.bank_sim_max")


# ---------------------------------------------------------------------------------------- end to end on the committed goldens
@pytest.fixture(scope="module", params=["d1280_3blk", "d1280_1blk_k2"])
def golden_expert(request):
    g, cfg, sd, images, refs, text = load_case(request.param)
    return g, cfg, VisionExpertHIP(sd, cfg["heads"], cfg["layers"], DEV), images, refs, text


def test_banked_paths_vs_reference_golden(golden_expert):
    g, cfg, ex, images, refs, text = golden_expert
    B, k = cfg["B"], cfg["k"]
    names = [f"c{b}" for b in range(B)]
    for n in list(ex.bank_classes()):
        ex.drop_references(n)
    for b, n in enumerate(names):
        ex.add_references(n, refs[b * k:(b + 1) * k], text_feats=text[b])
    assert ex.bank_classes() == names and all(t.shape[0] == B * k * 256 and t.dtype == BF16 for t in ex._bank)
    omap, omask = ex.one_shot_banked(images, names)
    assert omap.shape == (B, 1, 224, 224) and omask.shape == (B, 1, 16, 16)
    assert (omap.cpu() - torch.from_numpy(g["os_map"])).abs().max() < 1e-2          # 1 - cosine similarity
    assert (omask.cpu() - torch.from_numpy(g["os_mask"])).abs().max() < 1e-2
    omap0, omask0 = ex.one_shot(images, refs)
    assert (omap - omap0).abs().max() < 1e-2 and (omask - omask0).abs().max() < 1e-2
    for tf in (None, text):                                                          # the bank's text pairs, or the caller's
        (zmap, zmask), (omap2, omask2) = ex.forward_banked(images, names, tf)
        assert (zmap.cpu() - torch.from_numpy(g["zs_map"])).abs().max() < 8e-2
        assert (zmask.cpu() - torch.from_numpy(g["zs_mask"])).abs().max() < 8e-2
        assert (zmap.cpu() - torch.from_numpy(g["zs_map"])).abs().mean() < 1e-2
        assert torch.equal(omap2, omap) and torch.equal(omask2, omask)               # same B-image trunk pass, same head
    # a batch in another order, with a class twice; replacing and dropping classes moves the others without changing them
    perm = [B - 1] + list(range(B - 1)) + [0]
    pmap, pmask = ex.one_shot_banked(images[perm], [names[i] for i in perm])
    assert (pmap - omap[perm]).abs().max() < 1e-2 and torch.equal(pmap[-1], pmap[1 if B > 1 else 0])
    ex.add_references(names[0], refs[:k], text_feats=text[0])                        # replace: now behind the last class
    assert ex.bank_classes() == names[1:] + names[:1]
    rmap, rmask = ex.one_shot_banked(images, names)
    assert torch.equal(rmap, omap) and torch.equal(rmask, omask)
    with pytest.raises(KeyError, match="zipper"):
        ex.one_shot_banked(images, ["zipper"] * B)
    with pytest.raises(KeyError, match="zipper"):
        ex.drop_references("zipper")
    if B > 1:
        ex.drop_references(names[1])
        assert names[1] not in ex.bank_classes() and ex._bank[0].shape[0] == (B - 1) * k * 256
        with pytest.raises(KeyError, match=names[1]):
            ex.forward_banked(images, names)
        dmap, _ = ex.one_shot_banked(images[:1], names[:1])                          # another batch size: another GEMM plan
        assert (dmap - omap[:1]).abs().max() < 1e-2


def test_rot90_registers_the_four_quarter_turns():
    g, cfg, sd, images, refs, text = load_case("d1280_1blk_k2")
    B, k = cfg["B"], cfg["k"]
    ex = VisionExpertHIP(sd, cfg["heads"], cfg["layers"], DEV)
    names = [f"c{b}" for b in range(B)]
    for b, n in enumerate(names):
        ex.add_references(n, refs[b * k:(b + 1) * k], rot90=True)
    assert all(t.shape[0] == B * 4 * k * 256 for t in ex._bank)
    assert [ex._bank_index.lookup(n) for n in names] == [(b * 4 * k * 256, 4 * k * 256) for b in range(B)]
    stack = torch.stack([torch.rot90(refs, r, dims=(2, 3)) for r in range(4)], dim=1).reshape(B * 4 * k, 3, 224, 224)
    omap, omask = ex.one_shot_banked(images, names)
    omap0, omask0 = ex.one_shot(images, stack)                                       # reference-major, then the turn
    assert (omap - omap0).abs().max() < 1e-2 and (omask - omask0).abs().max() < 1e-2
    with pytest.raises(KeyError, match="text pair"):
        ex.forward_banked(images, names)                                             # no text pair was registered


def test_model_with_ref_bank_equals_precomputed_maps():
    """The composite fixture of test_model_with_attached_expert_equals_precomputed_maps with class names in place of reference
    images: exactly the loss of forward_banked's maps handed in, for both task stages."""
    from myriad_amd.myriad import MyriadHIP
    from tests.test_model_gpu import _composite_sd
    sd = _composite_sd([1, 2, 3, 4, 5])
    image, _, before, after, tgt, tmask = gu.synthetic_batch(2, 1000, seed=6, pad_tail=1)
    _, cfg, esd, _, _, _ = load_case("d1280_1blk_k2")
    _, refs, text = gu.expert_inputs(2, 2, cfg["C"], seed=7)
    expert = VisionExpertHIP(esd, cfg["heads"], cfg["layers"], DEV)
    scene = ["bottle", "cable"]
    for b, n in enumerate(scene):
        expert.add_references(n, refs[2 * b:2 * b + 2], text_feats=text[b])
    base = dict(image=image, before_ids=before, after_ids=after, target_ids=tgt, target_mask=tmask)
    for task in (0, 1):
        model = MyriadHIP(sd, dict(fixed_stage=1, fixed_taskstage=task, need_backward=False), device=DEV)
        model.train()
        with pytest.raises(KeyError, match="ref_bank"):
            model.forward(dict(base, ref_bank=scene))                                # no expert attached: loud failure
        model.attach_vision_expert(expert)
        s1 = dict(base, ref_bank=scene)
        l1 = float(model.forward(s1)["loss"].detach())
        assert s1["anomaly_maps"].shape == (2, 1, 224, 224) and s1["oneshot_anomaly_maps"].shape == (2, 1, 224, 224)
        (zs, _), (osm, _) = expert.forward_banked(image.to(DEV), scene)
        l2 = float(model.forward(dict(base, anomaly_maps=zs, oneshot_anomaly_maps=osm))["loss"].detach())
        assert l1 == l2, (task, l1, l2)
        other = text.flip(0)                                                         # the caller's text pair wins over the bank's
        l3 = float(model.forward(dict(base, ref_bank=scene, expert_text_feats=other))["loss"].detach())
        (zs3, _), (osm3, _) = expert.forward_banked(image.to(DEV), scene, other)
        l4 = float(model.forward(dict(base, anomaly_maps=zs3, oneshot_anomaly_maps=osm3))["loss"].detach())
        assert l3 == l4, (task, l3, l4)
        with pytest.raises(KeyError, match="zipper"):
            model.forward(dict(base, ref_bank=["bottle", "zipper"]))
