#!/usr/bin/env python3
"""Vision expert at full size: ImageBind-Huge vision trunk (1280 x 32 blocks, 257 tokens, taps 7/15/23/31)
+ zero-shot and one-shot map heads, synthetic weights.  python tools/expert_bench.py [--batch 8] [--k 1]
--bank: the per-class reference bank against today's one_shot in one process, variants interleaved, medians of --reps:
(a) the whole call, one_shot(images, refs) vs one_shot_banked(images, names), and add_references per class;
(b) the head alone on identical taps, the per-sample GEMM + rowmax_skip loop vs bank_sim_max per tap + bank_sim_finish.
--coreset [--refs 200]: a full-shot class of synthetic unit rows compacted by compact_references to 10 % and 1 %, exact and with
proj_dim 128, configurations interleaved, medians of --reps: the selection in ms and us per iteration beside its floor, the head
alone and one_shot_banked on the full bank against each coreset, and the largest loss of similarity beside cover_radius."""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from myriad_amd import ops
from myriad_amd.vision_expert import VisionExpertHIP
from tests import golden_utils as gu

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--k", type=int, default=1)
ap.add_argument("--blocks", type=int, default=32)
ap.add_argument("--bank", action="store_true", help="compare the reference bank with one_shot (see the module docstring)")
ap.add_argument("--coreset", action="store_true", help="greedy k-centre coreset of a full-shot class (compact_references)")
ap.add_argument("--refs", type=int, default=200, help="--coreset: references of the class (256 bank rows each)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--cpu", type=int, default=0, help="also time the oracle trunk (oracle/expert_ref.vision_trunk, fp32) on this many host threads, 2 images")
a = ap.parse_args()
dev = "cuda:0"
ops.ensure_workspace(dev)
layers = [7, 15, 23, 31] if a.blocks == 32 else [a.blocks - 1]
sd = gu.expert_weights(1280, a.blocks, 1024, len(layers), seed=1)
ex = VisionExpertHIP(sd, 16, layers, dev)
sd_cpu = sd if a.cpu else None
del sd
images, refs, text = gu.expert_inputs(a.batch, a.k, 1024, seed=2)
images, refs, text = images.to(dev), refs.to(dev), text.to(dev)
B = a.batch
# per image: patch stem + 32 blocks (4 D^2 + 8 D^2 linear MACs per token, attention 2 N D per token) -- SURVEY 8f: 334 GF
N, D = 257, 1280
gf_img = (2 * 256 * 588 * D + a.blocks * (2 * N * 12 * D * D + 4 * N * N * D)) / 1e9


def timeit(fn, n=5):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def bank_bench():
    names = [f"class{b % 4}" for b in range(B)]                      # a batch of 4 classes, each twice at batch 8
    k = a.k
    per_class = {n: refs[b * k:(b + 1) * k] for b, n in reversed(list(enumerate(names)))}
    t_add = []
    for n, r in per_class.items():
        ex.add_references(n, r)                                      # warm-up of this shape, then the timed replacement
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ex.add_references(n, r)
        torch.cuda.synchronize()
        t_add.append(time.perf_counter() - t0)
    ref_rows = torch.cat([per_class[n] for n in names])              # what one_shot gets: each sample's own class references
    _, qt = ex.trunk.forward(images)
    _, rt = ex.trunk.forward(ref_rows)
    launches = {}

    def count(fn, key):
        seen = []
        orig = ops._lib.check
        ops._lib.check = lambda rc, what: (seen.append(what), orig(rc, what))[1]
        try:
            fn()
        finally:
            ops._lib.check = orig
        launches[key] = len(seen)

    variants = {"one_shot": lambda: ex.one_shot(images, ref_rows), "one_shot_banked": lambda: ex.one_shot_banked(images, names),
                "head_loop": lambda: ex._one_shot_from_taps(qt, rt), "head_banked": lambda: ex._one_shot_banked_from_taps(qt, names)}
    for key in ("head_loop", "head_banked"):
        count(variants[key], key)
    times = {key: [] for key in variants}
    for key, fn in variants.items():                                 # warm-up: every variant twice before any is timed
        fn(); fn()
    torch.cuda.synchronize()
    inner = {"one_shot": 4, "one_shot_banked": 4, "head_loop": 32, "head_banked": 32}     # calls per sample: a window of tens of ms
    for _ in range(a.reps):                                          # interleaved: one sample of every variant per round
        for key, fn in variants.items():
            t0 = time.perf_counter()
            for _ in range(inner[key]):
                fn()
            torch.cuda.synchronize()
            times[key].append((time.perf_counter() - t0) / inner[key])
    med = {key: statistics.median(v) for key, v in times.items()}
    print("  spread (min .. max of the samples, ms): " + "   ".join(f"{key} {min(v)*1e3:.3f} .. {max(v)*1e3:.3f}" for key, v in times.items()))
    diff = max(float((x - y).abs().max()) for x, y in zip(variants["one_shot"](), variants["one_shot_banked"]()))
    print(f"bank, batch {B}, k={k}, {a.blocks} blocks, medians of {a.reps} (interleaved):")
    print(f"  (a) whole call  one_shot {med['one_shot']*1e3:.2f} ms ({B*(1+k)} trunk passes)   one_shot_banked "
          f"{med['one_shot_banked']*1e3:.2f} ms ({B} trunk passes)   x{med['one_shot']/med['one_shot_banked']:.2f}   "
          f"add_references {statistics.median(t_add)*1e3:.2f} ms per class of {k}   max |map difference| {diff:.2e}")
    print(f"  (b) head alone  loop {med['head_loop']*1e6:.0f} us in {launches['head_loop']} library calls   bank_sim_max x{len(qt)} + "
          f"finish {med['head_banked']*1e6:.0f} us in {launches['head_banked']} library calls   x{med['head_loop']/med['head_banked']:.2f}   "
          f"(both include the l2norm_rows launches; the loop also normalises the reference rows)")


def coreset_bench():
    """A full-shot class of --refs references (256 rows each) of synthetic unit rows, compacted to 10 % and 1 %, exact and with
    a 128-wide projection: the selection's time per iteration beside its floor, what the coreset saves in the head, and what
    it costs in similarity beside the cover radius."""
    import math
    from myriad_amd.expert_bank import BankIndex
    T, rows = len(layers), a.refs * 256
    g = torch.Generator(device=dev).manual_seed(3)

    def unit(x):
        return (x / x.norm(dim=-1, keepdim=True)).to(torch.bfloat16)

    # rows scattered around 4096 directions per tap (row i around direction i % 4096 in every tap): near-duplicates, as the
    # patches of aligned normal images are; queries around the same directions
    centres = [torch.randn(4096, D, device=dev, generator=g) / math.sqrt(D) for _ in range(T)]
    full = [unit(c[torch.arange(rows, device=dev) % 4096] + 0.5 * torch.randn(rows, D, device=dev, generator=g) / math.sqrt(D))
            for c in centres]
    nq = 64
    qt = [(c[torch.randint(0, 4096, (nq * N,), device=dev, generator=g)]
           + 0.5 * torch.randn(nq * N, D, device=dev, generator=g) / math.sqrt(D)).view(nq, N, D) for c in centres]

    def write_full():
        ex._bank_index, ex._bank_text, ex._bank_meta = BankIndex(), {}, {}
        ex._bank_index.append("full", rows)
        ex._bank = list(full)

    def sims(names):
        """The head of _one_shot_banked_from_taps on the 64 synthetic queries, keeping sim."""
        out = []
        for b0 in range(0, nq, 8):
            q8 = [t[b0:b0 + 8] for t in qt]
            L = N - 1
            ranges = [ex._bank_index.lookup(n) for n in names]
            part = torch.empty((T, 8, max(ops.bank_sim_chunks(r) for _, r in ranges), L), dtype=torch.float32, device=dev)
            dr = None
            for i, (q, bank) in enumerate(zip(q8, ex._bank)):
                qn, _ = ops.l2norm_rows(q.reshape(8 * N, D), eps=1e-8)
                _, dr = ops.bank_sim_max(qn, bank, ranges, L, 1, N, out=part[i], dev_ranges=dr)
            out.append(ops.bank_sim_finish(part, dr[1], ex.out_size)[0])
        return torch.cat(out)

    names = ["full"] * B
    write_full()
    sim_full = sims(["full"] * 8)
    q8 = [t[:B].contiguous() for t in qt]
    configs = [(0.10, None), (0.01, None), (0.10, 128), (0.01, 128)]
    t_sel = {c: [] for c in configs}
    info = {}
    for rep in range(a.reps + 1):                                    # round 0 warms every configuration up
        for c in configs:
            write_full()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info[c] = ex.compact_references("full", c[0], proj_dim=c[1])     # returns after reading cover2: synchronised
            if rep:
                t_sel[c].append(time.perf_counter() - t0)
    bank_bytes = T * rows * D * 2
    print(f"coreset, {a.refs} references = {rows} rows x D {D} x {T} taps ({bank_bytes/1e6:.0f} MB), medians of {a.reps} (interleaved):")
    for c in configs:
        n = info[c]["rows_after"]
        med = statistics.median(t_sel[c])
        if c[1] is None:
            floor = f"byte floor {bank_bytes/6.29e12*1e6:.1f} us (bank bytes / 6.29 TB/s)"
        else:
            floor = (f"floor 2 launch boundaries = 3.4-3.8 us (the projected rows, {T*rows*c[1]*2/1e6:.0f} MB, stay in the "
                     f"Infinity Cache); includes the {T} projection GEMMs")
        print(f"  keep {c[0]:.2f} proj {c[1]}: {n} rows  selection {med*1e3:.1f} ms ({min(t_sel[c])*1e3:.1f} .. {max(t_sel[c])*1e3:.1f})"
              f"  {med/n*1e6:.1f} us per iteration  [{floor}]  cover_radius {info[c]['cover_radius']:.4f}")
    # the head and the whole call on the full bank against the coresets, and what the similarity lost
    banks = {"full": (list(full), rows)}
    for c in configs:
        write_full()
        ex.compact_references("full", c[0], proj_dim=c[1])
        banks[f"keep {c[0]:.2f} proj {c[1]}"] = (list(ex._bank), ex._bank_index.lookup("full")[1])

    def use(key):
        tensors, r = banks[key]
        ex._bank_index = BankIndex()
        ex._bank_index.append("full", r)
        ex._bank = list(tensors)

    times = {(key, what): [] for key in banks for what in ("head", "call")}
    for rep in range(a.reps + 1):
        for key in banks:
            use(key)
            for what, fn, inner in (("head", lambda: ex._one_shot_banked_from_taps(q8, names), 8),
                                    ("call", lambda: ex.one_shot_banked(images, names), 2)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                torch.cuda.synchronize()
                if rep:
                    times[(key, what)].append((time.perf_counter() - t0) / inner)
    for key in banks:
        use(key)
        drop = float((sim_full - sims(["full"] * 8)).max()) if key != "full" else 0.0
        c = next((info[c] for c in configs if key == f"keep {c[0]:.2f} proj {c[1]}"), None)
        print(f"  {key}: {banks[key][1]} rows  head alone (batch {B}) {statistics.median(times[(key, 'head')])*1e6:.0f} us   "
              f"one_shot_banked {statistics.median(times[(key, 'call')])*1e3:.2f} ms   max sim_full - sim_coreset over {nq} "
              f"queries {drop:.4f}" + (f"   cover_radius {c['cover_radius']:.4f}" + ("" if c["exact"] else " (projected space)") if c else ""))


if a.coreset:
    coreset_bench()
    sys.exit(0)

if a.bank:
    bank_bench()
    sys.exit(0)

t_trunk = timeit(lambda: ex.trunk.forward(images))
t_zs = timeit(lambda: ex.zero_shot(images, text))
t_os = timeit(lambda: ex.one_shot(images, refs))
t_both = timeit(lambda: ex.forward(images, text, refs))
print(f"batch {B}, k={a.k}: trunk {t_trunk*1e3:.2f} ms ({B/t_trunk:.0f} img/s, {B*gf_img/t_trunk/1e3:.0f} TFLOP/s of {gf_img:.0f} GF/img); "
      f"zero-shot maps {t_zs*1e3:.2f} ms ({B/t_zs:.0f} img/s); one-shot maps {t_os*1e3:.2f} ms ({B/t_os:.0f} img/s, "
      f"{B*(1+a.k)} trunk passes); both map pairs from one pass over [images; references] {t_both*1e3:.2f} ms ({B/t_both:.0f} img/s)")

if a.cpu:
    from oracle import expert_ref as OR          # CPU leg of this bench only
    torch.set_num_threads(a.cpu)
    img2 = images[:2].cpu()
    with torch.no_grad():
        OR.vision_trunk(sd_cpu, img2[:1], 16, layers, a.blocks)
        t0 = time.perf_counter()
        OR.vision_trunk(sd_cpu, img2, 16, layers, a.blocks)
        t_cpu = (time.perf_counter() - t0) / 2
    print(f"oracle trunk on {a.cpu} host threads (fp32): {t_cpu*1e3:.0f} ms/image = {1/t_cpu:.2f} img/s ({gf_img/t_cpu/1e3:.2f} TFLOP/s)")
