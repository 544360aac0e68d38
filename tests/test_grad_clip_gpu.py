"""Global gradient-norm clipping and the non-finite step guard on the device (csrc/optim.hip: mh_grad_sumsq, mh_clip_finalize,
mh_adamw_gated_ctl, mh_adamw_bump_ctl; ParamStore.adamw_step(clip=...); MyriadHIP.train_step(max_grad_norm=, skip_nonfinite=)).
The float64 rule and its bounds live in tests/grad_clip_ref.py; the AdamW reference and its budgets in tests/adamw_ref.py."""
import math

import pytest
import torch

from tests import grad_clip_ref as G

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F64 = torch.float64
GRID_CAP = 256 * 16                                              # adamw_gated_kernel's grid cap, and the norm's


def _exact_sumsq(*pieces) -> float:
    """The exact sum of squares (fp32 squares are exact in fp64; math.fsum adds them without error), rounded once."""
    vals = []
    for p in pieces:
        vals.extend(p.detach().double().pow(2).cpu().tolist())
    return math.fsum(vals)


def _device_sumsq(pieces, used):
    """mh_grad_sumsq over `pieces` with the per-piece device flags `used`, then the partials added in the device's own order
    (mh_clip_rank_sum with one rank).  -> (sum, the partials written, slots per piece)."""
    from myriad_amd import ops
    slots = [ops.grad_sumsq_slots(p.numel()) for p in pieces]
    ws = torch.full((sum(slots) + 8,), -7.0, dtype=F64, device=DEV)          # poisoned: every slot must be written
    off = 0
    for i, p in enumerate(pieces):
        assert ops.grad_sumsq(p, used[i:i + 1], ws[off:]) == slots[i]
        off += slots[i]
    out = torch.zeros(1, dtype=F64, device=DEV)
    ops.clip_rank_sum(ws, off, out, 0)
    torch.cuda.synchronize()
    assert bool((ws[off:] == -7.0).all())                                    # and nothing behind them
    return float(out[0]), ws[:off].clone(), slots


@pytest.mark.parametrize("n", [4, 1020, 4 * 256 + 4, 4 * 256 * GRID_CAP + 4])
def test_sumsq_is_the_fp64_sum_and_deterministic(n):
    """Check 1: |sumsq - ref| <= (n + 16) * 2^-53 * ref at one float4, a partial block, two blocks and a grid-stride that wraps
    once; two runs give equal bits."""
    from myriad_amd import ops
    g = torch.randn(n, generator=torch.Generator(device=DEV).manual_seed(n % 1000), device=DEV)
    used = torch.ones(1, device=DEV)
    assert ops.grad_sumsq_slots(n) == min(GRID_CAP, -(-(n // 4) // 256))
    got, parts, _ = _device_sumsq([g], used)
    again, parts2, _ = _device_sumsq([g], used)
    ref = _exact_sumsq(g)
    print(f"n={n}: sumsq {got!r} ref {ref!r} rel err {abs(got - ref) / ref:.3e} bound {G.sumsq_bound(n):.3e}")
    assert abs(got - ref) <= G.sumsq_bound(n) * ref
    assert torch.equal(parts, parts2) and got == again


def test_sumsq_does_not_read_an_unused_range():
    """Check 1, the three-range buffer: the middle range's module is unused (use flag 0) and full of NaNs -- it contributes 0."""
    gen = torch.Generator(device=DEV).manual_seed(9)
    buf = torch.randn(1028 + 2052 + 516, generator=gen, device=DEV)
    pieces = [buf[:1028], buf[1028:3080], buf[3080:]]
    pieces[1].fill_(math.nan)
    used = torch.tensor([1.0, 0.0, 2.0], device=DEV)
    got, parts, slots = _device_sumsq(pieces, used)
    ref = _exact_sumsq(pieces[0], pieces[2])
    assert math.isfinite(got) and abs(got - ref) <= G.sumsq_bound(1028 + 516) * ref
    assert bool((parts[slots[0]:slots[0] + slots[1]] == 0).all())
    used[1] = 1.0                                                # the same range, used: the NaNs do show
    assert math.isnan(_device_sumsq(pieces, used)[0])


def test_launchers_refuse_bad_arguments_before_any_launch():
    from myriad_amd import _lib, ops
    g = torch.zeros(1024, device=DEV)
    used, steps = torch.ones(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ws, ctl = torch.zeros(4, dtype=F64, device=DEV), torch.zeros(4, dtype=F64, device=DEV)
    L = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    bad = [lambda: ops.grad_sumsq(g[:6], used, ws),                                          # n % 4
           lambda: ops.grad_sumsq(torch.zeros(4 * 256 * 5, device=DEV), used, ws),           # 5 slots needed, 4 there
           lambda: L.mh_grad_sumsq(g.data_ptr(), 1024, None, ws.data_ptr(), 4, s),           # null pointers
           lambda: L.mh_grad_sumsq(g.data_ptr(), 1024, used.data_ptr(), None, 4, s),
           lambda: ops.clip_finalize(ws, 1, None, 0.0, 1.0, True, ctl),                      # max_norm <= 0
           lambda: ops.clip_finalize(ws, 1, None, -1.0, 1.0, True, ctl),
           lambda: L.mh_clip_finalize(ws.data_ptr(), 1, None, 0, 1.0, 1.0, 1, None, s),
           lambda: ops.adamw_gated_ctl(g[:6], g[:6], g[:6], g[:6], 1e-3, 0.0, used, steps, ctl),
           lambda: L.mh_adamw_gated_ctl(g.data_ptr(), g.data_ptr(), g.data_ptr(), g.data_ptr(), 1024, 1e-3, 0.9, 0.999, 1e-8, 0.0,
                                        used.data_ptr(), steps.data_ptr(), None, s),
           lambda: L.mh_adamw_bump_ctl(used.data_ptr(), steps.data_ptr(), 1, None, s)]
    for i, call in enumerate(bad):
        try:
            rc = call()
        except _lib.MyriadHipError as e:
            assert "MH_ERR_ARG" in str(e), (i, e)
        else:
            assert rc == -1, (i, rc)
    torch.cuda.synchronize()
    assert bool((ctl == 0).all()) and int(steps[0]) == 0 and bool((g == 0).all())


def _ctl_of(g, max_norm, grad_scale, guard):
    from myriad_amd import ops
    used = torch.ones(1, device=DEV)
    ws = torch.zeros(ops.grad_sumsq_slots(g.numel()), dtype=F64, device=DEV)
    n = ops.grad_sumsq(g, used, ws)
    ctl = torch.zeros(4, dtype=F64, device=DEV)
    ops.clip_finalize(ws, n, None, max_norm, grad_scale, guard, ctl)
    torch.cuda.synchronize()
    return ctl


N_S = 4 * 256 + 4 + 1024                                          # three blocks, the last one partial


@pytest.mark.parametrize("case,fill,max_norm,grad_scale", [
    ("clipping active", 1.0, 1.0, 1.0),
    ("clipping inactive", 1.0, 1e4, 1.0),
    ("clipping off", 1.0, None, 1.0),
    ("grad_scale 0.5, active", 1.0, 1.0, 0.5),
    ("grad_scale 0.5, inactive", 1e-3, 1.0, 0.5),
    # finite elements whose squares overflow fp32: an fp32 accumulator would call this gradient inf.  max_norm = 1e10 keeps
    # s = 1e10 / (3e38 * sqrt(n)) ~ 7e-31 a NORMAL fp32 number, so that the 2^-24 bound on its one rounding means something
    # (at max_norm = 1 it would be a denormal, which carries fewer bits by construction)
    ("3e38 elements", 3e38, 1e10, 1.0),
])
def test_the_multiplier_s(case, fill, max_norm, grad_scale):
    """Check 2: |s - s_ref| <= (2^-24 + (n + 16) * 2^-53) * s_ref; s == (float)grad_scale exactly where nothing clips; the
    norm in ctl[1] is the double norm of the averaged gradient; with finite 3e38 elements the guard applies the update, the norm
    is finite and so are the updated parameters."""
    from myriad_amd import ops
    n = N_S
    gen = torch.Generator(device=DEV).manual_seed(21)
    if fill == 3e38:
        g = torch.where(torch.rand(n, generator=gen, device=DEV) < 0.5, -1.0, 1.0) * 3e38
    else:
        g = torch.randn(n, generator=gen, device=DEV) * fill
    ctl = _ctl_of(g, max_norm, grad_scale, guard=True)
    s, norm, apply, skipped = ctl.tolist()
    sumsq = _exact_sumsq(g)
    want = G.s_ref(sumsq, max_norm, grad_scale)
    print(f"{case}: s {s!r} s_ref {want!r} rel err {abs(s - want) / want:.3e} bound {G.s_bound(n):.3e}; norm {norm!r}")
    assert abs(s - want) <= G.s_bound(n) * want
    assert s == float(torch.tensor(s, dtype=F64).float())        # fp32-representable: the kernel's cast loses nothing
    assert apply == 1.0 and skipped == 0.0
    # sqrt and the product by grad_scale add two more fp64 roundings to half the sum's relative error
    assert abs(norm - G.norm_ref(sumsq, grad_scale)) <= (G.sumsq_bound(n) + 2.0 ** -51) * G.norm_ref(sumsq, grad_scale)
    active = max_norm is not None and G.norm_ref(sumsq, grad_scale) + 1e-6 > max_norm
    assert active == ("inactive" not in case and "off" not in case)
    if not active:
        assert s == grad_scale
    if fill == 3e38:
        assert math.isfinite(norm) and norm > 3e38
        p = torch.randn(n, generator=gen, device=DEV)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        used, steps = torch.ones(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        p0 = p.clone()
        ops.adamw_gated_ctl(p, g, m, v, 1e-3, 0.05, used, steps, ctl)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(m).all()) and bool(torch.isfinite(v).all())
        assert not torch.equal(p, p0)


def _store():
    """Three modules, odd-sized tensors (padding inside the ranges), both weight-decay groups."""
    from myriad_amd.myriad import ParamStore
    from myriad_amd.networks import ve_param_specs
    specs = ([("expert_adaptor.conv1.weight", (4, 37), (4, 37)), ("expert_adaptor.conv2.weight", (37, 4), (37, 4))]
             + ve_param_specs("VETokenizer.", 8, 5) + [("VETokenizer.base_prompts", (9, 33), (9, 33))]
             + ve_param_specs("VEInstructor.", 12, 1))
    st = ParamStore(specs, DEV)
    assert len(st.modules) == 3
    gen = torch.Generator(device=DEV).manual_seed(5)
    st.flat_p.copy_(torch.randn(st.total, generator=gen, device=DEV))
    return st, gen


def _fill_grads(st, gen, scale, flags):
    """Random gradients for every parameter (the padding between them stays zero, as the backward leaves it)."""
    st.flat_g_comm.zero_()
    for name, _, _ in st.specs:
        st.g[name].copy_(torch.randn(st.g[name].shape, generator=gen, device=DEV) * scale)
    st.used.copy_(torch.tensor([flags[m] for m in st.modules], device=DEV))


def _state(st):
    torch.cuda.synchronize()
    return [t.clone() for t in (st.flat_p, st.flat_m, st.flat_v, st.steps_dev)]


def test_clipped_updates_are_float64_adamw_on_the_scaled_gradient():
    """Check 3: four steps of a three-module store through adamw_step(clip=...), VEInstructor unused in step 2, step 3 below the
    threshold.  Each step's s is read back, checked as in check 2, and the float64 torch.optim.AdamW of tests/adamw_ref.py gets
    fp32(g * s) -- the kernel's own single multiplication -- so its budgets for p, m, v and the step counts apply unchanged."""
    from myriad_amd.myriad import GradClip, module_of
    from oracle import myriad_ref as R
    from tests.adamw_ref import AdamWRef
    st, gen = _store()
    names = [n for n, _, _ in st.specs]
    sl = lambda t, n: t[st.offsets[n][0]:st.offsets[n][0] + st.offsets[n][1]]
    ref = AdamWRef([sl(st.flat_p, n) for n in names], [0.05 if R.uses_weight_decay(n, len(r)) else 0.0 for n, _, r in st.specs])
    max_norm, grad_scale = 1.0, 0.5
    lrs = [1e-3, 8e-4, 6e-4, 4e-4]
    scales = [1.0, 1.0, 1e-4, 2.0]
    want_steps = {m: 0 for m in st.modules}
    for i in range(4):
        flags = {m: 2.0 for m in st.modules}
        if i == 1:
            flags["VEInstructor"] = 0.0
        _fill_grads(st, gen, scales[i], flags)
        live = [sl(st.flat_g, n) if flags[module_of(n)] > 0 else None for n in names]
        st.adamw_step(lrs[i], 0.05, grad_scale=grad_scale, clip=GradClip(max_norm))
        stats = st.grad_stats()
        s = stats["clip_scale"]
        sumsq = G.sumsq_ref(live)
        want = G.s_ref(sumsq, max_norm, grad_scale)
        assert abs(s - want) <= G.s_bound(st.total) * want, (i, s, want)
        assert (s == grad_scale) == (i == 2) and stats["applied"] and stats["skipped_steps"] == 0
        s32 = torch.tensor(s, dtype=torch.float32, device=DEV)
        assert float(s32) == s
        ref.step([None if g is None else g * s32 for g in live], lrs[i])
        for m in st.modules:
            want_steps[m] += flags[m] > 0
        for k, n in enumerate(names):
            ref.check(k, sl(st.flat_p, n), sl(st.flat_m, n), sl(st.flat_v, n), f"step {i} {n}")
            assert ref.steps(k) == want_steps[module_of(n)]
        assert st.module_steps() == want_steps
    assert want_steps["VEInstructor"] == 3


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("bad", [math.inf, math.nan])
def test_the_guard_skips_a_non_finite_update_and_nothing_else(bad, where):
    """Check 4: one inf / NaN at the first element of the first range or the last element of the last range: p, m, v and every
    step counter keep their bits, skipped_steps grows by one, and the next clean step is the update the skipped one would have
    been (same step number: bit-equal to the plain path from the same state).  With both options off the same buffer goes
    through today's path untouched by the guard."""
    from myriad_amd.myriad import GradClip
    st, gen = _store()
    flags = {m: 1.0 for m in st.modules}
    _fill_grads(st, gen, 1.0, flags)
    st.adamw_step(1e-3, 0.05, clip=GradClip(None, True))                     # a clean step first: moments and counters non-zero
    assert st.grad_stats()["applied"] and st.grad_stats()["skipped_steps"] == 0 and st.grad_stats()["clip_scale"] == 1.0
    s0 = _state(st)
    _fill_grads(st, gen, 1.0, flags)
    clean = st.flat_g_comm.clone()
    at = st.ranges[0][1] if where == "first" else st.ranges[-1][2] - 1
    st.flat_g[at] = bad
    poisoned = st.flat_g_comm.clone()
    for k in (1, 2):                                                         # twice: the count runs on
        st.adamw_step(8e-4, 0.05, clip=GradClip(None, True))
        for a, b in zip(_state(st), s0):
            assert torch.equal(a, b)
        stats = st.grad_stats()
        assert not stats["applied"] and stats["skipped_steps"] == k and not math.isfinite(stats["grad_norm"])
    st.flat_g_comm.copy_(clean)
    st.adamw_step(8e-4, 0.05, clip=GradClip(None, True))
    got = _state(st)
    assert st.grad_stats()["applied"] and st.grad_stats()["skipped_steps"] == 2
    # the plain path from the same state
    plain, _ = _store()
    for dst, src in zip((plain.flat_p, plain.flat_m, plain.flat_v, plain.steps_dev), s0):
        dst.copy_(src)
    plain.flat_g_comm.copy_(clean)
    plain.adamw_step(8e-4, 0.05)
    for name, a, b in zip("pmvs", got, _state(plain)):
        assert torch.equal(a, b), name
    assert not torch.equal(got[0], s0[0]) and bool((got[3] == s0[3] + 1).all())
    # opt-in: without the options the poisoned buffer reaches the parameters, as before
    plain.flat_g_comm.copy_(poisoned)
    plain.adamw_step(8e-4, 0.05)
    torch.cuda.synchronize()
    assert plain.ctl is None and not bool(torch.isfinite(plain.flat_p[at]))
    assert bool((plain.steps_dev == s0[3] + 2).all())


# ---- the model's step (the small model of tests/dp_common.py)
STAGES = [1, 2, 0]                                               # step 1 (stage 2): the tokenizer is unused
SEED = 11


def _train(monkeypatch, early_env, spy_names=(), **opts):
    """Three train_steps with look-ahead; -> (snapshot, {spied name: calls}, grad_stats per step)."""
    from myriad_amd import ops
    from tests import dp_common as C
    if early_env is not None:
        monkeypatch.setenv("MYRIAD_EARLY_ADAMW", early_env)
    m, cfg = C.build_model(DEV)
    m.lora.base_seed = SEED
    calls = {}

    def spy(owner, name):
        real = getattr(owner, name)
        calls[name] = 0

        def wrapped(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        monkeypatch.setattr(owner, name, wrapped)
    spy(m.store, "adamw_module")
    for name in spy_names:
        spy(ops, name)
    stats = []
    for i in range(3):
        m.fixed_stage = STAGES[i]
        nxt = C.batch(0, i + 1, cfg["vocab"], DEV) if i < 2 else None
        m.train_step(C.batch(0, i, cfg["vocab"], DEV), C.LRS[i], 0.05, next_samples=nxt, **opts)
        stats.append(m.grad_stats())
    m.finish_update()
    return C.snapshot(m), dict(calls), stats


CTL_OPS = ("grad_sumsq", "clip_rank_sum", "clip_finalize", "adamw_gated_ctl", "adamw_bump_ctl")


@pytest.fixture(scope="module")
def plain_run():
    """Three steps with both options off (the early tokenizer update on, as by default), spied on."""
    mp = pytest.MonkeyPatch()
    try:
        return _train(mp, None, spy_names=("adamw_gated",) + CTL_OPS)
    finally:
        mp.undo()                                                # the spies count this run only


def test_clipping_keeps_every_update_behind_the_norm(monkeypatch, plain_run):
    """Check 5: with max_grad_norm the tokenizer is not updated from inside the backward (no adamw_module call; the plain run
    does make them), and three steps equal, bit for bit, backward -> norm over every range -> finalise -> _ctl update by hand."""
    from myriad_amd import ops
    from tests import dp_common as C
    max_norm = 1e-2
    got, calls, stats = _train(monkeypatch, None, max_grad_norm=max_norm)
    assert calls["adamw_module"] == 0 and plain_run[1]["adamw_module"] == 2          # stages 1 and 0 use the tokenizer
    assert all(s["applied"] and s["clip_scale"] < 1.0 and s["grad_norm"] > max_norm for s in stats), stats
    ref, cfg = C.build_model(DEV)
    ref.lora.base_seed = SEED
    st = ref.store
    ctl = torch.zeros(4, dtype=F64, device=DEV)
    ws = torch.zeros(sum(ops.grad_sumsq_slots(b - a) for _, a, b, _ in st.ranges), dtype=F64, device=DEV)
    for i in range(3):
        ref.fixed_stage = STAGES[i]
        with torch.no_grad():
            ref._forward_impl(C.batch(0, i, cfg["vocab"], DEV), True)
            ref.backward()
        off = 0
        for mi, a, b, _ in st.ranges:
            off += ops.grad_sumsq(st.flat_g[a:b], st.used[mi:mi + 1], ws[off:])
        ops.clip_finalize(ws, off, None, max_norm, 1.0, False, ctl)
        for mi, a, b, decays in st.ranges:
            ops.adamw_gated_ctl(st.flat_p[a:b], st.flat_g[a:b], st.flat_m[a:b], st.flat_v[a:b], C.LRS[i], 0.05 if decays else 0.0,
                                st.used[mi:mi + 1], st.steps_dev[mi:mi + 1], ctl)
        ops.adamw_bump_ctl(st.used, st.steps_dev, ctl)
        torch.cuda.synchronize()
        assert ctl.tolist()[:2] == [stats[i]["clip_scale"], stats[i]["grad_norm"]]
    want = C.snapshot(ref)
    for k in ("p", "m", "v"):
        assert torch.equal(got[k], want[k]), k
    assert got["steps"] == want["steps"] and got["steps"]["VETokenizer"] == 2
    assert not torch.equal(got["p"], plain_run[0]["p"])                              # and clipping did change the run


def test_a_neutral_clip_and_the_off_path_change_nothing(monkeypatch, plain_run):
    """Check 6: max_grad_norm = 1e30 (s == grad_scale exactly) with the update at the tail gives p, m, v and step counts bit-equal
    to the run with both options off; and that run launches ops.adamw_gated and none of the clipping entries."""
    got, calls, stats = _train(monkeypatch, "0", max_grad_norm=1e30, skip_nonfinite=True)
    assert all(s["clip_scale"] == 1.0 and s["applied"] and s["skipped_steps"] == 0 for s in stats)
    off, off_calls, off_stats = plain_run
    for k in ("p", "m", "v"):
        assert torch.equal(got[k], off[k]), k
    assert got["steps"] == off["steps"]
    assert off_calls["adamw_gated"] > 0 and all(off_calls[n] == 0 for n in CTL_OPS), off_calls
    assert all(s["grad_norm"] is None for s in off_stats)
