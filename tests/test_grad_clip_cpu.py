"""Host side of gradient-norm clipping and the non-finite guard: the float64 rule against torch.nn.utils.clip_grad_norm_, the list
of normed pieces against brute-force element sets, and the runner's two config keys."""
import math

import numpy as np
import pytest
import torch

from tests import grad_clip_ref as G


def _pieces(seed, sizes, scale):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) * scale for n in sizes]


@pytest.mark.parametrize("case,scale,max_norm,grad_scale,unused", [
    ("clipping active", 3.0, 1.0, 1.0, ()),
    ("clipping inactive", 1e-3, 1.0, 0.5, ()),
    ("an unused piece (grad None)", 3.0, 0.7, 0.5, (1,)),
])
def test_s_ref_is_clip_grad_norm_in_float64(case, scale, max_norm, grad_scale, unused):
    raw = _pieces(3, [37, 1024, 5], scale)
    for i in unused:
        raw[i][:3] = 1e4                                         # were an unused piece counted, the norm would show it
    live = [None if i in unused else g for i, g in enumerate(raw)]
    params = [torch.nn.Parameter(torch.zeros(g.numel(), dtype=torch.float64)) for g in raw]
    for prm, g in zip(params, live):
        prm.grad = None if g is None else g.double() * grad_scale      # the optimiser's gradient: the rank average
    total = torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2.0)
    sumsq = G.sumsq_ref(live)
    assert float(total) == pytest.approx(G.norm_ref(sumsq, grad_scale), rel=1e-14)
    s = G.s_ref(sumsq, max_norm, grad_scale)
    active = G.norm_ref(sumsq, grad_scale) + 1e-6 > max_norm
    assert active == (case == "clipping active" or bool(unused))
    if not active:
        assert s == grad_scale                                   # the clamp to 1: exactly the plain average
    for prm, g in zip(params, live):
        if g is None:
            assert prm.grad is None
        else:
            torch.testing.assert_close(prm.grad, g.double() * s, rtol=1e-14, atol=0.0)
    assert G.s_ref(sumsq, None, grad_scale) == grad_scale


def _brute(ranges, total, shard, exclude, skip_idx):
    """Per element of the buffer: 2 * module index + decays if the update touches it, else -1 -- from one membership mask per
    condition, with no interval arithmetic."""
    e = np.arange(total)
    inside = lambda spans: np.logical_or.reduce([(lo <= e) & (e < hi) for lo, hi in spans] or [np.zeros(total, bool)])
    label = np.full(total, -1)
    for mi, a, b, d in ranges:
        if mi not in skip_idx:
            label[(a <= e) & (e < b)] = 2 * mi + int(d)
    if shard is not None:
        label[~inside(shard)] = -1
    label[inside(exclude)] = -1
    return label


def _painted(pieces, total):
    label = np.full(total, -1)
    for mi, a, b, d in pieces:
        assert a < b and a % 4 == 0 and b % 4 == 0
        assert (label[a:b] == -1).all()                          # no element twice
        label[a:b] = 2 * mi + int(d)
    return label


@pytest.mark.parametrize("world", [1, 2, 4])
def test_update_pieces_are_the_brute_force_element_sets(world):
    """The pieces adamw_step norms and updates for (ranges, shard, exclude, skip) are exactly the elements a per-element walk
    finds -- per rank with a segmented buffer ('rs_ag' shards from DataParallel itself), and over all ranks together every
    element of every module range exactly once."""
    from myriad_amd.lora import lora_param_specs
    from myriad_amd.myriad import ParamStore, update_pieces
    from myriad_amd.networks import ve_param_specs
    from myriad_amd.runner import DataParallel
    specs = ([("expert_adaptor.conv1.weight", (4, 37), (4, 37)), ("expert_adaptor.conv2.weight", (37, 4), (37, 4))]
             + ve_param_specs("VETokenizer.", 8, 5) + [("VETokenizer.base_prompts", (9, 33), (9, 33))]
             + ve_param_specs("VEInstructor.", 12, 1) + lora_param_specs(2, 36, 3))
    st = ParamStore(specs, "cpu")
    ta, tb = st.module_range("VETokenizer", True)
    cuts = [(ta + 31) // 32 * 32, tb // 32 * 32]                 # the exchange cut at the tokenizer's run, as _dp_segment does
    seen = []
    for rank in range(world):
        dp = DataParallel(device=None, mode="rs_ag")
        dp.world, dp.rank = world, rank
        dp.set_segments(st.total, cuts)
        shard = dp.shards(st.total) if world > 1 else None
        segs = dp.segments(st.total)
        assert len(segs) == 3
        for exclude, skip_idx in (((), ()), ([segs[1]], ()), ((), {st.modules.index("VETokenizer")}),
                                  ([(ta + 8, ta + 24), (ta + 100, tb + 4)], {0})):
            got = _painted(update_pieces(st.ranges, shard, exclude, skip_idx), st.total)
            assert (got == _brute(st.ranges, st.total, shard, exclude, skip_idx)).all(), (rank, exclude, skip_idx)
        seen.extend(update_pieces(st.ranges, shard))
    assert (_painted(seen, st.total) == _brute(st.ranges, st.total, None, (), ())).all()


def test_grad_clip_of_turns_both_options_off_into_none():
    from myriad_amd.myriad import GradClip
    assert GradClip.of(None, False) is None and GradClip.of(0.0, False) is None and GradClip.of(-1.0, False) is None
    c = GradClip.of(0, True)
    assert c.max_norm is None and c.skip_nonfinite and c.rank_sums is None
    c = GradClip.of(2.5)
    assert c.max_norm == 2.5 and not c.skip_nonfinite
    with pytest.raises(ValueError):
        GradClip(0.0)
    with pytest.raises(ValueError):
        GradClip(math.nan)


@pytest.mark.parametrize("run,want", [
    ({}, (None, False)), ({"max_grad_norm": 0}, (None, False)), ({"max_grad_norm": -1.0}, (None, False)),
    ({"max_grad_norm": 1.0}, (1.0, False)), ({"max_grad_norm": "0.5", "skip_nonfinite_grad": True}, (0.5, True)),
    ({"skip_nonfinite_grad": True}, (None, True)),
])
def test_runner_reads_the_two_config_keys(run, want, tmp_path):
    """run.max_grad_norm (absent, 0 or negative = off) and run.skip_nonfinite_grad reach every train_step; with both off the
    runner passes neither argument and logs no gradient statistics."""
    from myriad_amd.runner import RunnerBase, grad_clip_options
    assert grad_clip_options(run) == want

    class Cfg:
        run_cfg = dict(run, output_dir=str(tmp_path), iters_per_epoch=3, log_freq=2)

    class Model:
        def __init__(self):
            self.calls, self.stats_calls = [], 0

        def train(self, mode=True):
            return self

        def train_step(self, samples, lr, weight_decay=0.05, **kw):
            self.calls.append(kw)
            return torch.tensor(1.0)

        def finish_update(self):
            pass

        def grad_stats(self):
            self.stats_calls += 1
            return {"grad_norm": 3.25, "clip_scale": 0.5, "applied": True, "skipped_steps": 2}

    class Loader:
        def __len__(self):
            return 3

        def __next__(self):
            return {}

    class Sched:
        def step(self, cur_epoch, cur_step):
            return 1e-4

    model = Model()
    runner = RunnerBase(Cfg(), "job", model, {"ds": None}, device="cpu")
    assert (runner.max_grad_norm, runner.skip_nonfinite_grad) == want
    runner._sched, runner._loader = Sched(), Loader()
    stats = runner.train_epoch(0)
    assert len(model.calls) == 3
    if want == (None, False):
        assert all("max_grad_norm" not in kw and "skip_nonfinite" not in kw for kw in model.calls)
        assert model.stats_calls == 0 and set(stats) == {"lr", "loss"}
    else:
        assert all((kw["max_grad_norm"], kw["skip_nonfinite"]) == want for kw in model.calls)
        assert stats["grad_norm"] == "3.250" and stats["skipped_steps"] == 2
