"""Beam sampling in the decode slots' beam groups, the parts that need no device: the seeds that travel with the requests through
RefillPlanner into BeamSlotScheduler, the host rule at item 0, the two new entries of the C ABI and the evaluation script's flags.

The first two tests pin ground the sampled beam slots stand on and that was there before them (seeded_requests, RefillPlanner and
beam_sample_select(item=0) are unchanged): they pass without the feature.  The last two need it."""
import inspect

import numpy as np
import pytest
import torch

from myriad_amd import _lib, ops
from myriad_amd.decode_host import BeamSlotScheduler, RefillPlanner, beam_sample_select, seeded_requests
from tests import beam_sample_ref as BR


class _Countdown:
    """A stand-in for BeamItem: the search of a request goes on for `life` selections."""

    def __init__(self, life):
        self.life, self.gen, self.finished = life, 0, 1

    def select(self, top_s, top_i):
        self.gen += 1
        return np.zeros(2, np.int64), np.zeros(2, np.int64), np.zeros(2, np.float32), self.gen < self.life

    def result(self):
        return [(self.gen,)], np.zeros(1, np.float32)


def _drive(n, G, prefill_batch, refill_min, **seed_kw):
    """The slot loop of SlotDecoder._run_beams on plain values: {request index: the seed it was admitted with}."""
    lives = [1 + (3 * i) % 5 for i in range(n)]                     # request i ends after lives[i] selections (1: at its refill)
    made = iter(lives)
    sched = BeamSlotScheduler(G, lambda: _Countdown(next(made)), ordered=False)
    reqs = seeded_requests(((i, 5 + 7 * i) for i in range(n)), **seed_kw)
    plan = RefillPlanner(sched, reqs, prefill_batch, 2048, refill_min, length=lambda q: q[0][1])
    seen, done = {}, []
    while True:
        group = plan.next_pass()
        while group:
            for g, ((i, _), seed) in group:
                assert sched.admitted == i                          # admission in input order
                seen[i] = seed
                sched.admit(g, None, None)
            group = plan.next_pass()
        done += [d[0] for d in sched.pop()]
        if not sched.live():
            break
        sched.step([None] * G, [None] * G)
        done += [d[0] for d in sched.pop()]
    assert sorted(done) == list(range(n))
    return seen, plan.passes


@pytest.mark.parametrize("prefill_batch,refill_min", [(1, 1), (2, 1), (3, 2), (4, 4)])
def test_request_i_takes_the_ith_seed_whatever_the_refill_settings(prefill_batch, refill_min):
    n, G = 11, 3
    g = torch.Generator().manual_seed(77)
    want = [int(torch.randint(0, 2**63 - 1, (1,), generator=g)) for _ in range(n)]
    got, passes = _drive(n, G, prefill_batch, refill_min, generator=torch.Generator().manual_seed(77))
    assert [got[i] for i in range(n)] == want
    assert passes == n if prefill_batch == 1 else passes < n
    untouched = torch.Generator().manual_seed(5)
    state = untouched.get_state().clone()
    given = list(range(100, 100 + n))
    got, _ = _drive(n, G, prefill_batch, refill_min, generator=untouched, seeds=given)
    assert [got[i] for i in range(n)] == given and torch.equal(untouched.get_state(), state)
    with pytest.raises(ValueError):
        _drive(n, G, prefill_batch, refill_min, seeds=given[:-1])


def test_the_host_rule_at_item_0_is_the_rule_of_the_request_alone():
    """What the engine hands the host for a flagged group -- the group's rows, its seed, its t and item = 0 -- is the reference's
    step for those rows alone (B = 1), whichever group holds the request: the group index is no argument of it, and the item
    field does matter (as item 2 of a batch the same rows draw something else)."""
    nb, V, seed, t = 3, 64, 2**45 + 9, 4
    g = torch.Generator().manual_seed(12)
    x, scores = torch.randn(nb, V, generator=g) * 2.0, -torch.rand(nb, generator=g)
    seen = [[1, 5], [], [7]]
    args = (-1, float(np.float32(1.0 / 0.8)), 20, 0.9, 1.2, seed, t)
    assert "group" not in inspect.signature(beam_sample_select).parameters
    acc, flat, key = beam_sample_select(x.numpy(), scores.numpy(), seen, *args, 0)
    ref = BR.step(x, scores, seen, 1, nb, *args)[0]
    assert flat.tolist() == ref.sel_flat
    tol = BR.TOL * np.maximum(1.0, np.abs(np.array(ref.sel_key, dtype=np.float64)))
    assert np.all(np.abs(key - np.array(ref.sel_key)) <= tol) and np.all(np.abs(acc - np.array(ref.sel_acc)) <= tol)
    moved = BR.step(x, scores, seen, 1, nb, *args, item0=2)[0]
    _, flat2, _ = beam_sample_select(x.numpy(), scores.numpy(), seen, *args, 2)
    assert flat2.tolist() == moved.sel_flat and flat2.tolist() != flat.tolist()


def test_the_items_entries_are_declared_and_wrapped():
    sig = _lib.signatures()
    assert len(sig["mh_beam_sample_topk_items"][1]) == 25 and len(sig["mh_beam_seen_update_items"][1]) == 8
    assert len(sig["mh_beam_sample_topk"][1]) == 25 and len(sig["mh_beam_seen_update"][1]) == 7      # the batch forms as they were
    p = inspect.signature(ops.beam_sample_topk_items).parameters
    assert [k for k in ("live", "gen", "bprm", "seed", "seen", "pos", "kvlen", "t_add") if k not in p] == []
    assert list(inspect.signature(ops.beam_seen_update_items).parameters)[-1] == "live"
    with pytest.raises(_lib.MyriadHipError):                         # the wrappers' checks come before the library is loaded
        ops.beam_seen_update_items(torch.zeros(4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.long),
                                   1, 2, 64, torch.ones(1, dtype=torch.int32))


def test_eval_flags_keep_or_drop_the_scripts_sampling():
    import eval_aqa
    a = eval_aqa.parse_args(["--cfg-path", "x.yaml", "--num-beams", "4", "--beam-sample", "--repetition-penalty", "1.05"])
    assert a.beam_sample and a.num_beams == 4 and a.repetition_penalty == 1.05
    a = eval_aqa.parse_args(["--cfg-path", "x.yaml", "--num-beams", "4"])
    assert not a.beam_sample and a.repetition_penalty == 1.0         # the default stays deterministic beams
    with pytest.raises(SystemExit):
        eval_aqa.parse_args(["--cfg-path", "x.yaml", "--beam-sample"])
    with pytest.raises(SystemExit):                                  # the penalty is forwarded under beams only
        eval_aqa.parse_args(["--cfg-path", "x.yaml", "--repetition-penalty", "1.05"])
