"""The per-request seeds of a device-sampled decode-slot run (myriad_amd.llama.seeded_requests), driven on the CPU by RefillPlanner
and a scripted scheduler: request i gets the i-th seed whatever the slot count and the refill settings are."""
import pytest
import torch

from myriad_amd.llama import RefillPlanner, SlotScheduler, seeded_requests

LENGTHS = [5, 23, 9, 14, 7, 18, 11, 30, 4, 12, 6]
NEW = [3, 1, 6, 2, 6, 4, 1, 5, 2, 6, 3]                     # tokens request i generates (1: it ends on its first pick)
MAX_NEW = 6


def _drive(slots, prefill_batch, refill_min, **seed_kw):
    """SlotDecoder.run's loop with scripted picks: returns {request index: seed} in the order the requests were admitted."""
    sched = SlotScheduler(slots, MAX_NEW, eos_id=2)
    reqs = seeded_requests(range(len(LENGTHS)), **seed_kw)
    plan = RefillPlanner(sched, reqs, prefill_batch, 2048, refill_min, length=lambda q: LENGTHS[q[0]])
    owner, got = {}, {}
    ids_of = lambda i: [7] * (NEW[i] - 1) + [2 if NEW[i] < MAX_NEW else 7]      # noqa: E731  EOS ends it, or max_new_tokens does
    while True:
        group = plan.next_pass()
        while group:
            for s, (i, seed) in group:
                assert sched.admitted == i                           # admission in input order
                got[i] = seed
                if sched.admit(s, ids_of(i)[0], 0.0):
                    owner[s] = [i, 1]
            group = plan.next_pass()
        live = sched.live()
        if not live:
            return got
        picks = [0] * slots
        for s in live:
            picks[s] = ids_of(owner[s][0])[owner[s][1]]
            owner[s][1] += 1
        sched.step(picks, [0.0] * slots)


def test_every_request_gets_the_same_seed_whatever_the_slots_and_the_refills_are():
    g = torch.Generator().manual_seed(17)
    want = [int(torch.randint(0, 2**63 - 1, (1,), generator=g)) for _ in LENGTHS]   # greedy_generate's draw, once per request
    assert len(set(want)) == len(want)
    for slots in (1, 4, 8):
        for prefill_batch, refill_min in ((1, 1), (4, 1), (4, 2)):
            got = _drive(slots, prefill_batch, refill_min, generator=torch.Generator().manual_seed(17))
            assert [got[i] for i in range(len(LENGTHS))] == want, (slots, prefill_batch, refill_min)


def test_explicit_seeds_replace_the_draws_and_leave_the_generator_alone():
    g = torch.Generator().manual_seed(17)
    before = g.get_state()
    seeds = [1000 + 3 * i for i in range(len(LENGTHS))]
    for slots, prefill_batch, refill_min in ((1, 1, 1), (4, 4, 2), (8, 4, 1)):
        got = _drive(slots, prefill_batch, refill_min, generator=g, seeds=iter(seeds))
        assert [got[i] for i in range(len(LENGTHS))] == seeds
    assert torch.equal(g.get_state(), before)
    with pytest.raises(ValueError, match="fewer seeds"):
        _drive(4, 1, 1, seeds=seeds[:4])
    for bad in (-1, 2**63):
        with pytest.raises(ValueError, match="outside"):
            list(seeded_requests([0], seeds=[bad]))
