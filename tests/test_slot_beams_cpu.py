"""Beam search in the decode slots, the host side without a device: BeamItem (one request's search) against the oracle
tests/beam_ref.beam_search on a scripted logits function, and BeamSlotScheduler under a scripted step."""
import numpy as np
import pytest
import torch

from myriad_amd.decode_host import BeamItem, BeamSlotScheduler, RefillPlanner
from tests import beam_ref

V, EOS, X1, X2 = 64, 2, 11, 12
STOPS = ((X1, X2),)


def _logits_fn(seed):
    """next-token logits as a pure function of (item, generated ids): random rows, with EOS, the two-token stop and a long path
    pushed up at fixed depths so that hypotheses finish at different lengths and by different rules"""
    def fn(prefixes):
        rows = []
        for item, pre in prefixes:
            g = torch.Generator().manual_seed(seed * 7919 + item * 104729 + sum((i + 1) * (t + 3) for i, t in enumerate(pre)) * 31 + len(pre))
            x = torch.randn(V, generator=g) * 2.0
            if len(pre) >= 2:
                x[EOS] += 3.0
            if len(pre) == 1:
                x[X1] += 3.5
            if pre and pre[-1] == X1:
                x[X2] += 5.0
            rows.append(x)
        return torch.stack(rows)
    return fn


def _drive(fn, item_no, nb, max_new, min_length, lp, es, nrs):
    """BeamItem fed what a device step records: per step the top K of running score + log_softmax over the item's rows (the first
    step over one row, the prompt's), EOS banned while gen < min_length, ties to the lower flat index."""
    item = BeamItem(nb, V, max_new, STOPS, EOS, lp, es, nrs)
    K = 2 * nb
    seqs, run = [()], torch.zeros(1)
    steps = 0
    while True:
        logp = torch.log_softmax(fn([(item_no, s) for s in seqs]).float(), -1)
        if steps < min_length:
            logp[:, EOS] = float("-inf")
        acc = (logp + run[:, None]).reshape(-1)
        sel = torch.sort(acc, descending=True, stable=True)[1][:K]
        ids, src, sc, going = item.select(acc[sel].numpy(), sel.numpy())
        steps += 1
        assert len(ids) == len(src) == len(sc) == nb and all(0 <= int(p) < len(seqs) for p in src)
        seqs = [seqs[int(p)] + (int(t),) for p, t in zip(src, ids)]
        assert seqs == item.run_seqs                                 # the rows' (ids, src) rebuild the running hypotheses
        run = torch.from_numpy(np.asarray(sc, dtype=np.float32).copy())
        if not going:
            return item, steps


@pytest.mark.parametrize("es", [False, True, "never"])
@pytest.mark.parametrize("lp", [0.0, 1.0])
@pytest.mark.parametrize("nb", [2, 4])
def test_beam_item_is_the_oracles_search(nb, lp, es):
    two_token_stop = False
    for seed in range(6):
        for min_length, nrs, max_new in ((1, 1, 7), (0, nb, 5), (3, 2, 9)):
            fn = _logits_fn(seed)
            want_ids, want_sc, tr = beam_ref.beam_search(fn, 1, nb, max_new, EOS, min_length=min_length, length_penalty=lp,
                                                         early_stopping=es, num_return_sequences=nrs, stop_seqs=STOPS,
                                                         return_trace=True)
            item, steps = _drive(fn, 0, nb, max_new, min_length, lp, es, nrs)
            seqs, scores = item.result()
            assert steps == len(tr["trace"]) and item.gen == steps
            assert [len(s) for s in seqs] == tr["lengths"]
            for r, s in enumerate(seqs):                             # sequences and their order
                assert list(s) == want_ids[r, :len(s)].tolist()
                two_token_stop |= len(s) >= 2 and tuple(s[-2:]) == STOPS[0]
            assert scores.dtype == np.float32 and np.array_equal(scores, want_sc.numpy())      # exact: the same f32 arithmetic
            assert item.finished == tr["finished"]
    assert two_token_stop                                            # some returned hypothesis ended on the two-token stop


def test_beam_item_refuses_bad_arguments():
    for kw in (dict(num_beams=0), dict(num_beams=2, vocab=3), dict(num_return_sequences=3), dict(early_stopping="yes"),
               dict(max_new_tokens=0)):
        with pytest.raises(ValueError):
            BeamItem(**dict(dict(num_beams=2, vocab=V, max_new_tokens=4), **kw))


class _ScriptedItem:
    """ends after `n` selections; feeds its index back so the test can see whose feed a group holds"""

    def __init__(self, index, n):
        self.index, self.n, self.gen, self.finished = index, n, 0, 0

    def select(self, top_s, top_i):
        self.gen += 1
        going = self.gen < self.n
        self.finished = 0 if going else 2
        return [self.index] * 2, [0, 1], [float(top_s[0])] * 2, going

    def result(self):
        return [(self.index,) * self.gen], np.array([float(self.gen)], dtype=np.float32)


def _scripted_run(lengths, groups, ordered):
    made = iter(range(len(lengths)))

    def make_item():
        i = next(made)
        return _ScriptedItem(i, lengths[i])

    sched = BeamSlotScheduler(groups, make_item, ordered=ordered)
    plan = RefillPlanner(sched, range(len(lengths)), length=lambda i: 8)
    out, admissions, live_log = [], [], []
    while True:
        group = plan.next_pass()
        while group:
            for g, i in group:
                admissions.append((g, i))
                if sched.admit(g, [0.5], [0]):
                    assert sched.feed[g][0] == [i, i]
            group = plan.next_pass()
        out += sched.pop()
        if not sched.live():
            break
        live_log.append(sched.live())
        fin = sched.step([[1.0]] * groups, [[0]] * groups)
        assert all(sched.rows[g] is None and sched.feed[g] is None for g in fin)
        out += sched.pop()
    return sched, out, admissions, live_log


def test_scheduler_admits_in_order_reuses_groups_and_counts_occupancy():
    #          request:  0  1  2  3  4  5
    lengths = [3, 1, 2, 4, 1, 2]                                     # 1 and 4 end at their first selection
    sched, out, adm, live_log = _scripted_run(lengths, 2, ordered=False)
    # 0 -> group 0; 1 ends at once in group 1, which takes 2 at the same refill point; 2 ends first and its group takes 3; ...
    assert adm == [(0, 0), (1, 1), (1, 2), (1, 3), (0, 4), (0, 5)]
    assert [o[0] for o in out] == [1, 2, 0, 4, 5, 3]                 # completion order
    assert live_log == [[0, 1], [0, 1], [0, 1], [1]]
    assert sched.steps == 4 and sched.live_row_steps == 7 and sched.occupancy == 7 / 8
    assert sched.admitted == 6 and sched.finished_hypotheses == 12
    for index, seqs, scores in out:
        assert seqs == [(index,) * lengths[index]] and scores.tolist() == [float(lengths[index])]
    with pytest.raises(ValueError):
        BeamSlotScheduler(0, lambda: None)


def test_scheduler_ordered_holds_results_back_and_a_busy_group_refuses():
    lengths = [3, 1, 2, 4, 1, 2]
    sched, out, _, _ = _scripted_run(lengths, 2, ordered=True)
    assert [o[0] for o in out] == [0, 1, 2, 3, 4, 5]
    one = BeamSlotScheduler(3, lambda: _ScriptedItem(0, 2))
    assert one.free() == [0, 1, 2] and one.live() == [] and one.occupancy == 0.0
    assert one.admit(1, [0.0], [0])
    with pytest.raises(ValueError):
        one.admit(1, [0.0], [0])
    assert one.free() == [0, 2] and one.live() == [1]
    assert one.step([[0.0]] * 3, [[0]] * 3) == [1]                   # an idle group's entries are ignored
    assert one.occupancy == 1 / 3 and one.free() == [0, 1, 2]
