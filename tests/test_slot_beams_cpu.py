"""Beam search's host side without a device: BeamItem (one request's search) alone and B of them under beam_batch_going (as
beam_generate drives them) against the oracle tests/beam_ref.beam_search on a scripted logits function, and BeamSlotScheduler
under a scripted step."""
import functools

import numpy as np
import pytest
import torch

from myriad_amd.decode_host import BeamItem, BeamSlotScheduler, RefillPlanner, beam_batch_going
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


def _record(fn, item_no, seqs, run, K, ban):
    """What a device step records for one item: the top K of running score + log_softmax over its rows (the first step over one
    row, the prompt's), EOS banned with `ban`, ties to the lower flat index."""
    logp = torch.log_softmax(fn([(item_no, s) for s in seqs]).float(), -1)
    if ban:
        logp[:, EOS] = float("-inf")
    acc = (logp + run[:, None]).reshape(-1)
    sel = torch.sort(acc, descending=True, stable=True)[1][:K]
    return acc[sel].numpy(), sel.numpy()


def _drive(fn, item_no, nb, max_new, min_length, lp, es, nrs):
    """BeamItem fed what a device step records (_record), EOS banned while gen < min_length."""
    item = BeamItem(nb, V, max_new, STOPS, EOS, lp, es, nrs)
    seqs, run = [()], torch.zeros(1)
    steps = 0
    while True:
        ids, src, sc, going = item.select(*_record(fn, item_no, seqs, run, 2 * nb, steps < min_length))
        steps += 1
        assert len(ids) == len(src) == len(sc) == nb and all(0 <= int(p) < len(seqs) for p in src)
        seqs = [seqs[int(p)] + (int(t),) for p, t in zip(src, ids)]
        assert seqs == item.run_seqs                                 # the rows' (ids, src) rebuild the running hypotheses
        run = torch.from_numpy(np.asarray(sc, dtype=np.float32).copy())
        if not going:
            return item, steps


def _drive_batch(fn, B, nb, max_new, min_length, lp, es, nrs):
    """B BeamItems in lockstep, as beam_generate drives them: every item is selected every step, whatever its own `going` said,
    and beam_batch_going ends the loop.  Returns (items, steps, per step every item's own `going`)."""
    items = [BeamItem(nb, V, max_new, STOPS, EOS, lp, es, nrs) for _ in range(B)]
    seqs, run = [[()] for _ in range(B)], [torch.zeros(1) for _ in range(B)]
    own = []
    while True:
        own.append([])
        for b, item in enumerate(items):
            ids, src, sc, going = item.select(*_record(fn, b, seqs[b], run[b], 2 * nb, len(own) - 1 < min_length))
            seqs[b] = [seqs[b][int(p)] + (int(t),) for p, t in zip(src, ids)]
            assert seqs[b] == item.run_seqs
            run[b] = torch.from_numpy(np.asarray(sc, dtype=np.float32).copy())
            own[-1].append(going)
        if not beam_batch_going(items):
            return items, len(own), own


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


@functools.lru_cache(maxsize=None)
def _batch_cases(nb, lp, es, B=3):
    """The batch driver and the oracle on every (seed, triple) of one parameter set, computed once:
    [(items, steps, own, oracle ids, oracle scores, oracle trace)]."""
    out = []
    for seed in range(6):
        for min_length, nrs, max_new in ((1, 1, 7), (0, nb, 5), (3, 2, 9)):
            fn = _logits_fn(seed)
            want = beam_ref.beam_search(fn, B, nb, max_new, EOS, min_length=min_length, length_penalty=lp, early_stopping=es,
                                        num_return_sequences=nrs, stop_seqs=STOPS, return_trace=True)
            out.append(_drive_batch(fn, B, nb, max_new, min_length, lp, es, nrs) + want)
    return out


_BATCH_PARAMS = [(nb, lp, es) for es in (False, True, "never") for lp in (0.0, 1.0) for nb in (2, 4)]


@pytest.mark.parametrize("nb,lp,es", _BATCH_PARAMS)
def test_a_batch_of_beam_items_is_the_oracles_batch_search(nb, lp, es):
    for items, steps, _, want_ids, want_sc, tr in _batch_cases(nb, lp, es):
        assert steps == len(tr["trace"]) and all(item.gen == steps for item in items)
        results = [item.result() for item in items]
        seqs = [s for ss, _ in results for s in ss]                  # batch-major, each item's best first
        assert [len(s) for s in seqs] == tr["lengths"]
        for r, s in enumerate(seqs):                                 # sequences and their order
            assert list(s) == want_ids[r, :len(s)].tolist()
        scores = np.concatenate([sc for _, sc in results])
        assert scores.dtype == np.float32 and np.array_equal(scores, want_sc.numpy())          # exact: the same f32 arithmetic
        assert sum(item.finished for item in items) == tr["finished"]


def test_the_batch_cases_hold_items_that_end_before_their_batch():
    """Some item's own `going` turned False at an earlier step than its batch ended: the cases above select such items on."""
    assert any(not g for p in _BATCH_PARAMS for _, _, own, *_ in _batch_cases(*p) for step in own[:-1] for g in step)


def test_the_batch_goes_on_where_no_item_would_alone():
    """beam_batch_going against any(own going), on a scripted two-item record sequence (the logits function above never makes
    the two differ).  nb = 2, early_stopping "never", lp = 1, max_new_tokens 8, stops (3,) and (4,).  Item 0 stays `unsat` while
    all its candidates stop: after step 1 one of its rows is a stopped hypothesis at -1e9, and steps 2 and 3 record that row's
    three stopping children and the other row's EOS, all at -1e9 (as if the live row's log-probs had collapsed): the best two
    enter the pool at -1e9 / len, which the best running score, -2e9 / 8, beats.  Item 1 fills its pool at step 1 with scores
    no running beam can beat (not `unsat`) and has live candidates until step 3."""
    NEG = np.float32(-1.0e9)
    items = [BeamItem(2, V, 8, ((3,), (4,)), EOS, 1.0, "never", 2) for _ in range(2)]
    script = [(([-0.5, -1.0, -1.5, -2.0], [5, 3, 2, 4]), ([-0.1, -0.2, -3.0, -3.5], [3, 4, 5, 6])),
              (([NEG] * 4, [V + 2, V + 3, V + 4, 2]), ([-4.0, -4.5, -5.0, -5.5], [5, 6, V + 5, V + 6])),
              (([NEG] * 4, [V + 2, V + 3, V + 4, 2]), ([-4.1, -4.6, -5.1, -5.6], [3, 4, V + 3, V + 4]))]
    seen = []
    for step in script:
        own = [item.select(*rec)[3] for item, rec in zip(items, step)]
        seen.append((own, beam_batch_going(items), [item.unsat for item in items], [item.all_hit for item in items],
                     items[0].fin_scores.copy()))
    assert seen[0][:4] == ([True, False], True, [True, False], [False, False])
    assert seen[1][:4] == ([False, False], True, [True, False], [True, False])       # each clause through another item
    assert seen[2][:4] == ([False, False], False, [True, False], [True, True])
    assert seen[1][4].tolist() == [-1.0, -5.0e8]                     # item 0's pool filled and then improved
    assert np.array_equal(seen[2][4], np.array([-1.0, NEG / np.float32(3.0)], dtype=np.float32))   # after its own going = False
    assert items[0].finished == 2 and items[0].result()[0] == [(3,), (3, 3, 2)]


def test_select_after_the_end_leaves_a_full_pool_unchanged():
    """An item that answered going = False is selected on while its batch runs: a full pool then stays as it is, whether the
    search ended on the full pool (early_stopping=True) or because nothing running can beat it."""
    for es in (True, False):
        full = 0
        for seed in range(6):
            fn = _logits_fn(seed)
            item, steps = _drive(fn, 0, 2, 7, 1, 1.0, es, 1)
            if not (item.is_fin.all() and steps < 7):
                continue
            full += 1
            pool = (item.fin_scores.copy(), list(item.fin_seqs), item.is_fin.copy())
            run = torch.tensor([-1.0, -2.0])                         # live running scores: the candidates' own scores are real
            for _ in range(2):
                *_, going = item.select(*_record(fn, 0, item.run_seqs, run, 4, False))
                assert not going
                assert np.array_equal(item.fin_scores, pool[0]) and item.fin_seqs == pool[1] and np.array_equal(item.is_fin, pool[2])
        assert full > 0


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
