"""The host side of the decode loops, on plain Python values: nothing here sees a device or the HIP library, so a scripted run can
drive every class.  The slot engine's bookkeeping (SlotScheduler), its refill and turn planners (RefillPlanner, TurnPlanner), the
chat pool's session table (SessionTable), the per-request random streams (seeded_requests), the replay of a known run
(replay_slot_run), the split-KV rules with their measurements, the host draw of one row (_host_draw), the beam-sampling
step of one item (beam_sample_select), and beam search's host rule: one request's search state (BeamItem), when a batch of them
goes on (beam_batch_going) and the slots' scheduler of the groups of num_beams rows (BeamSlotScheduler); draft-and-verify decoding's
drafter (NgramDrafter), the host side of its loop (DraftLoop, run_draft_loop) and the predictor of a run's step counts
(predict_draft_run), and in the decode slots the windows a verify step gives each slot (SlotScheduler.step_windows), the guesses of
the next step with the plain / verify rule (slot_guesses) and the predictor (replay_slot_run(draft=, draft_k=))."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m                                      # ops.round_up, restated: importing ops would load the library binding


def _host_draw(logits_row: torch.Tensor, ban: int, inv_temp: float, top_k: int, top_p: float, generator) -> int:
    """HF TopKLogitsWarper + TopPLogitsWarper + multinomial on one row (host)."""
    lg = logits_row.float().cpu() * inv_temp
    if ban >= 0:
        lg[ban] = float("-inf")
    if top_k and 0 < top_k < lg.numel():                             # HF applies TopKLogitsWarper (default top_k = 50) before top-p
        lg = lg.masked_fill(lg < torch.topk(lg, top_k).values[-1], float("-inf"))
    srt, idx = torch.sort(lg, descending=False)
    cum = srt.softmax(-1).cumsum(-1)
    remove = cum <= (1.0 - top_p)
    remove[-1:] = False                                              # min_tokens_to_keep = 1
    srt = srt.masked_fill(remove, float("-inf"))
    probs = torch.zeros_like(lg).scatter(0, idx, srt.softmax(-1))
    return int(torch.multinomial(probs, 1, generator=generator))


def _philox_x0(seed: int, t: int, flat, item: int):
    """The first word of Philox4x32-10 with key = the 64-bit seed and counter (t, flat[i], item, 1), for an array of flat indices
    (uint64 arithmetic on 32-bit values, so no product overflows)."""
    m32 = np.uint64(0xFFFFFFFF)
    c0 = np.full(len(flat), int(t) & 0xFFFFFFFF, dtype=np.uint64)
    c1 = np.asarray(flat, dtype=np.uint64) & m32
    c2 = np.full(len(flat), int(item) & 0xFFFFFFFF, dtype=np.uint64)
    c3 = np.ones(len(flat), dtype=np.uint64)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0


def beam_sample_select(logits, scores, seen_ids, ban: int, inv_temp: float, top_k: int, top_p: float, penalty: float, seed: int,
                       t: int, item: int, draw: bool = True):
    """One item's beam-sampling step on the host, from its nb rows of fp32 logits [nb, V], their running scores [nb] and the ids
    each hypothesis generated (seen_ids[j]): the rule of mh_beam_sample_topk (include/myriad_hip.h) in numpy, what the decode loop
    runs for an item whose device step raised the overflow flag.  Returns (acc [K], flat [K], key [K]), K = 2 * nb, in the
    record's order (key desc, flat asc).  Arithmetic in fp32 in the kernel's operation order; only the top-p masses are summed in
    fp64.  With draw = False the temperature, the cuts and the noise are left out (key = acc)."""
    x = np.asarray(logits, dtype=np.float32)
    nb, V = x.shape
    f32, ninf = np.float32, np.float32(-np.inf)
    accs, flats = [], []
    with np.errstate(all="ignore"):
        for j in range(nb):
            r = x[j]
            mx = np.max(np.where(np.isnan(r), ninf, r))
            lp = (r - mx) - np.log(np.sum(np.exp(r - mx), dtype=f32))
            lp = np.where(np.isnan(lp), ninf, lp).astype(f32)
            ids = sorted({int(i) for i in seen_ids[j] if 0 <= int(i) < V})
            if penalty != 1.0 and ids:
                v = lp[ids]
                lp[ids] = np.where(v < 0, v * f32(penalty), v / f32(penalty))
            if ban >= 0:
                lp[ban] = ninf
            if draw:
                w = lp * f32(inv_temp)
                w = np.where(np.isnan(w), ninf, w).astype(f32)
                k = min(max(int(top_k), 2), V)
                thr = np.partition(w, V - k)[V - k]
                tok = np.nonzero((w >= thr) & np.isfinite(w))[0]
                tok = tok[np.lexsort((tok, -w[tok]))]                # (w desc, id asc)
                if top_p < 1.0 and len(tok) > 2:
                    p = np.exp(w[tok].astype(np.float64) - float(w[tok[0]]))
                    cum = np.cumsum(p)
                    tok = tok[:max(int(np.sum(cum - p < top_p * cum[-1])), 2)]
            else:
                w, tok = lp, np.arange(V)
            a = (w[tok] + f32(scores[j])).astype(f32)
            accs.append(np.where(np.isnan(a), ninf, a))
            flats.append(j * V + tok.astype(np.int64))
        acc, flat = np.concatenate(accs), np.concatenate(flats)
        if draw:
            x0 = _philox_x0(seed, t, flat, item)
            u = ((x0 >> np.uint64(9)).astype(f32) + f32(0.5)) * f32(1.0 / 8388608.0)
            key = (acc + (-np.log(-np.log(u)))).astype(f32)
            key = np.where(np.isnan(key), ninf, key)
        else:
            key = acc
    order = np.lexsort((flat, -key))[:2 * nb]
    return acc[order], flat[order], key[order]


# The chat session's token step uses the split-KV attention kernel (mh_attn_decode_rope_split) when the single-workgroup kernel
# leaves most CUs idle and the cached context is long enough for the chunks to pay for the merge launch: B*H workgroups < 256 (the
# CU count) and at least SPLIT_KV_MIN_KEYS keys when the turn starts.  Measured at batch 1 on the full-size model
# (tools/chat_bench.py): ms per token split / single = 3.04 / 2.89 at 256 keys, 3.23 / 3.33 at 1,024,
# 3.39 / 3.86 at 2,048.  Each kernel has its own captured graph in the session; the choice is made per turn.
SPLIT_KV_MAX_ROWHEADS = 256
SPLIT_KV_MIN_KEYS = 1024


def split_kv_rule(B: int, H: int, kv_len: int) -> bool:
    return B * H < SPLIT_KV_MAX_ROWHEADS and kv_len >= SPLIT_KV_MIN_KEYS


# The slot engine's form of the rule (SlotDecoder(split_kv=None)): `live_rows` conversations decode in one call, the longest has
# `max_kv_len` keys when it is admitted.  It says yes only where the split rows kernel was measured faster than the single-workgroup
# rows kernel on the full-size model (tools/chat_bench.py --pool-split, DESIGN.md section 5, "Chat pool"; ms per token step,
# split_kv False / True, both pools interleaved in one process): N = 1: 3.390 / 3.218 at 1,136 keys, 3.961 / 3.463 at 2,160;
# N = 2: 3.688 / 3.578 and 4.235 / 3.875; N = 4: 3.982 / 3.987 and 4.562 / 4.619 -- at 128 row-heads the split kernel no longer
# wins.  So: at most 64 row-heads (the largest product at which split won) and at least 1,024 keys (the shortest context at which
# it won; the section 5 table says what was measured below that).
SPLIT_KV_ROWS_MAX_ROWHEADS = 64
SPLIT_KV_ROWS_MIN_KEYS = 1024


def split_kv_rows_rule(live_rows: int, H: int, max_kv_len: int) -> bool:
    return live_rows * H <= SPLIT_KV_ROWS_MAX_ROWHEADS and max_kv_len >= SPLIT_KV_ROWS_MIN_KEYS


def common_prefix(a, b) -> int:
    """Length of the longest common prefix of two key lists (the position keys of a context and of a cache)."""
    n = min(len(a), len(b))
    for i in range(n):
        if a[i] != b[i]:
            return i
    return n


class SlotScheduler:
    """The bookkeeping of a decode-slot run, on plain Python values (no device in sight, so a scripted step can drive it): which
    free slot takes which request, each slot's own ids and margins, when a slot finishes -- EOS, a stop sequence at the end of
    ITS ids (kept in the output, as greedy_generate keeps row 0's), or max_new_tokens -- and the order results leave in.

    One round of a run: `admit` requests into `free()` slots until none is free or the requests run out (a request whose first
    pick already ends it never occupies a slot), then, while `live()`, one token step whose per-slot picks go to `step`.
    `pop()` hands out finished (index, ids, margins): in completion order, or with `ordered` in admission (= input) order, a
    result waiting for every earlier one."""

    def __init__(self, slots: int, max_new_tokens: int, stop_ids=(), eos_id: int = 2, ordered: bool = False):
        if slots < 1 or max_new_tokens < 1:
            raise ValueError(f"slots and max_new_tokens must be >= 1, got {slots} and {max_new_tokens}")
        self.slots, self.max_new_tokens, self.eos_id, self.ordered = int(slots), int(max_new_tokens), int(eos_id), bool(ordered)
        self.stops = [tuple(int(t) for t in st) for st in stop_ids]
        self.rows = [None] * self.slots                              # per slot: [index, ids, margins] while it decodes
        self.admitted = 0
        self._done, self._next_out = {}, 0
        self.steps = self.live_row_steps = 0
        self.emitted = 0                                             # tokens the steps appended (the prefill picks not counted)
        self.taken = {}                                              # slot -> tokens the last step appended to it

    def free(self) -> list:
        return [s for s in range(self.slots) if self.rows[s] is None]

    def live(self) -> list:
        return [s for s in range(self.slots) if self.rows[s] is not None]

    def _ended(self, ids: list) -> bool:
        return (ids[-1] == self.eos_id or len(ids) >= self.max_new_tokens
                or any(len(ids) >= len(st) and tuple(ids[-len(st):]) == st for st in self.stops))

    def _finish(self, row) -> None:
        self._done[row[0]] = (row[0], row[1], row[2])

    def admit(self, slot: int, first_id: int, margin: float) -> bool:
        """The next request (index = how many were admitted before it) with its prefill pick.  True: it decodes on in `slot`."""
        if self.rows[slot] is not None:
            raise ValueError(f"slot {slot} is busy")
        row = [self.admitted, [int(first_id)], [float(margin)]]
        self.admitted += 1
        if self._ended(row[1]):
            self._finish(row)
            return False
        self.rows[slot] = row
        return True

    def step(self, ids, margins) -> list:
        """One token step's picks, indexed by slot (idle slots' entries are ignored).  Returns the slots that finished."""
        live = self.live()
        self.steps += 1
        self.live_row_steps += len(live)
        self.emitted += len(live)
        self.taken = {s: 1 for s in live}
        finished = []
        for s in live:
            row = self.rows[s]
            row[1].append(int(ids[s]))
            row[2].append(float(margins[s]))
            if self._ended(row[1]):
                self._finish(row)
                self.rows[s] = None
                finished.append(s)
        return finished

    def step_windows(self, windows) -> list:
        """One token step that gave every live slot a window of tokens (a verify step of draft decoding): `windows` = {slot: (ids,
        margins)}, at least one token per live slot.  A slot's tokens are appended one at a time and the window is cut where its
        request ends -- EOS, a stop sequence ending inside the window, max_new_tokens: the tokens past the cut are dropped and the
        slot finishes.  Counts one step and one live_row_step per live slot, like `step`; `emitted` counts the tokens kept and
        `taken[slot]` how many this step appended.  Returns the slots that finished."""
        live = self.live()
        for s in live:
            if s not in windows or len(windows[s][0]) < 1 or len(windows[s][0]) != len(windows[s][1]):
                raise ValueError(f"slot {s} is live: it needs a window of at least one (id, margin)")
        self.steps += 1
        self.live_row_steps += len(live)
        self.taken = {}
        finished = []
        for s in live:
            row, n = self.rows[s], 0
            for tok, mar in zip(*windows[s]):
                row[1].append(int(tok))
                row[2].append(float(mar))
                n += 1
                if self._ended(row[1]):
                    self._finish(row)
                    self.rows[s] = None
                    finished.append(s)
                    break
            self.taken[s] = n
            self.emitted += n
        return finished

    def pop(self) -> list:
        if not self.ordered:
            out = [self._done.pop(k) for k in list(self._done)]      # dicts keep insertion (= completion) order
        else:
            out = []
            while self._next_out in self._done:
                out.append(self._done.pop(self._next_out))
                self._next_out += 1
        return out

    @property
    def occupancy(self) -> float:
        return self.live_row_steps / (self.steps * self.slots) if self.steps else 0.0


class BeamItem:
    """One request's beam search on the host, on numpy values: HF GenerationMixin._beam_search's bookkeeping for a single item
    (tests/beam_ref.py states the rules), the one place the decode loops keep it -- LlamaDecode.beam_generate drives B items under
    beam_batch_going, the decode slots one per group under BeamSlotScheduler.  `select(top_s, top_i)` takes one step's record for
    the item -- its K = 2 * nb best (score, flat index = row_in_item * V + token), best first -- and answers (ids [nb], src [nb],
    running scores [nb], going): the tokens its nb rows are fed next, the row of the item each continues (0 .. nb - 1) and whether
    the search goes on.  A candidate stops on EOS, on a stop sequence at the end of ITS ids or at max_new_tokens; a stopped
    candidate among the best nb enters the pool at score / len ** length_penalty; `early_stopping` and the "can still improve"
    test (`unsat`) are HF's.  `select` stays callable after going = False: in a batch the item is selected on while another item
    runs, and a pool that was not full can still change.  `all_hit`: every candidate of the last step stopped.  `result()` is the
    best num_return_sequences hypotheses: (their ids as tuples, scores f32 [nrs])."""

    NEG = np.float32(-1.0e9)

    def __init__(self, num_beams: int, vocab: int, max_new_tokens: int, stop_ids=(), eos_id: int = 2, length_penalty: float = 1.0,
                 early_stopping=False, num_return_sequences: int = 1):
        nb, nrs = int(num_beams), int(num_return_sequences)
        if nb < 1 or int(vocab) < 2 * nb or int(max_new_tokens) < 1:
            raise ValueError(f"num_beams={nb} needs num_beams >= 1, a vocabulary of at least {2 * nb} tokens and max_new_tokens >= 1")
        if not 1 <= nrs <= nb:
            raise ValueError(f"num_return_sequences={nrs} must be between 1 and num_beams={nb}")
        if early_stopping not in (True, False, "never"):
            raise ValueError(f"early_stopping must be True, False or 'never', got {early_stopping!r}")
        self.nb, self.K, self.V, self.nrs = nb, 2 * nb, int(vocab), nrs
        self.max_new_tokens, self.eos_id, self.lp, self.early_stopping = int(max_new_tokens), int(eos_id), float(length_penalty), early_stopping
        self.stops = [tuple(int(t) for t in st) for st in stop_ids]
        self.run_seqs = [()] * nb
        self.fin_scores = np.full((nb,), self.NEG, dtype=np.float32)
        self.fin_seqs = [()] * nb
        self.is_fin = np.zeros((nb,), dtype=bool)
        self.unsat = True                                            # the early-stop heuristic still allows an improvement
        self.all_hit = False                                         # every candidate of the last step stopped
        self.gen = 0                                                 # tokens generated so far (= selections made)

    def select(self, top_s, top_i):
        nb, K, NEG, lp = self.nb, self.K, self.NEG, self.lp
        top_s, top_i = np.asarray(top_s, dtype=np.float32).reshape(K), np.asarray(top_i, dtype=np.int64).reshape(K)
        self.gen += 1
        gen_len = self.gen
        par, tok = top_i // self.V, top_i % self.V
        cand = [self.run_seqs[int(par[k])] + (int(tok[k]),) for k in range(K)]
        hits = np.array([c[-1] == self.eos_id or gen_len >= self.max_new_tokens
                         or any(len(c) >= len(st) and c[-len(st):] == st for st in self.stops) for c in cand])
        run_lp = top_s + hits.astype(np.float32) * NEG
        nxt = np.argsort(-run_lp, kind="stable")[:nb]
        self.run_seqs = [cand[k] for k in nxt]
        ids, src, run = tok[nxt], par[nxt], run_lp[nxt]
        did = hits.copy()
        did[nb:] = False                                             # only the top nb candidates may enter the pool
        sc = top_s / np.float32(gen_len ** lp)
        if self.is_fin.all() and self.early_stopping is True:
            sc = sc + NEG
        if not self.unsat:
            sc = sc + NEG
        sc = sc + (~did).astype(np.float32) * NEG
        merged = np.concatenate([self.fin_scores, sc])
        keep = np.argsort(-merged, kind="stable")[:nb]
        mseqs, mfin = self.fin_seqs + cand, np.concatenate([self.is_fin, did])
        self.fin_scores, self.fin_seqs, self.is_fin = merged[keep], [mseqs[k] for k in keep], mfin[keep]
        best_len = self.max_new_tokens if (self.early_stopping == "never" and lp > 0.0) else gen_len
        best_run = np.float32(run[0]) / np.float32(best_len ** lp)
        worst = self.fin_scores.min()
        self.unsat = self.unsat and bool(np.any(np.where(self.is_fin, best_run > worst, best_run > NEG)))
        self.all_hit = bool(hits.all())
        going = self.unsat and not (bool(self.is_fin.all()) and self.early_stopping is True) and not self.all_hit
        return ids, src, run, bool(going and gen_len < self.max_new_tokens)

    @property
    def finished(self) -> int:
        return int(self.is_fin.sum())

    def result(self):
        return [self.fin_seqs[i] for i in range(self.nrs)], self.fin_scores[:self.nrs].copy()


def beam_batch_going(items) -> bool:
    """Whether a batch of BeamItems searched in lockstep (beam_generate's; same arguments, every item selected every step) goes
    on: HF's rule over the whole batch, which is not any(item going) -- each clause may hold through a different item."""
    return (any(it.unsat for it in items) and not (items[0].early_stopping is True and all(it.is_fin.all() for it in items))
            and not all(it.all_hit for it in items) and items[0].gen < items[0].max_new_tokens)


class BeamSlotScheduler:
    """SlotScheduler over G = slots / num_beams beam groups: a group of num_beams rows holds one request's search (a BeamItem
    made by `make_item()`), and is free again as soon as its item ends.  Same round as SlotScheduler: `admit(group, top_s, top_i)`
    with the prefill's record (the K best first tokens; the item's first selection -- False: the request ended there and never
    occupies the group), then, while `live()`, `step(top_s [G, K], top_i [G, K])` with one token step's record (idle groups'
    entries are ignored), which returns the groups that finished.  After either, `feed[g]` = (ids, src, running scores) is what
    the group's rows take next, src counted within the group.  `pop()` hands out (index, sequences, scores f32 [nrs]) in
    completion order, or with `ordered` in admission order.  `slots` counts groups: RefillPlanner drives it unchanged."""

    def __init__(self, groups: int, make_item, ordered: bool = False):
        if groups < 1:
            raise ValueError(f"groups must be >= 1, got {groups}")
        self.slots, self.make_item, self.ordered = int(groups), make_item, bool(ordered)
        self.rows = [None] * self.slots                              # per group: [index, item] while it searches
        self.feed = [None] * self.slots
        self.admitted = 0
        self._done, self._next_out = {}, 0
        self.steps = self.live_row_steps = self.finished_hypotheses = 0

    def free(self) -> list:
        return [g for g in range(self.slots) if self.rows[g] is None]

    def live(self) -> list:
        return [g for g in range(self.slots) if self.rows[g] is not None]

    def _finish(self, index: int, item) -> None:
        seqs, scores = item.result()
        self.finished_hypotheses += item.finished
        self._done[index] = (index, seqs, scores)

    def admit(self, group: int, top_s, top_i) -> bool:
        if self.rows[group] is not None:
            raise ValueError(f"group {group} is busy")
        item, index = self.make_item(), self.admitted
        self.admitted += 1
        *feed, going = item.select(top_s, top_i)
        if not going:
            self._finish(index, item)
            return False
        self.rows[group], self.feed[group] = [index, item], tuple(feed)
        return True

    def step(self, top_s, top_i) -> list:
        live = self.live()
        self.steps += 1
        self.live_row_steps += len(live)
        finished = []
        for g in live:
            index, item = self.rows[g]
            *feed, going = item.select(top_s[g], top_i[g])
            self.feed[g] = tuple(feed)
            if not going:
                self._finish(index, item)
                self.rows[g] = self.feed[g] = None
                finished.append(g)
        return finished

    pop = SlotScheduler.pop

    @property
    def occupancy(self) -> float:
        return self.live_row_steps / (self.steps * self.slots) if self.steps else 0.0


class RefillPlanner:
    """Which waiting requests are prefilled together, and when: the host side of the slot engine's packed prefill, on plain Python
    values like SlotScheduler (whose free / live slots it reads), so a scripted run can drive it.

    `next_pass()` is asked at every refill point until it answers []: it hands out [(slot, request), ...] for ONE prefill pass --
    the next waiting requests in input order, one per free slot in ascending slot order, at most `prefill_batch` of them and as
    many as keep the pass's row count (the lengths' sum rounded up to 64) within `prefill_rows`; the first always goes, so a
    request too long to share a pass, or longer than the cap, gets a pass of its own.  `refill_min` = k holds a pass back while
    fewer than k slots are free, unless nothing is live or the requests have run out (the input ended and everything left is
    waiting already: the planner looks one request past the pass it could fill).  prefill_batch = 1, refill_min = 1 is the
    engine's one-request refill: the lowest free slot takes the next request, again if that one ended on its first pick."""

    def __init__(self, sched: "SlotScheduler", requests, prefill_batch: int = 1, prefill_rows: int = 2048, refill_min: int = 1,
                 length=len):
        if prefill_batch < 1 or refill_min < 1 or prefill_rows < 1:
            raise ValueError(f"prefill_batch, refill_min and prefill_rows must be >= 1, got {prefill_batch}, {refill_min} and "
                             f"{prefill_rows}")
        self.sched, self.it, self.more, self.waiting, self.length = sched, iter(requests), True, [], length
        self.prefill_batch, self.prefill_rows = int(prefill_batch), int(prefill_rows)
        self.refill_min = min(int(refill_min), sched.slots)
        self.passes = self.packed_rows = 0

    def next_pass(self) -> list:
        free = self.sched.free()
        if not free:
            return []
        want = min(self.prefill_batch, len(free))
        while self.more and len(self.waiting) < want + (self.refill_min > 1):    # refill_min = 1 never needs to look ahead
            try:
                self.waiting.append(next(self.it))
            except StopIteration:
                self.more = False
        if not self.waiting or (len(free) < self.refill_min and self.sched.live() and self.more):
            return []
        n, rows = 0, 0
        for req in self.waiting[:want]:
            if n and round_up(rows + self.length(req), 64) > self.prefill_rows:
                break
            n, rows = n + 1, rows + self.length(req)
        group, self.waiting = self.waiting[:n], self.waiting[n:]
        self.passes += 1
        self.packed_rows += rows
        return list(zip(free, group))


class TurnPlanner:
    """RefillPlanner's place in SlotDecoder.run_turns: every turn has ITS session's slot, so the passes are fixed when the call
    starts -- the turns in list order, up to `prefill_batch` per pass and as many as keep the pass's NEW rows (rounded up to 64)
    within `prefill_rows`; the first of a pass always goes.  `items` = [(slot, request)], `length(request)` = its new rows."""

    def __init__(self, items, prefill_batch: int = 1, prefill_rows: int = 2048, length=len):
        if prefill_batch < 1 or prefill_rows < 1:
            raise ValueError(f"prefill_batch and prefill_rows must be >= 1, got {prefill_batch} and {prefill_rows}")
        self.groups, self.passes, self.packed_rows = [], 0, 0
        rows = 0
        for item in items:
            n = length(item[1])
            if not self.groups or len(self.groups[-1]) >= int(prefill_batch) or round_up(rows + n, 64) > int(prefill_rows):
                self.groups.append([])
                rows = 0
            self.groups[-1].append(item)
            rows += n
        self._length = length

    def next_pass(self) -> list:
        if not self.groups:
            return []
        group = self.groups.pop(0)
        self.passes += 1
        self.packed_rows += sum(self._length(req) for _, req in group)
        return group


class ScorePlan:
    """The passes of LlamaDecode.score_continuations, fixed when the call starts, on plain Python values (no device in sight).

    Prompt i has `prompt_lens[i]` rows and the candidates `candidates[i]`, each a non-empty list of ids t_0 .. t_{n-1}.  The prompts
    go in list order into groups of at most `slots` prompts whose rows (rounded up to 64) stay within `rows` -- one packed prompt
    prefill each, prompt i in slot `slot[i]` of its group; the first of a group always goes.  log p(t_0 | prompt) comes from the
    prompt's LAST prefill row; log p(t_j | prompt, t_<j), j >= 1, from candidate row j - 1.  So a scoring pass packs rows
    t_0 .. t_{n-2} of a candidate at positions S_i .. S_i + n - 2 as the segment (row0, n - 1, slot_i, S_i) of
    mh_attn_prefill_ragged_shared, and a one-token candidate has no segment.  A group's candidates go in order into scoring passes
    of at most `rows` packed rows (rounded up to 64); a candidate is never split, the first of a pass always goes, and a prompt
    whose candidates overflow a pass is visited again by the next with the same slot and past -- the scoring pass writes no cache
    row, so the prompt stays cached.

    `groups` = [dict(prompts, slots, first_rows, first_targets, first_map, passes)]: `first_rows` replicates a prompt's row of
    the prefill's [P, V] logits once per candidate (the gather list), `first_targets` the t_0 beside it and `first_map` its
    (prompt, candidate, 0).  A pass = dict(seg, M, ids, pos, targets, map): the segment table, the padded frame's rows, and per
    packed row (frame order, the segments back to back from row 0) the token id fed, its position, the target id scored on that
    row's logits and its (prompt, candidate, token index).

    ValueError: no prompt, a prompt without rows, an empty candidate list, an empty candidate, an id outside [0, vocab), or a
    last fed position S_i + n - 2 outside the rotary table of `max_pos` rows (S_i + n - 1 > max_pos) -- the kernel clamps a
    position silently, so the host refuses."""

    def __init__(self, prompt_lens, candidates, vocab: int, max_pos: int, slots: int = 8, rows: int = 2048):
        if slots < 1 or rows < 1:
            raise ValueError(f"slots and rows must be >= 1, got {slots} and {rows}")
        prompt_lens = [int(n) for n in prompt_lens]
        if not prompt_lens or len(prompt_lens) != len(candidates):
            raise ValueError("one non-empty list of candidates per prompt, at least one prompt")
        cands = []
        for i, (S, cs) in enumerate(zip(prompt_lens, candidates)):
            if S < 1:
                raise ValueError(f"prompt {i} has no rows")
            cs = [[int(t) for t in c] for c in cs]
            if not cs:
                raise ValueError(f"prompt {i}: an empty candidate list")
            for c, ids in enumerate(cs):
                if not ids:
                    raise ValueError(f"prompt {i}: candidate {c} is empty")
                if any(not 0 <= t < int(vocab) for t in ids):
                    raise ValueError(f"prompt {i}: candidate {c} has an id outside [0, {int(vocab)})")
                if S + len(ids) - 1 > int(max_pos):
                    raise ValueError(f"prompt {i}: candidate {c} ends at position {S + len(ids) - 2}, the rotary table has "
                                     f"{int(max_pos)}")
            cands.append(cs)
        self.prompt_lens, self.candidates = prompt_lens, cands
        self.groups, self.passes, self.packed_rows, self.segments = [], 0, 0, 0
        members, used = [], 0
        for i, S in enumerate(prompt_lens):
            if members and (len(members) >= int(slots) or round_up(used + S, 64) > int(rows)):
                self._close(members, int(rows))
                members, used = [], 0
            members.append(i)
            used += S
        self._close(members, int(rows))

    def _close(self, members, rows_cap: int) -> None:
        group = dict(prompts=list(members), slots=list(range(len(members))), first_rows=[], first_targets=[], first_map=[],
                     passes=[])
        cur = None
        for slot, i in enumerate(members):
            S = self.prompt_lens[i]
            for c, ids in enumerate(self.candidates[i]):
                group["first_rows"].append(slot)
                group["first_targets"].append(ids[0])
                group["first_map"].append((i, c, 0))
                n = len(ids) - 1
                if n == 0:
                    continue
                if cur is None or round_up(cur["used"] + n, 64) > rows_cap:
                    cur = dict(seg=[], used=0, ids=[], pos=[], targets=[], map=[])
                    group["passes"].append(cur)
                cur["seg"].append((cur["used"], n, slot, S))
                cur["used"] += n
                cur["ids"] += ids[:-1]
                cur["pos"] += list(range(S, S + n))
                cur["targets"] += ids[1:]
                cur["map"] += [(i, c, j) for j in range(1, n + 1)]
        for ps in group["passes"]:
            ps["M"] = round_up(ps.pop("used"), 64)
            self.packed_rows += len(ps["ids"])
            self.segments += len(ps["seg"])
        self.passes += 1 + len(group["passes"])
        self.packed_rows += sum(self.prompt_lens[i] for i in members)
        self.groups.append(group)


class SessionTable:
    """Which conversation lives in which decode slot, and what its slot's cache holds: the host side of SlotDecoder.run_turns, on
    plain Python values like SlotScheduler (no device in sight).

    At most `slots` sessions are open; a session (any object: hashable ones by value, others by identity, held until `close`)
    is pinned to one slot from its first turn until `close(session)` frees it.  Per session the table keeps one key per cached
    position, DecodeSession's convention: `begin(session, keys)` answers (slot, past, reason) with past =
    min(common_prefix(keys, cached), len(keys) - 1) -- at least one row is always prefilled, it gives the first logits -- and
    `end(session, keys, ids)` records the context's keys plus ("t", id) for ids[:-1]: the last pick of a turn has no KV, and a slot
    row goes idle the moment its turn ends, so no id the host does not know is ever fed (DecodeSession's ("x",) case does not
    arise).  Between `begin` and `end` the session's keys are dropped: a turn that fails or is abandoned midway leaves a cache
    nobody trusts.

    `sync(stamp)` is called with what the cached rows depend on -- (the caller's weights_version, _decode_weights_id, the merge
    id of a merged qkv copy) -- before the turns of a call: whenever it moves, every session's keys are dropped, with
    DecodeSession's reasons ("weights changed" / "decode weights changed").  `clear()` drops them all ("empty cache"): the
    caches were overwritten.  `reason` is None when the cached rows were usable, whatever `past` came out."""

    def __init__(self, slots: int):
        if slots < 1:
            raise ValueError(f"slots must be >= 1, got {slots}")
        self.slots = int(slots)
        self.stamp = None
        self._open = {}                                              # key -> [session, slot, keys, why the keys are empty]

    @staticmethod
    def _key(session):
        try:
            hash(session)
            return ("v", session)
        except TypeError:
            return ("id", id(session))                               # the entry holds the object, so the id stays its own

    def __len__(self) -> int:
        return len(self._open)

    def __contains__(self, session) -> bool:
        return self._key(session) in self._open

    def slot_of(self, session) -> int:
        return self._open[self._key(session)][1]

    def keys_of(self, session) -> list:
        return list(self._open[self._key(session)][2])

    def open(self, session) -> int:
        """The session's slot; a new session takes the lowest free one."""
        k = self._key(session)
        if k not in self._open:
            used = {e[1] for e in self._open.values()}
            if len(used) >= self.slots:
                raise ValueError(f"all {self.slots} slots hold an open session: close() one before opening another")
            self._open[k] = [session, min(set(range(self.slots)) - used), [], "empty cache"]
        return self._open[k][1]

    def close(self, session) -> None:
        self._open.pop(self._key(session), None)

    def drop(self, session, reason: str = "empty cache") -> None:
        e = self._open.get(self._key(session))
        if e is not None:
            e[2], e[3] = [], reason

    def clear(self, reason: str = "empty cache") -> None:
        for e in self._open.values():
            e[2], e[3] = [], reason

    def sync(self, stamp) -> None:
        if self.stamp is not None and stamp != self.stamp:
            self.clear("weights changed" if stamp[0] != self.stamp[0] else "decode weights changed")
        self.stamp = stamp

    def begin(self, session, keys, reset_reason: Optional[str] = None):
        slot = self.open(session)
        e = self._open[self._key(session)]
        if len(keys) < 1:
            raise ValueError("a turn needs at least one context position")
        reason = reset_reason if reset_reason is not None else (None if e[2] else e[3])
        cached = [] if reason is not None else e[2]
        past = min(common_prefix(keys, cached), len(keys) - 1)
        e[2], e[3] = [], "empty cache"                               # until end(): the slot is being written
        return slot, past, reason

    def end(self, session, keys, ids) -> None:
        e = self._open.get(self._key(session))
        if e is not None:
            e[2], e[3] = list(keys) + [("t", int(t)) for t in list(ids)[:-1]], None

    def plan(self, turns, stamp):
        """One run_turns call: `turns` = [(session, keys) or (session, keys, reset_reason)], at most one per session.  Syncs
        the stamp and begins every turn; returns [(slot, past, reason)] in the turns' order."""
        seen = set()
        for t in turns:
            k = self._key(t[0])
            if k in seen:
                raise ValueError("at most one turn per session in one call")
            seen.add(k)
        new = [k for k in seen if k not in self._open]
        if len(self._open) + len(new) > self.slots:
            raise ValueError(f"{len(self._open)} open sessions + {len(new)} new ones do not fit {self.slots} slots: close() some")
        self.sync(stamp)
        return [self.begin(t[0], t[1], t[2] if len(t) > 2 else None) for t in turns]


def seeded_requests(requests, generator: Optional[torch.Generator] = None, seeds=None):
    """Pairs every request with the seed of its own random stream: yields (request, seed) in input order.  The seed is drawn when
    the request is taken from the input -- torch.randint(0, 2**63 - 1, (1,), generator=generator), the draw greedy_generate makes
    once per call -- so request i gets the i-th draw however RefillPlanner groups or holds back the refills; `seeds` (an iterable
    of ints in [0, 2**63), one per request in input order) replaces the draws and leaves `generator` untouched.  No device in
    sight, like SlotScheduler and RefillPlanner."""
    given = None if seeds is None else iter(seeds)
    for req in requests:
        if given is None:
            seed = int(torch.randint(0, 2**63 - 1, (1,), generator=generator))
        else:
            seed = next(given, None)
            if seed is None:
                raise ValueError("seeds: fewer seeds than requests")
            seed = int(seed)
            if not 0 <= seed < 2**63:
                raise ValueError(f"seeds: {seed} is outside [0, 2**63)")
        yield req, seed


def _request_generator(seed: int, t: int) -> torch.Generator:
    """The host generator for token t of the request with `seed`: the rare row the device sampler hands back (kept = -1) is drawn
    from it, never from the run's shared generator, so it cannot shift another request's stream."""
    g = torch.Generator()
    g.manual_seed((int(seed) * 0x9E3779B1 + int(t)) % 2**63)
    return g


def f32_at_least(x: float):
    """The smallest float32 >= x (a numpy float32).  For every float32 p: p < x (x a double) iff p < f32_at_least(x), so a device
    that tests p >= this value decides exactly what the host decides with p < x."""
    t = np.float32(x)
    return t if float(t) >= float(x) else np.nextafter(t, np.float32(np.inf))


def slot_guesses(sched: "SlotScheduler", drafter, k: int) -> dict:
    """The guesses of the next step of a slot run with draft decoding, {live slot: real guesses}: drafter.propose(the slot's ids
    so far, k - 1), clamped to max_new_tokens - len(ids) - 1 guesses, so that no row is fed past the last token the request can
    still emit (a window of 1 + n guesses emits at most 1 + n tokens) and pos + rows never leaves the slot's capacity.  [] where
    the drafter has nothing.  THE RULE: the step is the verify step (slots x k rows) iff at least one live slot has a real guess,
    otherwise the engine's plain one-row-per-slot step."""
    out = {}
    for s in sched.live():
        ids = sched.rows[s][1]
        room = min(int(k) - 1, sched.max_new_tokens - len(ids) - 1)
        out[s] = [int(t) for t in drafter.propose(list(ids), room)][:room] if room > 0 else []
    return out


def replay_slot_run(lengths, ids, slots: int, max_new_tokens: int, stop_ids=(), eos_id: int = 2, prefill_batch: int = 1,
                    prefill_rows: int = 2048, refill_min: int = 1, draft=None, draft_k: int = 4, host_drawn=None) -> dict:
    """The counters of a slot run whose picks are known: request i has a prompt of lengths[i] rows and generates ids[i] (which must
    end where the stop rule ends it).  SlotScheduler + RefillPlanner driven as SlotDecoder.run drives them, without a device.
    With `draft` (a drafter nobody teaches during the run) and `draft_k` = K the run is SlotDecoder.run(draft=, draft_k=)'s with no
    host draw: every step takes slot_guesses' guesses and is a verify step iff a live slot has one, a slot's window is its fed
    token's pick plus the leading guesses its known answer confirms, and the answer gains verify_steps, plain_steps, draft_proposed
    (real guesses fed), draft_accepted (emitted tokens that were confirmed guesses) and emitted.  `host_drawn` (with `draft`):
    per request the token indices the host drew; such a row ends its slot's window, whatever the guess behind it."""
    if draft is not None:
        return _replay_draft_slot_run(lengths, ids, slots, max_new_tokens, stop_ids, eos_id, prefill_batch, prefill_rows, refill_min,
                                      draft, int(draft_k), host_drawn)
    sched = SlotScheduler(slots, max_new_tokens, stop_ids, eos_id)
    plan = RefillPlanner(sched, range(len(lengths)), prefill_batch, prefill_rows, refill_min, length=lambda i: lengths[i])
    owner, prefills = [None] * slots, 0
    while True:
        group = plan.next_pass()
        while group:
            for s, i in group:
                prefills += 1
                if sched.admit(s, ids[i][0], 0.0):
                    owner[s] = [i, 1]
            group = plan.next_pass()
        live = sched.live()
        if not live:
            break
        picks = [0] * slots
        for s in live:
            picks[s] = ids[owner[s][0]][owner[s][1]]
            owner[s][1] += 1
        sched.step(picks, [0.0] * slots)
    return dict(prefills=prefills, prefill_passes=plan.passes, packed_rows=plan.packed_rows, steps=sched.steps,
                live_row_steps=sched.live_row_steps, occupancy=sched.occupancy)


def _replay_draft_slot_run(lengths, ids, slots, max_new_tokens, stop_ids, eos_id, prefill_batch, prefill_rows, refill_min, draft,
                           K: int, host_drawn=None) -> dict:
    """replay_slot_run with a drafter: see there."""
    host_drawn = [set(h) for h in host_drawn] if host_drawn is not None else [()] * len(lengths)
    sched = SlotScheduler(slots, max_new_tokens, stop_ids, eos_id)
    plan = RefillPlanner(sched, range(len(lengths)), prefill_batch, prefill_rows, refill_min, length=lambda i: lengths[i])
    owner, prefills = [None] * slots, 0                              # per slot: its request
    st = dict(verify_steps=0, plain_steps=0, draft_proposed=0, draft_accepted=0)
    while True:
        group = plan.next_pass()
        while group:
            for s, i in group:
                prefills += 1
                if sched.admit(s, ids[i][0], 0.0):
                    owner[s] = i
            group = plan.next_pass()
        live = sched.live()
        if not live:
            break
        guesses = slot_guesses(sched, draft, K) if K > 1 else {s: [] for s in live}
        verify = any(guesses[s] for s in live)
        windows = {}
        for s in live:
            chain, n = ids[owner[s]], len(sched.rows[s][1])          # row j's pick is chain[n + j] while every earlier guess was right
            take = 1
            while take <= len(guesses[s]) and n + take < len(chain) and n + take - 1 not in host_drawn[owner[s]] \
                    and guesses[s][take - 1] == chain[n + take - 1]:
                take += 1
            windows[s] = (chain[n:n + take], [0.0] * take)
        sched.step_windows(windows)
        st["verify_steps" if verify else "plain_steps"] += 1
        if verify:
            st["draft_proposed"] += sum(len(guesses[s]) for s in live)
            st["draft_accepted"] += sum(sched.taken[s] - 1 for s in live)
    return dict(prefills=prefills, prefill_passes=plan.passes, packed_rows=plan.packed_rows, steps=sched.steps,
                live_row_steps=sched.live_row_steps, occupancy=sched.occupancy, emitted=sched.emitted, **st)


# ---- draft-and-verify greedy decoding (LlamaDecode.greedy_generate(draft=...)): the drafter, the predictor of a run's step counts
# and the host side of the loop.  The device verifies K - 1 guessed tokens in one K-row token step whose rows carry the bits of K
# one-row steps, so whatever the drafter proposes the ids and margins are those of the plain loop; the drafter only decides how
# many steps the answer takes.
DRAFT_START = -1                                                     # the start sentinel in front of every answer


class NgramDrafter:
    """Proposes the continuation of an answer from the answers seen so far: for every context of 1 .. `max_order` ids (the start
    sentinel counts as one) the table counts each id that followed it.  Deterministic, no device call.  Any object with `propose`
    and `observe` serves as a drafter."""

    def __init__(self, corpus=(), max_order: int = 4):
        if int(max_order) < 1:
            raise ValueError(f"max_order must be >= 1, got {max_order}")
        self.max_order = int(max_order)
        self.table = {}                                              # context tuple -> {successor: count}, in order of first sight
        for ids in corpus:
            self.observe(ids)

    def observe(self, ids) -> None:
        """Add a finished answer (its generated ids)."""
        seq = [DRAFT_START] + [int(t) for t in ids]
        for i in range(1, len(seq)):
            for n in range(1, min(self.max_order, i) + 1):
                succ = self.table.setdefault(tuple(seq[i - n:i]), {})
                succ[seq[i]] = succ.get(seq[i], 0) + 1

    def _next(self, h: list):
        for n in range(min(self.max_order, len(h)), 0, -1):          # the longest suffix the table knows
            succ = self.table.get(tuple(h[-n:]))
            if succ:
                return max(succ, key=succ.get)                       # most frequent; max() keeps the first of equals = first observed
        return None

    def propose(self, history, k: int) -> list:
        """At most k ids that may follow `history` (the ids generated so far in this answer; the sentinel is put in front here):
        the most frequent successor of the longest known suffix, ties to the one observed first, extended on its own proposals."""
        h, out = [DRAFT_START] + [int(t) for t in history], []
        while len(out) < int(k):
            t = self._next(h)
            if t is None:
                break
            out.append(t)
            h.append(t)
        return out


def _ends_with_stop(ids: list, stop_ids) -> bool:
    return any(len(ids) >= len(st) and ids[-len(st):] == list(st) for st in stop_ids)


class DraftLoop:
    """The host side of one B = 1 answer decoded with draft-and-verify steps: which step comes next and with which guesses, and
    what a step's record adds to the answer.  `take` gets a step's record -- the K picks with their margins and p_max and n_out,
    the count the device accepted (a plain step: one pick, n_out = 1) -- and emits n_out tokens, cut at EOS, at a stop sequence
    ending inside the window and at max_new_tokens.  Under do_sample a row with p_max < top_p (the host-draw rule) ends the window
    on the device already; its id is drawn here (`draw(j)`) and handed on as `fed`, the id the next step must be fed in place of
    the one the device fed itself.  `stats` gains steps (tokens), verify_steps, plain_steps, draft_proposed (real guesses fed) and
    draft_accepted (emitted tokens that were confirmed guesses)."""

    def __init__(self, drafter, k: int, max_new_tokens: int, stop_ids=(), eos_id: int = 2, min_length: int = 1,
                 do_sample: bool = False, top_p: float = 1.0, stats: Optional[dict] = None):
        self.drafter, self.k = drafter, int(k)
        self.max_new_tokens, self.stop_ids, self.eos_id, self.min_length = int(max_new_tokens), tuple(stop_ids), int(eos_id), int(min_length)
        self.do_sample, self.top_p = bool(do_sample), float(top_p)
        self.stats = {} if stats is None else stats
        for name in ("steps", "verify_steps", "plain_steps", "draft_proposed", "draft_accepted", "sampled_rows", "host_sampled_rows"):
            self.stats.setdefault(name, 0)
        self.stats.setdefault("min_pmax", 1.0)
        self.ids, self.margins = [], []
        self.done, self.fed, self.use_draft = False, None, True

    def ban(self) -> int:
        """The EOS ban of the next (plain) step."""
        return self.eos_id if len(self.ids) < self.min_length else -1

    def guesses(self) -> list:
        """The K - 1 guesses of the next step, real proposals first and id 0 as filler, or [] for a plain one-row step: while
        the EOS ban is on, when the drafter proposes nothing, at K = 1, or with the verify step switched off (`use_draft`)."""
        if not self.use_draft or self.k < 2 or len(self.ids) < self.min_length:
            return []
        prop = [int(t) for t in self.drafter.propose(list(self.ids), self.k - 1)][:self.k - 1]
        if not prop:
            return []
        self.stats["draft_proposed"] += len(prop)
        return prop + [0] * (self.k - 1 - len(prop))

    def take(self, ids, margins, pmax, n_out: int, draw=None, first: bool = False, kept=None) -> None:
        """One step's record.  `first`: the prefill's pick, which counts as neither kind of step.  `kept` (the device sampler's
        kept counts of the rows): the device drew every row but those with kept < 0, which the host draws -- the kept rule in
        place of the p_max rule; such a row ended the window on the device."""
        n_out, rows = int(n_out), len(ids)
        if not 1 <= n_out <= rows:
            raise ValueError(f"n_out={n_out} of a {rows}-row record")
        if not first:
            self.stats["verify_steps" if rows > 1 else "plain_steps"] += 1
        self.fed, taken = None, 0
        for j in range(n_out):
            tok, pm = int(ids[j]), float(pmax[j])
            self.margins.append(float(margins[j]))
            self.stats["steps"] += 1
            if self.do_sample:
                self.stats["min_pmax"] = min(self.stats["min_pmax"], pm)
                if pm < self.top_p:
                    self.stats["sampled_rows"] += 1
                if kept is not None and kept[j] >= 0:
                    self.stats["device_sampled_rows"] = self.stats.get("device_sampled_rows", 0) + 1
                elif kept is not None or pm < self.top_p:
                    if j != n_out - 1:
                        raise ValueError("a row that needs a host draw must end its window")
                    self.stats["host_sampled_rows"] += 1
                    tok = self.fed = int(draw(j))
            self.ids.append(tok)
            taken += 1
            if tok == self.eos_id or _ends_with_stop(self.ids, self.stop_ids) or len(self.ids) >= self.max_new_tokens:
                self.done = True
                break
        if rows > 1:
            self.stats["draft_accepted"] += taken - 1


def run_draft_loop(loop: DraftLoop, first, plain_step, verify_step) -> DraftLoop:
    """Drive `loop` to the end of its answer.  `first` = the prefill's record (ids, margins, pmax, n_out, draw);
    `plain_step(ban, fed)` and `verify_step(guesses, fed)` run one step and return such a record, `fed` being the id the host
    drew for the last token (else None: the device fed itself)."""
    loop.take(*first, first=True)
    while not loop.done:
        g = loop.guesses()
        loop.take(*(verify_step(g, loop.fed) if g else plain_step(loop.ban(), loop.fed)))
    return loop


def predict_draft_run(drafter, chain, k: int, min_length: int = 1, host_drawn=()) -> dict:
    """The step counts of decoding the answer `chain` (every emitted id, the prefill's pick first) with `drafter` at K = k rows
    per verify step: verify_steps, plain_steps, draft_proposed, draft_accepted, as DraftLoop counts them.  `host_drawn`: the
    token indices (places in `chain`) the host drew -- such a row ends its window, whatever the guess behind it."""
    chain, host_drawn = [int(t) for t in chain], set(host_drawn)
    st = dict(verify_steps=0, plain_steps=0, draft_proposed=0, draft_accepted=0)
    n = 1
    while n < len(chain):
        prop = [] if k < 2 or n < min_length else [int(t) for t in drafter.propose(chain[:n], k - 1)][:k - 1]
        if not prop:
            st["plain_steps"] += 1
            n += 1
            continue
        st["verify_steps"] += 1
        st["draft_proposed"] += len(prop)
        fed = prop + [0] * (k - 1 - len(prop))
        take = 1                                                     # row j's pick is chain[n + j] while every earlier guess was right
        while take < k and n + take < len(chain) and n + take - 1 not in host_drawn and fed[take - 1] == chain[n + take - 1]:
            take += 1
        st["draft_accepted"] += take - 1
        n += take
    return st


def load_draft_corpus(path: str, tokenize=None) -> list:
    """A drafter's corpus from a file: a JSON list of id lists, or a results .jsonl of an evaluation run whose `output` texts
    `tokenize` (text -> ids) turns into ids."""
    import json
    with open(path) as f:
        text = f.read()
    try:
        data = json.loads(text)
        if isinstance(data, list) and all(isinstance(r, list) for r in data):
            return [[int(t) for t in r] for r in data]
        data = [data]
    except json.JSONDecodeError:
        data = [json.loads(ln) for ln in text.splitlines() if ln.strip()]
    if tokenize is None:
        raise ValueError(f"{path}: a results file needs a tokenizer to turn its output texts into ids")
    return [[int(t) for t in tokenize(r["output"])] for r in data if isinstance(r, dict) and "output" in r]
