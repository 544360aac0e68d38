"""Host restatements of the verify step's per-row tail (myriad_amd/csrc/draft_sample.hip), in numpy and plain integers: what the
kernel tests hold the launches to, and what tests/test_draft_sampling_cpu.py pins against a token-by-token walk."""
import numpy as np


def bitmap_ids(words, V):
    """The ids < V whose bits are set in a row of the seen bitmap (int32 / uint32 words)."""
    w = np.asarray(words).astype(np.int64) & 0xFFFFFFFF
    return {int(i) * 32 + b for i in np.nonzero(w)[0] for b in range(32) if (int(w[i]) >> b) & 1 and int(i) * 32 + b < V}


def bitmap_of(ids, V):
    """A bitmap row (int32 words) with the bits of `ids` set."""
    w = np.zeros((V + 31) // 32, dtype=np.uint32)
    for i in ids:
        w[i >> 5] |= np.uint32(1 << (i & 31))
    return w.view(np.int32)


def penalise(row, ids, pen):
    """HF's repetition penalty on one f32 row: x * p below zero, x / p otherwise, each id of the set once (f32 arithmetic)."""
    out = np.array(row, dtype=np.float32)
    p = np.float32(pen)
    for i in sorted(set(ids)):
        out[i] = out[i] * p if out[i] < 0 else out[i] / p
    return out


def penalty_draft_ref(logits, seen_sets, ids_k, nrow, live, K, pen):
    """mh_repetition_penalty_draft_rows: logits f32 [G*K, V]; seen_sets[g] = the ids of group g's bitmap; ids_k [G*K]."""
    logits = np.array(logits, dtype=np.float32)
    V = logits.shape[1]
    for g in range(len(live)):
        for j in range(K):
            if live[g] and j < nrow[g]:
                extra = [int(t) for t in ids_k[g * K:g * K + j + 1] if 0 <= int(t) < V]
                logits[g * K + j] = penalise(logits[g * K + j], set(seen_sets[g]) | set(extra), pen)
    return logits


def pick_draft_ref(logits, gen, nrow, live, K, min_length, eos_id):
    """The greedy pick of mh_sample_rows_draft (draw = 0): per row the arg-max (lowest id of the largest value) with eos_id banned
    while gen[g] + j < min_length; an idle row picks -1."""
    logits = np.asarray(logits, dtype=np.float32)
    out = []
    for g in range(len(live)):
        for j in range(K):
            if not live[g] or j >= nrow[g]:
                out.append(-1)
                continue
            x = logits[g * K + j].copy()
            if gen[g] + j < min_length:
                x[eos_id] = -np.inf
            out.append(int(np.argmax(x)))
    return out


def accept_sampled_ref(nxt, mar, pmx, kept, ids, nguess, live, top_p, pos, kv, nid, gen, seen_set, K, V):
    """One group of mh_draft_accept_sampled_rows: (rec [4K + 1], ids[0], next_id, pos, kvlen, gen, seen set); kept / seen_set None
    as in the launch."""
    if not live:
        return [-1.0] * K + [0.0] * (3 * K + 1), ids[0], nid, pos, kv, gen, seen_set
    n = 1
    for j in range(min(max(nguess, 0), K - 1)):
        host = kept[j] < 0 if kept is not None else (top_p > 0 and not pmx[j] >= top_p)
        if host or nxt[j] != ids[j + 1]:
            break
        n += 1
    rec = [float(t) for t in nxt] + list(mar) + list(pmx) + [float(k) for k in (kept if kept is not None else [0] * K)] + [float(n)]
    if seen_set is not None:
        seen_set = set(seen_set) | {int(t) for t in ids[:n] if 0 <= int(t) < V}
    return rec, nxt[n - 1], nxt[n - 1], pos + n, pos + n + 1, gen + n, seen_set
