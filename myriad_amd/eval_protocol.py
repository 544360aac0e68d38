"""AQA evaluation protocol: generated text -> anomaly label, per-scene accuracy / AUROC, jsonl records,
rank-sharded evaluation.  Host-side numpy; mirrors

  * `get_model_answer` / `get_performance`, scripts/eval_protocol/summary_results.py:8-182
  * the per-sample record the evaluation driver writes, evaluation_aqa_dataset.py:339-387
  * the result-directory summary table, scripts/eval_protocol/summary_results.py:185-245

The keyword lists that define the protocol are data (`eval_rules.json`, extracted from the reference script by
tools/make_golden_host.py); parity is pinned by tests/golden/eval_protocol.json, produced by the reference's own
functions on seeded synthetic answers."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

_RULES_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_rules.json")


@dataclass(frozen=True)
class AnswerRules:
    abnormal_words: Tuple[str, ...]
    normal_words: Tuple[str, ...]

    @staticmethod
    def default() -> "AnswerRules":
        d = json.load(open(_RULES_PATH))
        return AnswerRules(tuple(d["abnormal_words"]), tuple(d["normal_words"]))


def classify_answer(text: str, mode: int = 0, rules: Optional[AnswerRules] = None) -> int:
    """1 = anomalous, 0 = normal, -1 = undecided.  mode 0: free text, the abnormal phrases are tried FIRST (so
    'has no defect but is damaged' is anomalous); modes 2 / 3: three- / four-way multiple choice where the last
    letter is the 'normal' option (summary_results.py:8-123)."""
    if mode == 0:
        rules = rules or AnswerRules.default()
        if any(w in text for w in rules.abnormal_words):
            return 1
        if any(w in text for w in rules.normal_words):
            return 0
        return -1
    if mode in (2, 3):
        normal_letter = "C" if mode == 2 else "D"
        if normal_letter in text:
            return 0
        letters = "AB" if mode == 2 else "ABC"
        return 1 if any(f"is {c}." in text for c in letters) else -1
    raise NotImplementedError(f"answer mode {mode}")


def auroc(gt: Sequence[int], score: Sequence[float]) -> float:
    """Area under the ROC curve = Mann-Whitney U / (n_pos * n_neg) with average ranks for ties (what
    sklearn.metrics.roc_auc_score computes for binary labels)."""
    gt = np.asarray(gt)
    score = np.asarray(score, dtype=np.float64)
    n_pos, n_neg = int((gt == 1).sum()), int((gt == 0).sum())
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    order = np.argsort(score, kind="mergesort")
    ranks = np.empty(len(score), dtype=np.float64)
    s = score[order]
    i = 0
    while i < len(s):
        j = i
        while j + 1 < len(s) and s[j + 1] == s[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    return float((ranks[gt == 1].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def scene_performance(records: Iterable[dict], rules: Optional[AnswerRules] = None,
                      score_key: Optional[str] = None) -> Tuple[float, float, float]:
    """(mean accuracy, mean AUROC, mean thresholded accuracy) over scenes (summary_results.py:126-182).
    Undecided answers (-1) are dropped from all three; the threshold is the largest score of a normal sample.
    `score_key` names the record field AUROC and the threshold are taken from ("llm_anomaly_score": the language model's own
    score, make_ad_record's llm_score); the default is the reference's choice, the vision expert's score."""
    rules = rules or AnswerRules.default()
    scenes: Dict[str, Dict[str, list]] = {}
    for r in records:
        pred = classify_answer(r["output"], 0, rules)
        scene = r["scene"] if "scene" in r else r["image_path"].split("/")[1]
        s = scenes.setdefault(scene, {"gt": [], "pred": [], "score": []})
        key = score_key or ("anomaly_map_scores" if "anomaly_map_scores" in r else "anomaly_score")
        if pred != -1:
            s["gt"].append(1 if r["is_anomaly"] else 0)
            s["pred"].append(pred)
            s["score"].append(float(r[key]))
    accs, aucs, th_accs = [], [], []
    for s in scenes.values():
        gt, pred, score = np.array(s["gt"]), np.array(s["pred"]), np.array(s["score"])
        th = score[gt == 0].max()
        accs.append(float((gt == pred).mean()))
        aucs.append(auroc(gt, score))
        th_accs.append(float((gt == (score > th).astype(gt.dtype)).mean()))
    return float(np.mean(accs)), float(np.mean(aucs)), float(np.mean(th_accs))


# ------------------------------------------------------------------------------------------------ localisation metrics
SEG_KEY_BITS = 20


def seg_key(scores) -> np.ndarray:
    """The 20-bit histogram key of fp32 scores (csrc/seg_metrics.hip): -0 counts as +0; the bits of a negative value are all
    flipped, a non-negative one gets its sign bit set (unsigned order of the result = numeric order); the top 20 bits are kept."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    u = np.where(u == np.uint32(0x80000000), np.uint32(0), u)
    t = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return (t >> np.uint32(32 - SEG_KEY_BITS)).astype(np.int64)


def seg_bin_value(keys) -> np.ndarray:
    """The smallest fp32 value of each bin: the transform inverted on key << 12."""
    t = (np.asarray(keys, dtype=np.uint64) << np.uint64(32 - SEG_KEY_BITS)).astype(np.uint32)
    u = np.where(t & np.uint32(0x80000000), t ^ np.uint32(0x80000000), ~t)
    return u.astype(np.uint32).view(np.float32)


def _sk_auc(x: np.ndarray, y: np.ndarray) -> float:
    """sklearn.metrics.auc: the trapezoid area, negated where x decreases; x must be monotone."""
    if x.shape[0] < 2:
        raise ValueError(f"At least 2 points are needed to compute area under curve, but x.shape = {x.shape}")
    dx = np.diff(x)
    direction = 1.0
    if np.any(dx < 0):
        if np.all(dx <= 0):
            direction = -1.0
        else:
            raise ValueError(f"x is neither increasing nor decreasing : {x}.")
    return float(direction * np.sum(dx * (y[1:] + y[:-1]) / 2.0))


def seg_metrics_from_hist(neg, pos, w, n_regions: int, max_step: int = 200, expect_fpr: float = 0.3) -> dict:
    """Pixel AUROC / AP / F1-max and AUPRO of `ALEvaluator.eval_seg` / `cal_pro_score` (scripts/eval_protocol/eval_align.py:
    281-343) from the three histogram rows SegMetrics accumulates: per 20-bit key the count of normal pixels (`neg`), of anomalous
    pixels (`pos`) and the sum over anomalous pixels of floor(2^40 / area of the pixel's ground-truth region) (`w`).  Device-free,
    fp64.  A bin stands for the smallest fp32 value in it, so all four numbers are the reference's formulas applied to the maps
    TRUNCATED to the 20-bit key (exact for non-negative bf16 maps and for fp32 scores that are their bin's smallest member):
      auroc_px  trapezoid over the non-empty bins, descending, a bin being one tied score (roc_auc_score);
      ap_px     sum of (R_n - R_{n-1}) P_n (average_precision_score);
      f1_px     the finite maximum of 2 P R / (P + R) over the bins' thresholds (precision_recall_curve);
      aupro     thresholds np.arange(min, max, (max - min) / max_step) on the fp32 extremes, strict `>`, per threshold the mean
                over regions of tp_r / area_r = (suffix sum of w) / (n_regions 2^40), within 2^16 / 2^40 = 2^-24 of the exact
                mean (each of a region's <= 2^16 pixels loses less than one unit of 2^-40 to the floor); the points with
                fpr < expect_fpr, their fpr min-max normalised, sklearn's auc.  Where the reference divides by zero (one such
                point, no region) this returns NaN as it does.
    auroc_px_tie_bound = sum_b pos_b neg_b / (2 P N): the AUROC of the unquantised fp32 scores lies within it of auroc_px (only
    the pairs that share a bin can be ordered differently, and each counts 1/2 here).  No such bound is claimed for the others."""
    neg, pos, w = (np.asarray(a, dtype=np.int64).ravel() for a in (neg, pos, w))
    if not (neg.shape == pos.shape == w.shape == (1 << SEG_KEY_BITS,)):
        raise ValueError(f"seg_metrics_from_hist: need three rows of {1 << SEG_KEY_BITS} bins, got {neg.shape} {pos.shape} {w.shape}")
    P, N = int(pos.sum()), int(neg.sum())
    if P == 0 or N == 0:
        raise ValueError(f"seg_metrics_from_hist: {P} anomalous and {N} normal pixels; the metrics need both classes")
    keys = np.nonzero((neg + pos) > 0)[0]
    vals = seg_bin_value(keys)                             # ascending with the key
    nb, pb, wb = neg[keys][::-1], pos[keys][::-1], w[keys][::-1]          # descending score
    tps, fps = np.cumsum(pb).astype(np.float64), np.cumsum(nb).astype(np.float64)
    tpr, fpr = np.concatenate([[0.0], tps / P]), np.concatenate([[0.0], fps / N])
    auroc_px = float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0))
    precision, recall = tps / (tps + fps), tps / P
    ap_px = float(np.sum(np.diff(np.concatenate([[0.0], recall])) * precision))
    with np.errstate(divide="ignore", invalid="ignore"):
        f1 = (2 * precision * recall) / (precision + recall)
    f1_px = float(np.max(f1[np.isfinite(f1)]))
    tie_bound = float(np.sum(pb.astype(np.float64) * nb.astype(np.float64)) / (2.0 * P * N))

    # cal_pro_score.  Suffix sums over ascending bins: s[i] = total of the bins i.. ; "score > th" = the bins whose value > th
    min_th, max_th = vals[0], vals[-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = (max_th - min_th) / max_step
        ths = np.arange(min_th, max_th, delta)
        first = np.searchsorted(vals.astype(np.float64), ths.astype(np.float64), side="right")
        suf_neg = np.concatenate([np.cumsum(nb)[::-1], [0]])
        suf_w = np.concatenate([np.cumsum(wb)[::-1], [0]])
        pros = suf_w[first].astype(np.float64) / (float(n_regions) * float(1 << 40)) if n_regions else np.full(len(ths), np.nan)
        fprs = suf_neg[first].astype(np.float64) / N
        keep = fprs < expect_fpr
        fprs = fprs[keep]
        fprs = (fprs - fprs.min()) / (fprs.max() - fprs.min())
        aupro = _sk_auc(fprs, pros[keep])
    return {"auroc_px": auroc_px, "ap_px": ap_px, "f1_px": f1_px, "aupro": aupro, "auroc_px_tie_bound": tie_bound,
            "n_pixels": P + N, "n_anomalous": P, "n_regions": int(n_regions)}


SEG_MAX_REGIONS = 1 << 22      # a bin of row 2 holds at most n_regions * 2^40: int64 head-room


def seg_metrics_from_state(hist, counters, max_step: int = 200, expect_fpr: float = 0.3) -> dict:
    """The metrics of an accumulated SegMetrics state: hist [3, 2^20] int64 (rows neg / pos / w of seg_metrics_from_hist),
    counters [4] int64 (pixels, anomalous pixels, regions, non-finite scores).  ValueError where the state cannot be scored."""
    hist, counters = np.asarray(hist, dtype=np.int64), np.asarray(counters, dtype=np.int64).ravel()
    if hist.shape != (3, 1 << SEG_KEY_BITS) or counters.shape != (4,):
        raise ValueError(f"seg metrics state: need hist {(3, 1 << SEG_KEY_BITS)} and 4 counters, got {hist.shape} {counters.shape}")
    n_pix, n_pos, n_reg, n_bad = (int(c) for c in counters)
    if n_bad:
        raise ValueError(f"seg metrics: {n_bad} of {n_pix} scores were NaN or infinite; they are in no histogram row")
    if n_pos == 0 or n_pix - n_pos == 0:
        raise ValueError(f"seg metrics: {n_pos} anomalous and {n_pix - n_pos} normal pixels; the metrics need both classes")
    if n_reg >= SEG_MAX_REGIONS:
        raise ValueError(f"seg metrics: {n_reg} regions >= 2^22: the region-weighted row may have overflowed int64")
    return seg_metrics_from_hist(hist[0], hist[1], hist[2], n_reg, max_step, expect_fpr)


def merge_seg_shards(paths: Sequence[str], out_path: Optional[str] = None, max_step: int = 200, expect_fpr: float = 0.3) -> dict:
    """Add the per-rank `.seg.rankK.npz` states of a sharded evaluation (integer sums: any order gives the same bits) and score
    the total; `out_path`: where to write the metrics as json."""
    hist, counters = None, None
    for p in paths:
        with np.load(p) as z:
            h, c = z["hist"].astype(np.int64), z["counters"].astype(np.int64)
        hist, counters = (h, c) if hist is None else (hist + h, counters + c)
    if hist is None:
        raise ValueError("merge_seg_shards: no shard given")
    res = seg_metrics_from_state(hist, counters, max_step, expect_fpr)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f)
    return res


# ------------------------------------------------------------------------------------------------ records
def postprocess_generation(token_ids, tokenizer) -> List[str]:
    """evaluation_aqa_dataset.py:339-341, 369: ids clamped to [1, 40000], decoded, cut at the first '###'."""
    import torch
    ids = torch.clamp(torch.as_tensor(token_ids), 1, 40000)
    return [t.split("###")[0] for t in tokenizer.batch_decode(ids, add_special_tokens=False)]


def make_ad_record(image_id: int, img_path: str, is_anomaly: bool, output_text: str,
                   anomaly_map_max: Optional[float] = None, llm_score: Optional[float] = None) -> dict:
    """One jsonl line for the 'ad' / '1cls' / 'shot' task types (evaluation_aqa_dataset.py:361-384).  `output_text`
    is already cut at '###'; `anomaly_map_max` is the maximum of the 0..255 expert map.  `llm_score` (an addition of this build,
    absent by default) is the language model's own anomaly score p(Yes) / (p(Yes) + p(No)) at the first generated token, written
    as "llm_anomaly_score" in the format of "anomaly_score"."""
    item = {"image_id": int(image_id), "image_path": "/".join(img_path.split("/")[-5:]), "is_anomaly": bool(is_anomaly)}
    if anomaly_map_max is not None:
        ok = ("Yes" in output_text and bool(is_anomaly)) or ("No" in output_text and not bool(is_anomaly))
        item["error"] = "0" if ok else "1"
        item["output"] = output_text
        item["anomaly_score"] = str(round(float(anomaly_map_max) / 255.0, 4))
    if llm_score is not None:
        item["llm_anomaly_score"] = str(round(float(llm_score), 4))
    return item


def llm_anomaly_score(watch_logprobs_first) -> float:
    """p_yes / (p_yes + p_no) from the first token step's log-probs of the (Yes, No) ids (generate(output_scores=True,
    watch_ids=[yes, no])["watch_logprobs"][row, 0]): the softmax over the two, taken in float64."""
    ly, ln = (float(v) for v in watch_logprobs_first[:2])
    if ly == ln:                                         # also both -inf
        return 0.5
    with np.errstate(over="ignore"):
        return float(1.0 / (1.0 + np.exp(np.float64(ln) - np.float64(ly))))


def answer_anomaly_score(logprobs_row) -> float:
    """The softmax over the candidates' log-likelihoods at index 0 (MyriadHIP.score_answers' "answer_logprobs"[row]): for the
    default pair [ABNORMAL_DESCRIBE, NORMAL_DESCRIBE] p_abn / (p_abn + p_nor) with whole answers in the place of
    llm_anomaly_score's first tokens.  Taken in float64 from the sums; a -inf entry counts as probability 0, all entries equal
    (all -inf included) give 1 / C."""
    lp = np.asarray([float(v) for v in logprobs_row], dtype=np.float64)
    if lp.size == 0:
        raise ValueError("answer_anomaly_score: no candidates")
    m = lp.max()
    if not np.isfinite(m) or bool((lp == m).all()):
        return 1.0 / lp.size
    e = np.exp(lp - m)
    return float(e[0] / e.sum())


def add_answer_ranking(record: dict, logprobs_row, best_text: str) -> dict:
    """eval_aqa.py --rank-answers: "llm_answer_score" = answer_anomaly_score in the format of "anomaly_score" and
    "ranked_output", the best candidate's text, joined to a record."""
    record["llm_answer_score"] = str(round(answer_anomaly_score(logprobs_row), 4))
    record["ranked_output"] = best_text
    return record


def write_jsonl(path: str, records: Iterable[dict]) -> None:
    with open(path, "w") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")


def read_jsonl(path: str) -> List[dict]:
    return [json.loads(l) for l in open(path) if l.strip()]


# ------------------------------------------------------------------------------------------------ multi-GPU eval
def shard_indices(n: int, rank: int, world: int) -> List[int]:
    """Replicas only: rank r evaluates samples r, r+world, ... ; no collective on the data path."""
    return list(range(rank, n, world))


def merge_shards(paths: Sequence[str], out_path: str) -> int:
    """Concatenate the per-rank jsonl files and restore dataset order (image_id)."""
    recs = [r for p in paths for r in read_jsonl(p)]
    recs.sort(key=lambda r: r["image_id"])
    write_jsonl(out_path, recs)
    return len(recs)


# ------------------------------------------------------------------------------------------------ summary table
def summarize_result_dir(result_path: str, rules: Optional[AnswerRules] = None) -> List[str]:
    """`summary_v2.txt` rows (summary_results.py:185-245): one row per checkpoint ordinal parsed from
    `<prefix>_ckpt<N>_...jsonl`, columns 1cls / 1shot / 2shot / 4shot accuracy then the same four AUROCs.
    With several files for one cell the reference scores the FIRST file each time (`f_names[0]` inside its loop);
    that is kept so the table is identical."""
    files: Dict[int, Dict[str, List[str]]] = {}
    for f in sorted(os.listdir(result_path)):
        if not f.endswith("jsonl"):
            continue
        k = int(f.split("_")[1].replace("ckpt", ""))
        cell = files.setdefault(k, {"1cls": [], "1shot": [], "2shot": [], "4shot": []})
        if "1cls" in f:
            cell["1cls"].append(f)
        else:
            few = int(f.split("kshot=")[-1].split("_")[0])
            cell[f"{few}shot"].append(f)
    order = ["1cls", "1shot", "2shot", "4shot"]
    rows = ["Head 1cls(Myriad) 1shot(Myriad) 2shot(Myriad) 4shot(Myriad)   1cls(Expert) 1shot(Expert) 2shot(Expert) 4shot(Expert)"]
    for k in sorted(files):
        rec = {}
        for proc, names in files[k].items():
            rec[proc] = ["-", "-"]
            if names:
                try:
                    acc, auc, _ = scene_performance(read_jsonl(os.path.join(result_path, names[0])), rules)
                    rec[proc] = [f"{acc:.4f}", f"{auc:.4f}"]
                except Exception:
                    pass
        rows.append(f"{k:03d} " + "{} {} {} {}   {} {} {} {}".format(*([rec[p][0] for p in order] + [rec[p][1] for p in order])))
    return rows
