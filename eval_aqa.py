#!/usr/bin/env python3
"""AQA evaluation entry point: counterpart of the reference's evaluation_aqa_dataset.py (:40-62, 233-390) for the
task types that script can actually run (`1cls`, `shot`: the other dataset classes are never imported there).

    python eval_aqa.py --cfg-path eval_configs/myriad.yaml --task_type 1cls --split mvtec --bs 4 [--ckpt 9] [--k_shot 0]

Same flow: Config -> model_cls.from_config(model_cfg) on cuda:{gpu-id} -> DataLoader(bs) -> model.generate(samples,
max_new_tokens=90, stopping_criteria=[###], do_sample=True, top_p=0.01, temperature=1.0, min_length=1, use_cache=True)
-> ids clamped to [1, 40000] -> batch_decode -> one jsonl record per sample (image_id, image_path, is_anomaly, error,
output, anomaly_score) -> memory / mean latency.  `--world/--rank` shard the test set by index for multi-GPU runs
(replicas only: no collective on the data path; merge with myriad_amd.eval_protocol.merge_shards).
`--seg-metrics` also scores the expert's anomaly maps against the ground-truth masks on the device (myriad_amd.seg_metrics:
pixel AUROC / AP / F1-max, AUPRO) and writes `<result>.seg.json`, or with --world > 1 the rank's state `<result>.seg.rankK.npz`
(merge with myriad_amd.eval_protocol.merge_seg_shards).
"""
import argparse
import os
import sys
import time
from datetime import datetime

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ANNO_FILES = {"1cls": {"visa": "DC_VISA_test_normal.jsonl", "mvtec": "DC_MVTEC_test_normal.jsonl"},
              "shot": {"visa": "DC_VISA_test_normal.jsonl", "mvtec": "DC_MVTEC_test_normal.jsonl"}}
ROOTS = {"visa": "./data/EvalADDataset", "mvtec": "./data/EvalADDataset"}


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Demo")
    parser.add_argument("--cfg-path", required=True, help="path to configuration file.")
    parser.add_argument("--gpu-id", type=int, default=0, help="specify the gpu to load the model.")
    parser.add_argument("--task_type", type=str, default="1cls", choices=["1cls", "shot"])
    parser.add_argument("--split", type=str, default="mvtec", choices=["visa", "mvtec"])
    parser.add_argument("--ckpt", type=int, default=-1)
    parser.add_argument("--bs", type=int, default=1)
    parser.add_argument("--round_index", type=int, default=14)
    parser.add_argument("--k_shot", type=int, default=0)
    parser.add_argument("--start", type=int, default=0)
    parser.add_argument("--options", nargs="+")
    # additions of this build (the reference derives the output path from the checkpoint path and runs one process)
    parser.add_argument("--out", type=str, default=None, help="result jsonl (default: next to the checkpoint, reference naming)")
    parser.add_argument("--dataset", type=str, default="anomaly_detection", help="dataset builder (tests use 'synthetic')")
    parser.add_argument("--world", type=int, default=1)
    parser.add_argument("--rank", type=int, default=0)
    parser.add_argument("--limit", type=int, default=0, help="evaluate only the first N batches (smoke runs)")
    parser.add_argument("--slots", type=int, default=0, help="N > 0: stream the test set through N decode slots "
                        "(model.generate_stream: per-sample positions and stop rule); 0: one generate() per batch")
    parser.add_argument("--num-beams", type=int, default=1, help="N > 1: beam search with N beams instead of the evaluation "
                        "script's sampling (num_beams=N, do_sample=False), in either loop; with --slots the slot count must be a "
                        "multiple of N and beam search in the decode slots needs its switch, MYRIAD_SLOT_BEAMS=1")
    parser.add_argument("--beam-sample", action="store_true", help="with --num-beams N: keep the evaluation script's do_sample=True "
                        "with its top_p / temperature (beam-search multinomial sampling, the reference chat call's mode) instead of "
                        "deterministic beams, in either loop; needs the beam sampling switch, MYRIAD_BEAM_SAMPLING=1")
    parser.add_argument("--repetition-penalty", type=float, default=1.0, help="with --num-beams N: repetition_penalty of the "
                        "beam search, in either loop; needs the beam sampling switch, MYRIAD_BEAM_SAMPLING=1")
    parser.add_argument("--prefill-batch", type=int, default=1, help="with --slots: P > 1 prefills up to P waiting samples in one "
                        "packed pass when slots are free (1: every sample is prefilled alone)")
    parser.add_argument("--refill-min", type=int, default=1, help="with --slots: hold a refill back until this many slots are free "
                        "(fuller packed passes at the price of occupancy)")
    parser.add_argument("--llm-score", action="store_true", help="also write llm_anomaly_score = p(Yes) / (p(Yes) + p(No)) at the "
                        "first generated token (generate(output_scores=True): the language model's own anomaly score)")
    parser.add_argument("--rank-answers", action="store_true", help="also rank the two trained answers by log-likelihood "
                        "(model.score_answers, nothing decoded): llm_answer_score = p(abnormal answer) / (p(abnormal) + p(normal)) "
                        "and ranked_output = the likelier answer's text")
    parser.add_argument("--rank-only", action="store_true", help="--rank-answers without generation: output is the likelier "
                        "answer's text")
    parser.add_argument("--seg-metrics", action="store_true", help="also score ve_anomaly_maps against the dataset's gt_mask: "
                        "pixel AUROC / AP / F1-max and AUPRO, accumulated on the device; writes <result>.seg.json "
                        "(--world > 1: <result>.seg.rankK.npz, to be merged with eval_protocol.merge_seg_shards)")
    parser.add_argument("--draft-k", type=int, default=0, help="K > 1: draft-and-verify greedy decoding with K rows per verify "
                        "step (--bs 1, or --slots N with N * K <= 64 and the switch MYRIAD_SLOT_DRAFT=1): an n-gram drafter that observes every finished answer guesses K - 1 tokens, "
                        "one token step verifies them; the records are those of the run without it (with --llm-score behind the switch "
                        "MYRIAD_DRAFT_SAMPLING=1)")
    parser.add_argument("--draft-corpus", type=str, default=None, help="with --draft-k: teach the drafter up front from a results "
                        ".jsonl of an earlier run (its `output` texts are tokenised) or a JSON list of id lists")
    parser.add_argument("--seg-max-step", type=int, default=200, help="with --seg-metrics: thresholds of the PRO curve")
    parser.add_argument("--seg-expect-fpr", type=float, default=0.3, help="with --seg-metrics: the PRO curve is cut at this FPR")
    args = parser.parse_args(argv)
    args.rank_answers = args.rank_answers or args.rank_only
    if args.beam_sample and args.num_beams <= 1:
        parser.error("--beam-sample needs --num-beams N > 1")
    if args.repetition_penalty != 1.0 and args.num_beams <= 1:
        parser.error("--repetition-penalty needs --num-beams N > 1")
    if args.draft_corpus and not args.draft_k:
        parser.error("--draft-corpus needs --draft-k K")
    if args.draft_k and (args.draft_k < 1 or args.draft_k > 8):
        parser.error(f"--draft-k takes 1 to 8 rows, got {args.draft_k}")
    # --llm-score with --draft-k: the verify step writes the token scores behind the switch MYRIAD_DRAFT_SAMPLING=1
    if args.draft_k and (args.num_beams > 1 or (args.llm_score and os.environ.get("MYRIAD_DRAFT_SAMPLING", "0") == "0")):
        parser.error("--draft-k is greedy decoding: it takes no --num-beams, --beam-sample, --repetition-penalty or --llm-score")
    if args.draft_k and args.slots <= 0 and args.bs != 1:
        parser.error("--draft-k without --slots decodes one sequence at a time: it needs --bs 1")
    if args.draft_k and args.slots > 0 and os.environ.get("MYRIAD_SLOT_DRAFT", "0") == "0":
        parser.error("--draft-k with --slots: draft decoding in the decode slots needs its switch, MYRIAD_SLOT_DRAFT=1")
    if args.draft_k and args.slots * args.draft_k > 64:
        parser.error(f"--slots {args.slots} --draft-k {args.draft_k}: the verify step holds slots x K rows, at most 64")
    if not args.seg_metrics and (args.seg_max_step != 200 or args.seg_expect_fpr != 0.3):
        parser.error("--seg-max-step / --seg-expect-fpr need --seg-metrics")
    if args.seg_max_step < 1:
        parser.error(f"--seg-max-step must be at least 1, got {args.seg_max_step}")
    if not 0.0 < args.seg_expect_fpr <= 1.0:
        parser.error(f"--seg-expect-fpr must lie in (0, 1], got {args.seg_expect_fpr}")
    return args


def seg_paths(save_path: str, world: int = 1, rank: int = 0):
    """(metrics json, state npz or None) next to the result file: <result>.seg.json; a rank of a sharded run writes its state
    <result>.seg.rankK.npz instead (<result>: the jsonl path without the suffix and without the rank's own `.rankK`)."""
    stem = save_path[:-6] if save_path.endswith(".jsonl") else save_path
    if world > 1:
        if stem.endswith(f".rank{rank}"):
            stem = stem[:-len(f".rank{rank}")]
        return None, f"{stem}.seg.rank{rank}.npz"
    return f"{stem}.seg.json", None


def seg_gt(data_sample):
    """The batch's ground-truth masks; a dataset that yields none is an error."""
    if "gt_mask" not in data_sample:
        raise KeyError("--seg-metrics: the dataset yields no 'gt_mask' (set with_gt_mask: True in its config; "
                       f"the samples have {sorted(data_sample)})")
    return data_sample["gt_mask"]


def seg_update(seg, maps, gt_mask, device):
    """Feed maps and their masks to the accumulator; a model without expert maps is an error."""
    if maps is None:
        raise KeyError("--seg-metrics: the model returned no ve_anomaly_maps (no vision expert output to score)")
    seg.update(maps.detach().to(device), gt_mask)


def seg_finish(seg, args, save_path):
    import json
    json_path, npz_path = seg_paths(save_path, args.world, args.rank)
    if npz_path:
        seg.save(npz_path)
        print(f"Segmentation-metric state saved to {npz_path}")
        return None
    res = seg.compute(max_step=args.seg_max_step, expect_fpr=args.seg_expect_fpr)
    with open(json_path, "w") as f:
        json.dump(res, f)
    print("Segmentation metrics:", res, "->", json_path)
    return res


def llm_watch_ids(tokenizer):
    """The ids the training labels teach as the answer's first token: (Yes, No) of ABNORMAL_DESCRIBE / NORMAL_DESCRIBE."""
    from myriad_amd import datasets as D
    return [int(tokenizer(t, add_special_tokens=False).input_ids[0]) for t in (D.ABNORMAL_DESCRIBE, D.NORMAL_DESCRIBE)]


def rank_texts():
    """The candidates of --rank-answers, score_answers' default: index 0 is the abnormal answer."""
    from myriad_amd import datasets as D
    return [D.ABNORMAL_DESCRIBE, D.NORMAL_DESCRIBE]


def main(argv=None):
    import torch
    from torch.utils.data import DataLoader, Subset
    from myriad_amd import myriad  # noqa: F401
    from myriad_amd import datasets as D
    from myriad_amd import eval_protocol as EP
    from myriad_amd.config import Config
    from myriad_amd.myriad import StoppingCriteriaSub
    from myriad_amd.registry import registry
    from myriad_amd.runner import setup_seeds

    args = parse_args(argv)
    cfg = Config(args)
    setup_seeds(int(cfg.run_cfg.get("seed", 42)), 0)
    model_config = cfg.model_cfg
    model_config["round_index"] = args.round_index
    model_config["k_shot"] = args.k_shot
    if args.ckpt != -1:                                  # evaluation_aqa_dataset.py:245-249
        parts = model_config["ckpt"].split("/")
        parts[-1] = f"checkpoint_{args.ckpt}.pth"
        model_config["ckpt"] = "/".join(parts)
    model_config["device_8bit"] = args.gpu_id
    model_config["device"] = f"cuda:{args.gpu_id}"
    model_config["need_backward"] = False                # no dgrad copies of the frozen weights for an evaluation run
    model_cls = registry.get_model_class(model_config.arch)
    model = model_cls.from_config(model_config).to("cuda:{}".format(args.gpu_id))

    stop_words_ids = [torch.tensor([835]).to(model.device), torch.tensor([2277, 29937]).to(model.device)]   # '###', two encodings
    stopping_criteria = [StoppingCriteriaSub(stops=stop_words_ids)]
    if args.dataset == "synthetic":
        dcfg = dict(cfg.datasets_cfg.get("synthetic", {}) or {})
        if args.seg_metrics:
            dcfg["with_gt_mask"] = True
        ds = D.build_datasets({"synthetic": dcfg}, split="test")["synthetic"]
    else:
        dcfg = dict(cfg.datasets_cfg.get("anomaly_detection", {}) or {})
        if args.seg_metrics:
            dcfg["with_gt_mask"] = True
        dcfg["build_info"] = {"vis_root": ROOTS[args.split], "ann_paths": [ANNO_FILES[args.task_type][args.split]]}
        ds = D.build_datasets({"anomaly_detection": dcfg}, split="test")["anomaly_detection"]
    if args.world > 1:
        ds = Subset(ds, EP.shard_indices(len(ds), args.rank, args.world))
    loader = DataLoader(ds, batch_size=args.bs, num_workers=0, collate_fn=D.collate)

    ckpt_name = os.path.splitext(os.path.basename(model_config.get("ckpt", "") or "checkpoint_0.pth"))[0]
    num_ckpt = ckpt_name.split("_")[-1]
    prefix = (f"results_ckpt{num_ckpt}_training={args.task_type}_split={args.split}_kshot={args.k_shot}_roundindex={args.round_index}_"
              f"{datetime.now().strftime('%Y%m%d_%H%M')}")
    save_path = args.out or os.path.join(os.path.dirname(model_config.get("ckpt", "") or "."), f"{prefix}.jsonl")
    if args.world > 1 and args.out is None:
        save_path = save_path[:-6] + f".rank{args.rank}.jsonl"
    print(f"Results will be saved to {save_path}")
    generate_kwargs = {"max_new_tokens": 90, "stopping_criteria": stopping_criteria, "do_sample": True, "use_cache": True,
                       "min_length": 1, "top_p": 0.01, "temperature": 1.0}           # evaluation_aqa_dataset.py:289-301

    if args.num_beams > 1:
        generate_kwargs.update(num_beams=args.num_beams, do_sample=bool(args.beam_sample))
        if args.repetition_penalty != 1.0:
            generate_kwargs.update(repetition_penalty=args.repetition_penalty)
    if args.llm_score:
        generate_kwargs.update(output_scores=True, watch_ids=llm_watch_ids(model.llama_tokenizer))

    drafter = None
    if args.draft_k:
        from myriad_amd.decode_host import NgramDrafter, load_draft_corpus
        corpus = ()
        if args.draft_corpus:
            corpus = load_draft_corpus(args.draft_corpus, lambda t: model.llama_tokenizer(t, add_special_tokens=False).input_ids)
        drafter = NgramDrafter(corpus)
        generate_kwargs.update(draft=drafter, draft_k=args.draft_k)

    model.eval()
    seg = None
    if args.seg_metrics:
        from myriad_amd.seg_metrics import SegMetrics
        seg = SegMetrics(model.device)
    if args.slots > 0 and not args.rank_only:
        return save_path, _run_slots(args, model, loader, generate_kwargs, save_path, seg)
    records, all_time, sampled = [], 0.0, 0
    draft_stats = dict(steps=0, verify_steps=0, plain_steps=0, draft_proposed=0, draft_accepted=0)
    for testid, data_sample in enumerate(loader):
        if testid < args.start:
            continue
        if args.limit and testid >= args.start + args.limit:
            break
        with torch.no_grad():
            t1 = time.time()
            ranked = model.score_answers(data_sample) if args.rank_answers else None
            outputs = ranked if args.rank_only else model.generate(data_sample, **generate_kwargs)
            torch.cuda.synchronize()
            all_time += time.time() - t1
        if args.rank_only:                               # nothing was generated: the likelier answer is the output
            texts = [rank_texts()[int(b)] for b in ranked["best"]]
        else:
            sampled += model.last_generate_stats.get("sampled_rows", 0)     # a beam search draws nothing
            if drafter is not None:                      # the run warms itself: every finished answer teaches the drafter
                drafter.observe(outputs["token_ids"][0].tolist())
                for k in draft_stats:
                    draft_stats[k] += model.last_generate_stats.get(k, 0)
            texts = EP.postprocess_generation(outputs["token_ids"], model.llama_tokenizer)
        maps = outputs.get("ve_anomaly_maps")
        if seg is not None:
            seg_update(seg, maps, seg_gt(data_sample), model.device)
        for ind, text in enumerate(texts):
            amax = None
            if maps is not None:                         # anomaly_map_handler (:93-104): uint8(map * 255) then max
                amax = float((maps[ind].detach().float().cpu() * 255.0).to(torch.uint8).max())
            llm = EP.llm_anomaly_score(outputs["watch_logprobs"][ind, 0]) if args.llm_score and not args.rank_only else None
            records.append(EP.make_ad_record(int(data_sample["image_id"][ind]), data_sample["img_path"][ind],
                                             bool(data_sample["is_anomaly"][ind]), text, amax, llm))
            if ranked is not None:
                EP.add_answer_ranking(records[-1], ranked["answer_logprobs"][ind], rank_texts()[int(ranked["best"][ind])])
    EP.write_jsonl(save_path, records)
    if seg is not None:
        seg_finish(seg, args, save_path)
    n_batches = max(1, len(records) // max(1, args.bs))
    print("CUDA Memory:", torch.cuda.max_memory_allocated() / (1024 * 1024))
    print("Mean Time: ", all_time / n_batches)
    if sampled:
        print(f"note: {sampled} generated tokens had p_max < top_p and were drawn, not arg-maxed (see LlamaHIP.greedy_generate)")
    if drafter is not None:
        print(f"draft-and-verify (K = {args.draft_k}): {draft_stats['steps']} tokens in {draft_stats['verify_steps']} verify + "
              f"{draft_stats['plain_steps']} plain steps, {draft_stats['draft_accepted']} of {draft_stats['draft_proposed']} guesses kept")
    return save_path, records


def _run_slots(args, model, loader, generate_kwargs, save_path, seg=None):
    """The evaluation loop over model.generate_stream: the same records, in the dataset's order."""
    import torch
    from myriad_amd import eval_protocol as EP

    meta, ranks = [], []                                 # per sample, in input order: what its record needs besides the text
    gt = {}                                              # --seg-metrics: a sample's ground-truth mask until its map arrives

    def batches():
        for testid, data_sample in enumerate(loader):
            if testid < args.start:
                continue
            if args.limit and testid >= args.start + args.limit:
                break
            for ind in range(len(data_sample["image_id"])):
                if seg is not None:
                    gt[len(meta)] = seg_gt(data_sample)[ind:ind + 1]
                meta.append((int(data_sample["image_id"][ind]), data_sample["img_path"][ind], bool(data_sample["is_anomaly"][ind])))
            if args.rank_answers:                        # between two token steps of the stream: a pass of its own caches
                r = model.score_answers(data_sample)
                ranks.extend((r["answer_logprobs"][ind], int(r["best"][ind])) for ind in range(len(data_sample["image_id"])))
            yield data_sample

    records = []
    drafter = generate_kwargs.get("draft")
    with torch.no_grad():
        t1 = time.time()
        for out in model.generate_stream(batches(), slots=args.slots, prefill_batch=args.prefill_batch, refill_min=args.refill_min,
                                         **generate_kwargs):
            text = EP.postprocess_generation(out["token_ids"][None], model.llama_tokenizer)[0]
            if drafter is not None:                      # the run warms itself: every finished answer teaches the drafter
                drafter.observe(out["token_ids"].tolist())
            amax = None
            if seg is not None:
                m = out["ve_anomaly_map"]
                seg_update(seg, None if m is None else m.reshape(1, *m.shape[-2:]), gt.pop(out["index"]), model.device)
            if out["ve_anomaly_map"] is not None:        # anomaly_map_handler (:93-104): uint8(map * 255) then max
                amax = float((out["ve_anomaly_map"].detach().float().cpu() * 255.0).to(torch.uint8).max())
            llm = EP.llm_anomaly_score(out["watch_logprobs"][0]) if args.llm_score else None
            records.append(EP.make_ad_record(*meta[out["index"]], text, amax, llm))
            if args.rank_answers:
                lp, best = ranks[out["index"]]
                EP.add_answer_ranking(records[-1], lp, rank_texts()[best])
        torch.cuda.synchronize()
        all_time = time.time() - t1
    EP.write_jsonl(save_path, records)
    if seg is not None:
        seg_finish(seg, args, save_path)
    st = model.last_generate_stats
    n_batches = max(1, len(records) // max(1, args.bs))
    print("CUDA Memory:", torch.cuda.max_memory_allocated() / (1024 * 1024))
    print("Mean Time: ", all_time / n_batches, f" decode slots {args.slots}: occupancy {st.get('occupancy', 0.0):.3f} over "
          f"{st.get('steps', 0)} token steps, {st.get('prefills', 0)} prefills in {st.get('prefill_passes', 0)} passes")
    if st.get("host_sampled_rows"):
        print(f"note: {st['host_sampled_rows']} generated tokens had p_max < top_p and were drawn, not arg-maxed "
              "(see LlamaHIP.greedy_generate)")
    if drafter is not None:
        print(f"draft-and-verify (K = {args.draft_k}): {st.get('emitted', 0) + st.get('prefills', 0)} tokens in "
              f"{st.get('verify_steps', 0)} verify + {st.get('plain_steps', 0)} plain steps, {st.get('draft_accepted', 0)} of "
              f"{st.get('draft_proposed', 0)} guesses kept")
    return records


if __name__ == "__main__":
    main()
