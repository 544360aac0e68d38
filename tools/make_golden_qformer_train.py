"""Write tests/golden/qformer_train_param_order.json from the REFERENCE's own Q-Former (build container only).

With freeze_qformer: False the reference trains `query_tokens` and every parameter left in `Qformer` after the surgery of
myriad.py:151-156 (cls, word/position embeddings and the text FFNs deleted).  Their named_parameters() order is the order of
the optimiser state inside a checkpoint_N.pth (runner_base.py:110-119); the file lists it for a 4-layer Q-Former (cross-
attention on layers 0 and 2), so checkpoint.reference_param_order can be checked against the reference module itself.

    python tools/make_golden_qformer_train.py [--ref PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

import make_golden as mg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("MYRIAD_REFERENCE", "reference"))
    a = ap.parse_args()
    M = mg.load_reference(a.ref)
    q = mg.ref_qformer(M, 128, 4, 2, 256, 192, 8)
    names = ["query_tokens"] + ["Qformer." + n for n, _ in q.named_parameters()]
    path = os.path.join(mg.OUT, "qformer_train_param_order.json")
    with open(path, "w") as f:
        json.dump(dict(layers=4, cross_attention_freq=2, names=names), f, indent=0)
        f.write("\n")
    print("wrote", path, len(names), "names")


if __name__ == "__main__":
    main()
