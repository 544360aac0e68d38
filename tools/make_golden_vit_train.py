"""Write tests/golden/vit_param_order.json from the REFERENCE's own EVA ViT (build container only).

With freeze_vit: False the reference trains every parameter of `visual_encoder` and `ln_vision` (myriad.py:134-144).  Their
named_parameters() order -- visual_encoder is the first child module the model registers (myriad.py:108), ln_vision the second --
is the order of the optimiser state inside a checkpoint_N.pth (runner_base.py:110-119); the file lists it for a 3-block ViT,
so checkpoint.reference_param_order can be checked against the reference module itself.  Names only: no weights.

    python tools/make_golden_vit_train.py [--ref PATH]
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
    import torch
    depth = 3
    vit = mg.ref_vit(M, 64, depth, 4, 4.3637, 28)
    ln_vision = torch.nn.LayerNorm(64)                     # blip2.py:119-125: a plain LayerNorm of the ViT's width
    names = ["visual_encoder." + n for n, _ in vit.named_parameters()] + ["ln_vision." + n for n, _ in ln_vision.named_parameters()]
    path = os.path.join(mg.OUT, "vit_param_order.json")
    with open(path, "w") as f:
        json.dump(dict(depth=depth, names=names), f, indent=0)
        f.write("\n")
    print("wrote", path, len(names), "names")


if __name__ == "__main__":
    main()
