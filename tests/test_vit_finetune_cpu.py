"""freeze_vit: False on the host side (CPU): configuration switches, the ViT + ln_vision parameter set, its weight-decay groups
and flat-buffer layout, the checkpoint's parameter order against the reference module's own listing, and the argument checks
of the master -> working-copy refresh kernel."""
import ctypes
import json
import os

import pytest
import torch

from myriad_amd import checkpoint as C
from myriad_amd import ops
from myriad_amd.eva_vit import vit_param_shapes, vit_param_specs
from myriad_amd.myriad import MODULE_ORDER, MODULES, MiniGPT4HIP, MyriadHIP, ParamStore, module_of, uses_weight_decay
from myriad_amd.qformer import qformer_param_specs
from myriad_amd.synthetic import full_config, shape_table

G = os.path.join(os.path.dirname(__file__), "golden")


class _Reached(Exception):
    pass


def _spy(cls, monkeypatch):
    def reached(*a, **k):
        raise _Reached()
    monkeypatch.setattr(ops, "ensure_workspace", reached)          # the first device step of the constructor
    seen = {}
    orig_init = cls.__init__

    def spy(self, weights, cfg=None, device="cuda:0"):
        seen.clear()
        seen.update(cfg)
        return orig_init(self, weights, cfg, device)
    monkeypatch.setattr(cls, "__init__", spy)
    return seen


@pytest.mark.parametrize("cls", [MyriadHIP, MiniGPT4HIP])
def test_from_config_accepts_a_trainable_fp32_vit(cls, monkeypatch):
    base = dict(weights={}, device="cuda:0")
    seen = _spy(cls, monkeypatch)
    with pytest.raises(_Reached):
        cls.from_config(dict(base, freeze_vit=False, vit_precision="fp32"))
    assert seen["freeze_vit"] is False and "use_grad_checkpoint" not in seen
    with pytest.raises(_Reached):
        cls.from_config(dict(base, freeze_vit=False, vit_precision="fp32", use_grad_checkpoint=True))
    assert seen["freeze_vit"] is False and seen["use_grad_checkpoint"] is True
    with pytest.raises(_Reached):                                  # together with the Q-Former
        cls.from_config(dict(base, freeze_vit=False, vit_precision="fp32", freeze_qformer=False))
    assert seen["freeze_vit"] is False and seen["freeze_qformer"] is False


@pytest.mark.parametrize("cls", [MyriadHIP, MiniGPT4HIP])
def test_from_config_refusals(cls, monkeypatch):
    base = dict(weights={}, device="cuda:0")
    _spy(cls, monkeypatch)
    for extra in ({}, dict(vit_precision="fp16")):                 # the reference's default precision is fp16
        with pytest.raises(NotImplementedError) as e:
            cls.from_config(dict(base, freeze_vit=False, **extra))
        assert "freeze_vit" in str(e.value) and "vit_precision" in str(e.value) and "fp32" in str(e.value)
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        cls.from_config(dict(base, freeze_vit=False, vit_precision="fp32", drop_path_rate=0.1))
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        cls.from_config(dict(base, drop_path_rate=0.1))
    with pytest.raises(NotImplementedError, match="use_grad_checkpoint"):
        cls.from_config(dict(base, use_grad_checkpoint=True))      # frozen ViT: as before
    with pytest.raises(NotImplementedError, match="freeze_llama"):
        cls.from_config(dict(base, freeze_vit=False, vit_precision="fp32", freeze_llama=False))


def _vit_specs(depth=3, D=64, hidden=279, n_tok=5):
    shapes = vit_param_shapes(D, 3, 14, n_tok, [hidden] * depth)
    return vit_param_specs(shapes) + [("ln_vision.weight", (D,), (D,)), ("ln_vision.bias", (D,), (D,))]


def test_param_store_modules_groups_and_runs():
    specs = _vit_specs()
    # the two new modules come behind every earlier one
    assert MODULE_ORDER == MODULES + ("visual_encoder", "ln_vision") and MODULES[-1] == "Qformer"
    adaptor = [("expert_adaptor.conv1.weight", (4, 64), (4, 64)), ("expert_adaptor.conv2.weight", (64, 4), (64, 4))]
    st = ParamStore(specs[::-1] + adaptor, "cpu")                  # any order in: module order out
    assert st.modules == ["expert_adaptor", "visual_encoder", "ln_vision"]
    for n, _, r in specs:
        decays = uses_weight_decay(n, len(r))
        mod = module_of(n)
        assert mod == ("ln_vision" if n.startswith("ln_vision.") else "visual_encoder")
        if n.endswith(("cls_token", "pos_embed", "qkv.weight", "proj.weight", "fc1.weight", "fc2.weight")):
            assert decays, n                                       # matrices, and the 3-D cls_token / pos_embed
        else:
            assert not decays, n                                   # biases, q_bias / v_bias, the norms, ln_vision
        o, k = st.offsets[n]
        a, b = st.module_range(mod, decays)
        assert a <= o and o + k <= b and (o >= st.n_wd) == (not decays)
        assert o % 4 == 0                                          # 16-byte aligned: the refresh kernel's vector loads
    # each module has one contiguous run per group, and the runs tile the buffer in module order
    runs = [(st.modules[mi], a, b, d) for mi, a, b, d in st.ranges]
    assert [(m, d) for m, _, _, d in runs] == [("expert_adaptor", True), ("visual_encoder", True), ("visual_encoder", False),
                                               ("ln_vision", False)]
    assert all(runs[i][2] == runs[i + 1][1] for i in range(len(runs) - 1)) and runs[0][1] == 0 and runs[-1][2] == st.n_used
    assert st.module_range("ln_vision", True) is None
    assert st.total % 32 == 0                                      # reduce-scatter shards of 4-element multiples at 2 / 4 / 8 ranks


def test_q_bias_v_bias_are_adjacent_and_blocks_evenly_spaced():
    st = ParamStore(_vit_specs(depth=3), "cpu")
    off = []
    for i in range(3):
        b = f"visual_encoder.blocks.{i}.attn."
        (oq, nq), (ov, _) = st.offsets[b + "q_bias"], st.offsets[b + "v_bias"]
        assert ov == oq + nq
        off.append(oq)
    assert off[1] - off[0] == off[2] - off[1]


def test_earlier_recipes_keep_their_layout():
    frozen = [("expert_adaptor.conv1.weight", (4, 192), (4, 192)), ("VETokenizer.base_prompts", (9, 64), (9, 64))]
    cfg = full_config(qf_layers=2, qf_dim=128, qf_inter=256, vit_dim=192, num_query_token=8, vit_depth=1, llm_layers=1,
                      llm_dim=256, vocab=64)
    qf = qformer_param_specs({n: torch.empty(s, device="meta") for n, (s, _) in shape_table(cfg, "myriad").items()})
    for base in (frozen, frozen + qf):
        a = ParamStore(base, "cpu")
        b = ParamStore(base + _vit_specs(), "cpu")
        wd_shift = b.n_wd - a.n_wd                                 # the ViT's decay run sits between the two groups
        for n, (o, k) in a.offsets.items():
            o2, k2 = b.offsets[n]
            assert k2 == k and o2 == (o if o < a.n_wd else o + wd_shift), n
        assert b.modules[:len(a.modules)] == a.modules
    st = ParamStore(frozen, "cpu")
    assert st.offsets == {"expert_adaptor.conv1.weight": (0, 768), "VETokenizer.base_prompts": (768, 576)}


def test_checkpoint_order_equals_the_reference_modules():
    """tests/golden/vit_param_order.json = named_parameters() of the reference's own VisionTransformer + a LayerNorm
    (tools/make_golden_vit_train.py)."""
    g = json.load(open(os.path.join(G, "vit_param_order.json")))
    specs = _vit_specs(depth=g["depth"])
    names = [n for n, _, _ in specs]
    assert sorted(names) == sorted(g["names"])
    assert C.reference_param_order(names[::-1]) == g["names"]
    # in the whole model: query_tokens (the model's own parameter), visual_encoder, ln_vision, then expert_adaptor ...
    order = C.reference_param_order(["llama_proj.bias", "expert_adaptor.conv1.weight", "query_tokens"] + names[::-1])
    assert order == ["query_tokens"] + g["names"] + ["expert_adaptor.conv1.weight", "llama_proj.bias"]


def test_patch_embedding_keeps_the_reference_layout_in_state_dicts():
    from myriad_amd.networks import from_reference_layout, to_reference_layout
    w = torch.randn(8, 3, 2, 2)
    assert torch.equal(from_reference_layout(w, (8, 3, 2, 2)), w) and torch.equal(to_reference_layout(w, (8, 3, 2, 2)), w)
    conv = from_reference_layout(w, (8, 12))                       # the conv stacks' GEMM order, unchanged
    assert torch.equal(conv, w.permute(0, 2, 3, 1).reshape(8, 12)) and torch.equal(to_reference_layout(conv, (8, 3, 2, 2)), w)


def test_mh_refresh_bf16_pair_argument_errors_before_any_launch():
    L = ops._L()
    nb = L.mh_refresh_bf16_pair_desc_bytes()
    assert nb == 64
    host = (ctypes.c_ubyte * (2 * nb + 16))()
    base = ctypes.addressof(host)
    base += (-base) % 16
    pack = L.mh_refresh_bf16_pair_pack
    # a valid entry: 100 x 70 -> 2 x 2 tiles; the next matrix starts behind them
    assert pack(base, 0, 0, 4096, 8192, 70, 16384, 100, 100, 70) == 4
    assert pack(base, 1, 4, 4096, 8192, 128, 0, 0, 64, 128) == 6   # no transposed copy
    assert pack(base, 0, 0, 4096, 0, 0, 16384, 100, 100, 70) == 4  # no row-major copy
    assert pack(base, 0, 0, 4096, 8192, 69, 16384, 100, 100, 70) < 0        # destination row shorter than the source row
    assert pack(base, 0, 0, 4096, 8192, 70, 16384, 99, 100, 70) < 0         # transposed row shorter than R
    assert pack(base, 0, 0, 4096, 0, 0, 0, 0, 100, 70) < 0                  # no destination at all
    assert pack(base, 0, 0, 0, 8192, 70, 16384, 100, 100, 70) < 0           # no source
    assert pack(base, 0, 0, 4098, 8192, 70, 16384, 100, 100, 70) < 0        # misaligned source
    assert pack(base, 0, 0, 4096, 8193, 70, 16384, 100, 100, 70) < 0        # misaligned destination
    assert pack(base, 0, 0, 4096, 8192, 70, 16384, 100, 0, 70) < 0          # empty matrix
    assert pack(base + 4, 0, 0, 4096, 8192, 70, 16384, 100, 100, 70) < 0    # misaligned table
    assert pack(0, 0, 0, 4096, 8192, 70, 16384, 100, 100, 70) < 0
    run = L.mh_refresh_bf16_pair
    assert run(0, 2, 6, 0) != 0                                    # no table
    assert run(4096 + 8, 2, 6, 0) != 0                             # misaligned table
    assert run(4096, 0, 6, 0) != 0 and run(4096, 2, 0, 0) != 0     # counts that cannot belong together
    assert run(4096, 3, 2, 0) != 0                                 # fewer tiles than matrices
    assert run(0, 0, 0, 0) == 0                                    # nothing to do


@pytest.mark.parametrize("world", [2, 4, 8])
def test_exchange_segments_and_shards_with_the_vit_in_the_buffer(world):
    """MyriadHIP._dp_segment on a store that holds the map tokenizer's head and the ViT: the cuts stay multiples of 4 * world,
    the ViT's runs lie in the last segment (exchanged after the backward), and the rs_ag shards of the ranks tile every segment
    -- the ViT's parameters and Adam moments included -- exactly once."""
    from types import SimpleNamespace
    from myriad_amd.networks import ve_param_specs
    from myriad_amd.runner import DataParallel
    specs = [("expert_adaptor.conv1.weight", (4, 64), (4, 64))] + ve_param_specs("VETokenizer.", 64, 5) + _vit_specs()
    st = ParamStore(specs, "cpu")
    owner = torch.zeros(st.total, dtype=torch.int32)
    for rank in range(world):
        dp = DataParallel(device=None, mode="rs_ag")
        dp.world, dp.rank = world, rank
        k = MyriadHIP._dp_segment(SimpleNamespace(store=st), dp)
        segs = dp.segments(st.total)
        assert k == 1 and len(segs) == 3
        assert all(lo % (4 * world) == 0 and hi % (4 * world) == 0 for lo, hi in segs)
        tok = st.module_range("VETokenizer", True)
        assert tok[0] <= segs[k][0] and segs[k][1] <= tok[1]
        for module, decays in (("visual_encoder", True), ("visual_encoder", False), ("ln_vision", False)):
            a, b = st.module_range(module, decays)
            assert segs[-1][0] <= a and b <= segs[-1][1], (module, decays)
        for (lo, hi), (a, b) in zip(segs, dp.shards(st.total)):
            assert lo <= a <= b <= hi and (a - lo) % 4 == 0 and (b - a) % 4 == 0
            assert (hi - lo) % (4 * world) == 0 and b - a == (hi - lo) // world      # equal pieces: the reduce-scatter in place
            owner[a:b] += 1
    assert bool((owner == 1).all())
