"""CPU checks of the q/v LoRA merge for the decode token step (LlamaHIP.decode_merge_lora): the reference rule of
tests/lora_merge_ref.py against float64, the switch's default and environment variable, the merged state dict's key names and
the library's new exports."""
import pytest
import torch

from myriad_amd import _lib
from myriad_amd.llama import decode_merge_lora_from_env
from myriad_amd.lora import merged_qv_names
from tests import golden_utils as gu
from tests import lora_merge_ref as LM

BF16 = torch.bfloat16


def _case(D, r, seed, b_std=0.05):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(3 * D, D, generator=g) * 0.02).to(BF16)
    a = (torch.rand(2 * r, D, generator=g) * 2 - 1) / D ** 0.5               # PEFT's kaiming-uniform bound
    bq, bv = torch.randn(D, r, generator=g) * b_std, torch.randn(D, r, generator=g) * b_std
    return w, a, bq, bv


@pytest.mark.parametrize("D,r", [(64, 8), (64, 16), (192, 8), (320, 16)])
def test_reference_rule_within_one_ulp_of_float64(D, r):
    w, a, bq, bv = _case(D, r, seed=D + r)
    s = 16.0 / r
    m = LM.merge_rows(w, a, bq, bv, s)
    exact = LM.merge_float64(w.float(), a, bq, bv, s)
    assert m.dtype == BF16 and m.shape == (3 * D, D)
    dist = LM.ulp_distance(m, exact)
    assert float(dist[:D].max()) <= 1.0 and float(dist[2 * D:].max()) <= 1.0, float(dist.max())
    assert torch.equal(m[D:2 * D], w[D:2 * D])                               # k rows: W bit for bit
    # the merge moved the q / v rows (the test would pass on a copy of W otherwise)
    assert float((m[:D].float() != w[:D].float()).float().mean()) > 0.5


def test_reference_rule_zero_b_is_w():
    w, a, bq, bv = _case(64, 8, seed=5)
    m = LM.merge_rows(w, a, torch.zeros_like(bq), torch.zeros_like(bv), 2.0)
    assert torch.equal(m.view(torch.int16), w.view(torch.int16))


def test_reference_rule_order_is_stated_fp32():
    """The sum is fp32 left to right, each product rounded on its own: a hand-built row where that order matters."""
    D, r = 64, 8
    w = torch.zeros(3 * D, D, dtype=BF16)
    a = torch.zeros(2 * r, D)
    bq, bv = torch.zeros(D, r), torch.zeros(D, r)
    a[0, 0], a[1, 0], a[2, 0] = 1.0, 1.0, 1.0
    bq[0, 0], bq[0, 1], bq[0, 2] = 2.0 ** 25, 1.0, -(2.0 ** 25)            # (2^25 + 1) rounds to 2^25 in fp32, then - 2^25 = 0
    m = LM.merge_rows(w, a, bq, bv, 1.0)
    assert float(m[0, 0]) == 0.0
    assert float(LM.merge_float64(w.float(), a, bq, bv, 1.0)[0, 0]) == 1.0   # the exact value differs: the order is the rule


def test_switch_defaults_off_and_reads_the_environment(monkeypatch):
    monkeypatch.delenv("MYRIAD_DECODE_MERGE_LORA", raising=False)
    assert decode_merge_lora_from_env() is False
    for v, want in (("0", False), ("1", True), ("yes", True)):
        monkeypatch.setenv("MYRIAD_DECODE_MERGE_LORA", v)
        assert decode_merge_lora_from_env() is want


def test_merged_state_dict_names_are_the_reference_llama_names():
    D, layers = 64, 3
    sd = gu.llama_weights(D, layers, 96, 128, seed=0)
    names = [n for i in range(layers) for n in merged_qv_names(i)]
    ref = [k for k in sd if k.endswith(("self_attn.q_proj.weight", "self_attn.v_proj.weight"))]
    assert sorted(names) == sorted(ref) and len(names) == 2 * layers
    assert merged_qv_names(1) == ("llama_model.model.layers.1.self_attn.q_proj.weight",
                                  "llama_model.model.layers.1.self_attn.v_proj.weight")


def test_merged_step_state_dict_drops_lora_and_merges_q_v():
    D, layers, r = 64, 2, 8
    sd = {k: (v.to(BF16).float() if v.dim() == 2 else v) for k, v in gu.llama_weights(D, layers, 96, 128, seed=1).items()}
    g = torch.Generator().manual_seed(2)
    for i in range(layers):
        p = f"llama_model.model.layers.{i}.self_attn."
        for n in ("q_proj", "v_proj"):
            sd[p + n + ".lora_A.default.weight"] = torch.randn(r, D, generator=g) * 0.05
            sd[p + n + ".lora_B.default.weight"] = torch.randn(D, r, generator=g) * 0.1
    out = LM.merged_step_state_dict(sd, layers, 2.0)
    assert not [k for k in out if ".lora_" in k]
    for i in range(layers):
        m = LM.merge_rows(LM.qkv_of(sd, i).to(BF16), *LM.lora_of(sd, i), 2.0).float()
        assert torch.equal(LM.qkv_of(out, i), m)


def test_header_declares_the_merge_entry_points():
    sigs = _lib.parse_header()
    for name in ("mh_lora_merge", "mh_lora_merge_pack", "mh_lora_merge_pack_fp8"):
        assert name in sigs and not name.startswith("mhdbg_")
