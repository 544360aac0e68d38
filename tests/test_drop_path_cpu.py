"""Stochastic depth (drop_path_rate) on the host side: the configuration gate, and the keep-bit generator against its plain
integer restatement (tests/drop_path_ref.py)."""
import math

import pytest
import torch

from myriad_amd import ops
from myriad_amd.eva_vit import drop_path_keep_bits, drop_path_keep_prob
from myriad_amd.myriad import MiniGPT4HIP, MyriadHIP
from tests import drop_path_ref as ref

SEED = 20240607            # the frequency test's seed: checked to pass under the restated rule


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


TRAIN = dict(freeze_vit=False, vit_precision="fp32")


@pytest.mark.parametrize("cls", [MyriadHIP, MiniGPT4HIP])
def test_config_gate(cls, monkeypatch):
    monkeypatch.delenv("MYRIAD_VIT_DROP_PATH", raising=False)
    base = dict(weights={}, device="cuda:0")
    seen = _spy(cls, monkeypatch)
    # switch off: the two refusals, word for word
    with pytest.raises(NotImplementedError) as e:
        cls.from_config(dict(base, drop_path_rate=0.1, **TRAIN))
    assert str(e.value) == "drop_path_rate > 0 (stochastic depth in the ViT's training forward) is not implemented"
    with pytest.raises(NotImplementedError) as e:
        cls.from_config(dict(base, drop_path_rate=0.1))
    assert str(e.value) == "drop_path_rate only matters for an unfrozen ViT"
    # switch on, frozen ViT: still refused
    for switch in (dict(vit_drop_path=True), "env"):
        if switch == "env":
            monkeypatch.setenv("MYRIAD_VIT_DROP_PATH", "1")
            switch = {}
        with pytest.raises(NotImplementedError, match="only matters for an unfrozen ViT"):
            cls.from_config(dict(base, drop_path_rate=0.1, **switch))
        for bad in (1.0, 1.5, -0.1):
            with pytest.raises(ValueError, match="drop_path_rate"):
                cls.from_config(dict(base, drop_path_rate=bad, **switch, **TRAIN))
        with pytest.raises(_Reached):
            cls.from_config(dict(base, drop_path_rate=0.4, drop_path_seed=11, **switch, **TRAIN))
        assert seen["drop_path_rate"] == 0.4 and seen["drop_path_seed"] == 11 and seen["freeze_vit"] is False
        with pytest.raises(_Reached):                              # rate 0 needs no switch and hands nothing on
            cls.from_config(dict(base, drop_path_rate=0, **TRAIN))
        assert "drop_path_rate" not in seen
    monkeypatch.setenv("MYRIAD_VIT_DROP_PATH", "0")                # only "1" is the switch
    with pytest.raises(NotImplementedError, match="is not implemented"):
        cls.from_config(dict(base, drop_path_rate=0.1, **TRAIN))


def test_keep_prob_is_the_linspace():
    for rate, depth in ((0.4, 39), (0.1, 3), (0.5, 2), (0.0, 5)):
        want = (1.0 - torch.linspace(0, rate, depth, dtype=torch.float64)).tolist()
        got = drop_path_keep_prob(rate, depth)
        assert len(got) == depth and got[0] == 1.0 and max(abs(a - b) for a, b in zip(got, want)) < 1e-12
    assert drop_path_keep_prob(0.3, 1) == [1.0]


def test_generator_equals_the_restatement():
    for seed, rank, step, micro, depth, B, rate in ((5, 0, 0, 0, 39, 8, 0.4), ((1 << 40) + 77, 3, (1 << 33) + 5, 2, 3, 4, 0.5),
                                                     (SEED, 1, 999, 0, 12, 1, 0.1), (0, 0, 0, 0, 1, 4, 0.9)):
        got = drop_path_keep_bits(seed, rank, step, micro, depth, B, rate)
        assert got.dtype == torch.bool and tuple(got.shape) == (depth, 2, B) and not got.is_cuda
        assert torch.equal(got, ref.keep_bits(seed, rank, step, micro, depth, B, rate))
        assert bool(got[0].all())                                  # block 0 never drops
    assert bool(drop_path_keep_bits(3, 0, 0, 0, 39, 8, 0.0).all())
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            drop_path_keep_bits(3, 0, 0, 0, 39, 8, bad)


def test_generator_changes_with_each_input():
    base = dict(seed=SEED, rank=0, step=7, micro=0, depth=39, batch=8, rate=0.4)
    b0 = drop_path_keep_bits(**base)
    assert torch.equal(b0, drop_path_keep_bits(**base))            # a pure function: a resumed run draws the same bits
    for key, val in (("seed", SEED + 1), ("seed", SEED + (1 << 32)), ("rank", 1), ("step", 8), ("step", 7 + (1 << 32)), ("micro", 1)):
        assert not torch.equal(b0, drop_path_keep_bits(**dict(base, **{key: val}))), key
    # block, branch and sample: at drop probabilities 0.3 and 0.6 (depth 3, rate 0.6) no two of the 2 x 2 x 8 positions share
    # their bit sequence over 64 steps (a chance collision has probability < 32^2 / 2 * 0.58^64 < 1e-12)
    seq = torch.stack([drop_path_keep_bits(**dict(base, depth=3, rate=0.6, step=s)) for s in range(64)], -1)   # [3, 2, B, 64]
    flat = seq[1:].reshape(-1, 64)                                 # (block 0 is all ones)
    assert len({tuple(r.tolist()) for r in flat}) == flat.shape[0]


def test_drop_frequency_follows_the_linspace():
    depth, B, rate, steps = 39, 8, 0.4, 256                        # 256 steps x 8 samples x 2 branches = 4096 draws a block
    drops = torch.zeros(depth, dtype=torch.int64)
    for s in range(steps):
        drops += (~drop_path_keep_bits(SEED, 0, s, 0, depth, B, rate)).sum((1, 2))
    n = steps * B * 2
    assert int(drops[0]) == 0
    for i in range(1, depth):
        p = rate * i / (depth - 1)
        assert abs(int(drops[i]) / n - p) <= 4 * math.sqrt(p * (1 - p) / n), (i, int(drops[i]) / n, p)
    # the restated rule gives the same counts where it is affordable to run
    few = sum((~ref.keep_bits(SEED, 0, s, 0, depth, B, rate)).sum((1, 2)) for s in range(4))
    assert torch.equal(few, sum((~drop_path_keep_bits(SEED, 0, s, 0, depth, B, rate)).sum((1, 2)) for s in range(4)))


def test_reference_forward_is_the_oracle_when_nothing_drops_and_identity_where_all_drops():
    from oracle import myriad_ref as R
    from myriad_amd.eva_vit import vit_param_shapes
    g = torch.Generator().manual_seed(3)
    sd = {n: torch.randn(s, generator=g, dtype=torch.float64) * 0.1 for n, s in vit_param_shapes(32, 3, 4, 5, [48, 48]).items()}
    image = torch.randn(3, 3, 8, 8, generator=g, dtype=torch.float64)
    want = R.vit_forward(sd, image, num_heads=4)
    ones = torch.ones(2, 2, 3, dtype=torch.bool)
    assert torch.allclose(ref.vit_forward_drop(sd, image, ones, [1.0, 1.0], num_heads=4), want, rtol=0, atol=1e-12)
    keep = ones.clone()
    keep[1, :, 2] = False                                           # sample 2 skips block 1: it leaves with block 0's output
    sd1 = {k: v for k, v in sd.items() if ".blocks.1." not in k}
    got = ref.vit_forward_drop(sd, image, keep, [1.0, 0.5], num_heads=4)
    assert torch.allclose(got[2], R.vit_forward(sd1, image, num_heads=4)[2], rtol=0, atol=1e-12)
    assert not torch.allclose(got[0], want[0])                     # a kept sample's branches are scaled by 1 / 0.5


def test_drop_path_map_checks():
    m = ops.DropPathMap.from_keep([True, False, True, True])
    assert m.slot.tolist() == [0, -1, 1, 2] and m.K == 3 and m.B == 4 and m.samples == [0, 2, 3] and not m.full
    assert ops.DropPathMap.from_keep(torch.tensor([False, False])).K == 0
    assert ops.DropPathMap([1, 0]).samples == [1, 0]
    for bad in ([0, 0, 1], [0, 2, -1], [-2, 0], [0, 3, 1, 2][:3], [], [0.0, 1.0], list(range(65))):
        with pytest.raises(ValueError):
            ops.DropPathMap(bad)
