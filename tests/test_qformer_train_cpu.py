"""freeze_qformer: False on the host side (CPU): configuration, trainable parameter set and order, weight-decay groups,
checkpoint round trip with the Q-Former's optimiser state, and the data-parallel exchange over the Q-Former's range."""
import json
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from myriad_amd import checkpoint as C
from myriad_amd.myriad import MODULES, MyriadHIP, MiniGPT4HIP, ParamStore, module_of, uses_weight_decay
from myriad_amd.networks import to_reference_layout
from myriad_amd.qformer import qformer_param_specs
from myriad_amd.runner import DataParallel
from myriad_amd.synthetic import full_config, shape_table

G = os.path.join(os.path.dirname(__file__), "golden")


def _qf_shapes(layers=4, dim=128, inter=256, vit_dim=192, nq=8):
    cfg = full_config(qf_layers=layers, qf_dim=dim, qf_inter=inter, vit_dim=vit_dim, num_query_token=nq, vit_depth=1,
                      llm_layers=1, llm_dim=256, vocab=64)
    return {n: torch.empty(s, device="meta") for n, (s, _) in shape_table(cfg, "myriad").items()}


def test_trainable_set_and_order_equal_the_reference_modules():
    """tests/golden/qformer_train_param_order.json = query_tokens + named_parameters() of the reference's own BertLMHeadModel
    after myriad.py:151-156 (tools/make_golden_qformer_train.py)."""
    g = json.load(open(os.path.join(G, "qformer_train_param_order.json")))
    specs = qformer_param_specs(_qf_shapes(layers=g["layers"]))
    names = [n for n, _, _ in specs]
    assert sorted(names) == sorted(g["names"])
    assert C.reference_param_order(names[::-1]) == g["names"]
    assert all(module_of(n) == "Qformer" for n in names)


def test_weight_decay_groups_and_flat_layout():
    specs = qformer_param_specs(_qf_shapes())
    shapes = {n: r for n, _, r in specs}
    for n, r in shapes.items():
        decays = uses_weight_decay(n, len(r))
        if n == "query_tokens" or n.endswith(".weight") and "LayerNorm" not in n:
            assert decays, n
        else:
            assert not decays, n                           # biases and LayerNorm parameters: no weight decay
    st = ParamStore([("expert_adaptor.conv1.weight", (4, 192), (4, 192))] + specs, "cpu")
    assert st.modules == ["expert_adaptor", "Qformer"] and MODULES[-1] == "Qformer"
    # the products read [3D, D] query|key|value and the cross layers' key|value as ONE matrix: adjacent in the flat buffer
    p = "Qformer.bert.encoder.layer."
    for grp in ([p + f"1.attention.self.{w}.weight" for w in ("query", "key", "value")],
                [p + f"0.attention.self.{w}.bias" for w in ("query", "key", "value")],
                [p + f"{i}.crossattention.self.{w}.weight" for i in (0, 2) for w in ("key", "value")],
                [p + f"{i}.crossattention.self.{w}.bias" for i in (0, 2) for w in ("key", "value")]):
        offs = [st.offsets[n] for n in grp]
        assert all(offs[i][0] + offs[i][1] == offs[i + 1][0] for i in range(len(offs) - 1)), grp
    assert st.module_range("Qformer", True) is not None and st.module_range("Qformer", False) is not None


def test_frozen_recipe_layout_is_unchanged_by_the_new_module():
    specs = [("expert_adaptor.conv1.weight", (4, 192), (4, 192)), ("VETokenizer.base_prompts", (9, 64), (9, 64))]
    st = ParamStore(specs, "cpu")
    assert st.modules == ["expert_adaptor", "VETokenizer"]
    assert st.offsets == {"expert_adaptor.conv1.weight": (0, 768), "VETokenizer.base_prompts": (768, 576)}


class _Reached(Exception):
    pass


@pytest.mark.parametrize("cls", [MyriadHIP, MiniGPT4HIP])
def test_from_config_freeze_switches(cls, monkeypatch):
    base = dict(weights={}, device="cuda:0")
    for k in ("freeze_vit", "freeze_llama"):
        with pytest.raises(NotImplementedError, match=k):
            cls.from_config(dict(base, **{k: False}))
    from myriad_amd import ops

    def reached(*a, **k):
        raise _Reached()
    monkeypatch.setattr(ops, "ensure_workspace", reached)          # the first device step of the constructor
    seen = {}
    orig_init = cls.__init__

    def spy(self, weights, cfg=None, device="cuda:0"):
        seen.update(cfg)
        return orig_init(self, weights, cfg, device)
    monkeypatch.setattr(cls, "__init__", spy)
    # the reference's YAML form: freeze_qformer False alone (dropout 0.1 by default) gets past every check
    with pytest.raises(_Reached):
        cls.from_config(dict(base, freeze_qformer=False))
    assert seen["freeze_qformer"] is False and "qformer_dropout" not in seen
    with pytest.raises(_Reached):
        cls.from_config(dict(base, freeze_qformer=False, qformer_dropout=0.2, qformer_dropout_seed=9))
    assert seen["qformer_dropout"] == 0.2 and seen["qformer_dropout_seed"] == 9
    with pytest.raises(ValueError, match="qformer_dropout"):
        cls.from_config(dict(base, freeze_qformer=False, qformer_dropout=1.0))


class _ToyModel:
    """state_dict / load_state_dict / store of MyriadHIP (freeze_qformer: False) without the GPU parts."""

    def __init__(self):
        specs = [("expert_adaptor.conv1.weight", (4, 192), (4, 192))] + qformer_param_specs(_qf_shapes(layers=2))
        self.store = ParamStore(specs, "cpu")
        g = torch.Generator().manual_seed(3)
        for t in (self.store.flat_p, self.store.flat_m, self.store.flat_v):
            t.copy_(torch.randn(t.shape, generator=g))
        self.store.flat_v.abs_()
        self.store.step = 5
        self.store.set_module_steps({"expert_adaptor": 5, "Qformer": 4})

    def state_dict(self):
        return {n: to_reference_layout(self.store.p[n], r).clone() for n, _, r in self.store.specs}

    def load_state_dict(self, sd, strict=False):
        for n, i, _ in self.store.specs:
            if n in sd:
                self.store.p[n].copy_(sd[n].float().reshape(i))


def test_checkpoint_round_trip_with_qformer_optimizer_state(tmp_path):
    m = _ToyModel()
    path = C.CheckpointManager(str(tmp_path)).save(m, 0, lr=1e-4)
    ck = torch.load(path, map_location="cpu")
    assert "query_tokens" in ck["model"] and "Qformer.bert.encoder.layer.1.output_query.LayerNorm.bias" in ck["model"]
    order = C.reference_param_order(list(ck["model"]))
    assert order[0] == "query_tokens" and order[1] == "expert_adaptor.conv1.weight"
    shapes = {n: r for n, _, r in m.store.specs}
    wd = [n for n in order if uses_weight_decay(n, len(shapes[n]))]
    nwd = [n for n in order if n not in wd]
    prm = {n: torch.nn.Parameter(ck["model"][n].clone()) for n in order}
    opt = torch.optim.AdamW([{"params": [prm[n] for n in wd], "weight_decay": 0.05},
                             {"params": [prm[n] for n in nwd], "weight_decay": 0.0}], lr=1e-4)
    opt.load_state_dict(ck["optimizer"])                   # a reference-layout AdamW state
    for n in order:
        st = opt.state[prm[n]]
        o, k = m.store.offsets[n]
        assert float(st["step"]) == (4.0 if module_of(n) == "Qformer" else 5.0)
        assert torch.equal(st["exp_avg"], m.store.flat_m[o:o + k].view(shapes[n]))
        assert torch.equal(st["exp_avg_sq"], m.store.flat_v[o:o + k].view(shapes[n]))
    m2 = _ToyModel()
    for t in (m2.store.flat_p, m2.store.flat_m, m2.store.flat_v):
        t.zero_()
    m2.store.set_module_steps({})
    C.CheckpointManager.load(m2, path)
    for a, b in ((m.store.flat_p, m2.store.flat_p), (m.store.flat_m, m2.store.flat_m), (m.store.flat_v, m2.store.flat_v)):
        assert torch.equal(a[:m.store.n_used], b[:m.store.n_used])
    assert m2.store.module_steps() == {"expert_adaptor": 5, "Qformer": 4}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, mode, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    specs = [("expert_adaptor.conv1.weight", (4, 192), (4, 192))] + qformer_param_specs(_qf_shapes(layers=2))
    st = ParamStore(specs, "cpu")
    torch.manual_seed(11 + rank)
    st.flat_g.copy_(torch.randn(st.total))
    st.used.fill_(1.0)
    mine = st.flat_g_comm.clone()
    dp = DataParallel(device=None, mode=mode)
    dp.allreduce(st.flat_g_comm, st.total)
    q.put((rank, st.module_range("Qformer", True), st.module_range("Qformer", False), mine.numpy().copy(),
           st.flat_g_comm.numpy().copy()))
    dp.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["allreduce", "rs_ag"])
def test_exchange_covers_the_qformer_range_world2_gloo(mode):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, mode, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(2):
        r, rw, rn, mine, red = q.get(timeout=120)
        got[r] = (rw, rn, torch.from_numpy(mine), torch.from_numpy(red))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (a, b), (c, d) = got[0][0], got[0][1]
    want = got[0][2] + got[1][2]                          # one-process sum (AdamW applies 1/world)
    for r in range(2):
        red = got[r][3]
        assert torch.allclose(red[a:b], want[a:b], atol=1e-6) and torch.allclose(red[c:d], want[c:d], atol=1e-6)
    assert torch.equal(got[0][3][a:b], got[1][3][a:b]) and torch.equal(got[0][3][c:d], got[1][3][c:d])
