"""GPU checks of the device sampler (mh_sample_rows, mh_repetition_penalty_rows) against tests/sampling_ref.py, its output
distribution, and the decode loop with `device_sampling` and `repetition_penalty` on."""
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import ops  # noqa: E402
from myriad_amd.llama import LlamaHIP  # noqa: E402
from oracle import myriad_ref as R  # noqa: E402
from tests import golden_utils as gu  # noqa: E402
from tests import sampling_ref as S  # noqa: E402

DEV = "cuda:0"
G = os.path.join(os.path.dirname(__file__), "golden")
SEED = 0x1234_5678_9ABC_DEF1


def load(name):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(G, name + ".npz")).items()}


def _buffers(R_, dev=DEV):
    return dict(out=torch.empty(R_, dtype=torch.long, device=dev), mar=torch.empty(R_, dtype=torch.float32, device=dev),
                pmx=torch.empty(R_, dtype=torch.float32, device=dev), kept=torch.empty(R_, dtype=torch.int32, device=dev),
                u=torch.empty(R_, dtype=torch.float32, device=dev))


def _params(inv_temp, top_p, top_k, penalty=1.0):
    return torch.tensor([inv_temp, top_p, float(top_k), penalty], dtype=torch.float32, device=DEV)


def _logits(R_, V, g, ldl=None):
    """[R, V] f32 view with row stride ldl (a multiple of 4: the kernel's row alignment)."""
    ldl = ldl or ((V + 3) // 4 * 4)
    full = torch.full((R_, ldl), float("nan"))
    full[:, :V] = torch.randn(R_, V, generator=g) * 3.0
    return full.to(DEV)[:, :V]


def test_sample_rows_equals_the_reference_over_the_grid():
    g = torch.Generator().manual_seed(3)
    extra = list(itertools.product((0.7, 1.0, 1.3), (1.0, 1.3), (False, True)))        # (T, penalty, ban) cycled over the grid
    rows = near = 0
    for n, (R_, V, top_k, top_p) in enumerate(itertools.product((1, 4, 16), (32000, 1000, 999), (1, 50, 1024), (0.01, 0.5, 0.9, 1.0))):
        T, pen, use_ban = extra[n % len(extra)]
        ban = 5 if use_ban else -1
        x = _logits(R_, V, g)
        seen_ids = [torch.randint(0, V, (6,), generator=g).tolist() for _ in range(R_)]
        bits = np.zeros((R_, (V + 31) // 32), dtype=np.uint32)
        for r, ids in enumerate(seen_ids):
            for i in ids:
                bits[r, i // 32] |= np.uint32(1 << (i % 32))
        seen = torch.from_numpy(bits.view(np.int32)).to(DEV)
        prm = _params(1.0 / T, top_p, top_k, pen)
        x_cpu = x.cpu()
        if pen != 1.0:
            ops.repetition_penalty_rows(x, seen, None, prm[3:])
        b = _buffers(R_)
        seed = torch.tensor([SEED + n], dtype=torch.long, device=DEV)
        step = torch.tensor([n % 7], dtype=torch.int32, device=DEV)
        ops.sample_rows(x, b["out"], b["mar"], b["pmx"], b["kept"], prm, seed, ban_id=ban, step=step, t_add=1, u_out=b["u"])
        am = _buffers(R_)
        ops.argmax_pmax_rows(x, am["out"], am["mar"], am["pmx"], ban_id=ban, inv_temp=1.0 / T)
        torch.cuda.synchronize()
        assert torch.equal(b["mar"], am["mar"]) and torch.allclose(b["pmx"], am["pmx"], rtol=1e-6, atol=0)
        for r in range(R_):
            u = S.uniform(SEED + n, n % 7 + 1, r)
            assert float(b["u"][r]) == u                                           # the host Philox, bit for bit
            row = x[r].cpu()
            assert torch.allclose(row, S.penalize(x_cpu[r], seen_ids[r], pen), rtol=1e-6, atol=0)
            ref = S.sample_row(row, top_k, top_p, 1.0 / T, ban, u=u)
            if ref["near"]:
                near += 1
                continue
            assert int(b["kept"][r]) == ref["kept"], (n, r)
            assert int(b["out"][r]) == ref["out"], (n, r, top_k, top_p, T)
            rows += 1
    assert near <= 0.02 * (rows + near), (near, rows)


def test_tied_top_k_overflow_reports_minus_one():
    V = 4000
    x = torch.randn(3, V, generator=torch.Generator().manual_seed(1))
    x[0, :1500] = 9.0                         # 1500 tied maxima > the 1024-candidate cap
    x[1, 100:1124] = 9.0                      # exactly 1024 tied: still on the device
    x = x.to(DEV)
    b = _buffers(3)
    ops.sample_rows(x, b["out"], b["mar"], b["pmx"], b["kept"], _params(1.0, 0.9, 50), torch.tensor([7], device=DEV), u_out=b["u"])
    torch.cuda.synchronize()
    assert int(b["kept"][0]) == -1 and int(b["out"][0]) == 0
    assert 1 <= int(b["kept"][1]) <= 1024 and 100 <= int(b["out"][1]) < 1124
    assert 1 <= int(b["kept"][2]) <= 50


def test_sample_rows_distribution_matches_the_kept_set():
    V, R_ = 1000, 16384
    row = torch.randn(V, generator=torch.Generator().manual_seed(9)) * 2.0
    x = row.to(DEV).expand(R_, V).contiguous()
    b = _buffers(R_)
    ops.sample_rows(x, b["out"], b["mar"], b["pmx"], b["kept"], _params(1.0, 0.9, 50), torch.tensor([SEED], device=DEV))
    torch.cuda.synchronize()
    ref = S.sample_row(row, 50, 0.9, 1.0)
    kept_ids = ref["order"][:ref["kept"]]
    assert (b["kept"].cpu() == ref["kept"]).all()
    out = b["out"].cpu().numpy()
    assert np.isin(out, kept_ids).all()                                             # nothing outside the kept set, ever
    counts = np.array([(out == i).sum() for i in kept_ids], dtype=np.float64)
    expect = ref["probs"] * R_
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    dof = len(kept_ids) - 1
    assert chi2 < dof + 6 * np.sqrt(2 * dof) + 10, (chi2, dof)                      # generous: ~6 sigma


def test_repetition_penalty_kernel_marks_prev_ids_and_applies_the_hf_rule():
    V, R_ = 1000, 3
    x0 = torch.randn(R_, V, generator=torch.Generator().manual_seed(4)) * 2.0
    x = x0.to(DEV)
    seen = torch.zeros((R_, (V + 31) // 32), dtype=torch.int32, device=DEV)
    pen = torch.tensor([1.3], device=DEV)
    history = [[17, 999], [17, 17], [0, 640]]
    for t in range(2):
        prev = torch.tensor([h[t] for h in history], dtype=torch.long, device=DEV)
        x = x0.to(DEV)
        ops.repetition_penalty_rows(x, seen, prev, pen)
    torch.cuda.synchronize()
    for r in range(R_):
        assert torch.allclose(x[r].cpu(), S.penalize(x0[r], history[r], 1.3), rtol=1e-6, atol=0)
        bits = seen[r].cpu().numpy().view(np.uint32)
        marked = {w * 32 + b for w in range(len(bits)) for b in range(32) if bits[w] >> b & 1}
        assert marked == set(history[r])


# ------------------------------------------------------------------------------------------------ decode loop
def _tiny(std=0.02, rounded=False):
    gd = load("llama_tiny")
    D, layers, heads, inter, V, seed = [int(x) for x in gd["meta"]]
    sd = gu.llama_weights(D, layers, inter, V, seed=seed, std=std)
    if rounded:
        sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() and v.numel() > 4096 else v) for k, v in sd.items()}
    return gd, sd, heads


def test_device_sampling_in_the_decode_loop_is_seeded_and_stays_on_the_device():
    gd, sd, heads = _tiny()
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    lm.device_sampling = True
    emb = gd["emb"][:2, :7].to(DEV)
    kw = dict(max_new_tokens=10, stop_ids=(), do_sample=True, top_p=0.9)
    a = lm.greedy_generate(emb, generator=torch.Generator().manual_seed(5), **kw)
    st = dict(lm.last_generate_stats)
    assert st["device_sampled_rows"] > 0 and st["host_sampled_rows"] == 0
    assert st["graph_replays"] >= a.shape[1] - 3 and st["graph_replays"] > 0
    b = lm.greedy_generate(emb, generator=torch.Generator().manual_seed(5), **kw)
    assert torch.equal(a, b)
    assert lm.last_generate_stats["graph_replays"] == b.shape[1] - 1                 # the graph is kept across calls
    c = lm.greedy_generate(emb, generator=torch.Generator().manual_seed(6), **kw)
    assert not torch.equal(a, c)
    greedy = lm.greedy_generate(emb, max_new_tokens=10, stop_ids=())
    k1 = lm.greedy_generate(emb, generator=torch.Generator().manual_seed(7), top_k=1, **kw)
    assert torch.equal(k1, greedy) and lm.last_generate_stats["host_sampled_rows"] == 0
    t2 = lm.greedy_generate(emb, generator=torch.Generator().manual_seed(5), temperature=2.0, **kw)   # no re-capture needed
    assert t2.shape == a.shape and lm.last_generate_stats["graph_replays"] == t2.shape[1] - 1
    with pytest.raises(ValueError):
        lm.greedy_generate(emb, temperature=0.0, **kw)


def test_device_sampling_keeps_every_golden_id_on_peaked_logits():
    g = load("decode_chain")
    c = gu.DECODE_CHAIN
    lm = LlamaHIP(gu.decode_chain_weights(), c["heads"], DEV, need_backward=False)
    lm.device_sampling = True
    for name, rows in (("b4", ["row0", "row1", "row2", "row3"]), ("b1", ["row0"]), ("stop835", ["stop835"])):
        ids = lm.greedy_generate(gu.decode_chain_inputs(rows).to(DEV), max_new_tokens=90, min_length=1, do_sample=True, top_p=0.01,
                                 temperature=1.0, generator=torch.Generator().manual_seed(1))
        assert torch.equal(ids, g[name + "_ids"]), (name, ids, g[name + "_ids"])
        assert lm.last_generate_stats["host_sampled_rows"] == 0


def _oracle_penalized_greedy(sd, emb, heads, steps, penalty):
    """HF greedy with RepetitionPenaltyLogitsProcessor over the generated ids, the whole sequence re-run each step."""
    ew = sd["llama_model.model.embed_tokens.weight"]
    lm = sd["llama_model.lm_head.weight"]
    B = emb.shape[0]
    ids, margins = [], []
    for t in range(steps):
        x = emb if not ids else torch.cat([emb, ew[torch.stack(ids, 1)]], 1)
        h, _ = R.llama_model(sd, x, None, heads)
        logits = torch.nn.functional.linear(h[:, -1], lm)
        if ids:
            logits = torch.stack([S.penalize(logits[r], [int(i[r]) for i in ids], penalty) for r in range(B)])
        top2 = logits.topk(2, dim=-1).values
        margins.append(top2[:, 0] - top2[:, 1])
        ids.append(logits.argmax(-1))
    return torch.stack(ids, 1), torch.stack(margins, 1)


@pytest.mark.parametrize("device_sampling", [False, True])
def test_repetition_penalty_greedy_equals_the_oracle(device_sampling):
    gd, sd, heads = _tiny(std=0.2, rounded=True)
    lm = LlamaHIP(sd, heads, DEV, need_backward=False)
    lm.device_sampling = device_sampling
    emb = gd["emb"][:2, :7]
    steps = 12
    with torch.no_grad():
        ref, margins = _oracle_penalized_greedy(sd, emb, heads, steps, 1.3)
    ids = lm.greedy_generate(emb.to(DEV), max_new_tokens=steps, stop_ids=(), eos_id=-7, repetition_penalty=1.3)
    plain = lm.greedy_generate(emb.to(DEV), max_new_tokens=steps, stop_ids=(), eos_id=-7)
    assert not torch.equal(ids, plain)                                              # the penalty changed the decode
    # equal up to (and including) the first step where the oracle's top-2 margin is within the bf16 fixture's error (0.05, as the
    # greedy test of this fixture in test_model_gpu.py): after a legitimate tie-flip the sequences diverge by construction
    compared = 0
    for t in range(steps):
        assert torch.equal(ids[:, t], ref[:, t]), (t, ids, ref)
        compared += 1
        if float(margins[:, t].min()) < 0.05:
            break
    assert compared >= 2
    # the same penalty on the sampled path with top_k = 1 is the penalised greedy decode
    k1 = lm.greedy_generate(emb.to(DEV), max_new_tokens=steps, stop_ids=(), eos_id=-7, repetition_penalty=1.3, do_sample=True,
                            top_k=1, generator=torch.Generator().manual_seed(3))
    assert torch.equal(k1, ids)
    with pytest.raises(ValueError):
        lm.greedy_generate(emb.to(DEV), max_new_tokens=2, repetition_penalty=0.0)
