"""Two data-parallel ranks of a freeze_vit: False model on ONE GPU (the pattern of tests/test_dp_gpu.py): both exchange modes,
overlap on.  The ranks must end with identical parameters and optimiser state -- the ViT and ln_vision masters included -- equal,
bit for bit, to ONE process that sums the two ranks' gradients and applies AdamW with 1/world (the mean gradient)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference(dev):
    from tests import dp_common as C
    from tests import vit_dp_worker as W
    model, cfg = W.build_model(dev)
    st = model.store
    losses = {0: [], 1: []}
    for i in range(W.N_STEPS):
        gs = []
        for r in (0, 1):
            model.fixed_stage = W.STAGES[r][i]
            with torch.no_grad():
                losses[r].append(float(model._forward_impl(C.batch(r, i, cfg["vocab"], dev), True)))
                model.backward()
            torch.cuda.synchronize()
            gs.append(st.flat_g_comm.clone())
        st.flat_g_comm.copy_(gs[0] + gs[1])
        st.adamw_step(W.LRS[i], 0.05, grad_scale=0.5)
    return C.snapshot(model), losses, model


@pytest.mark.parametrize("mode", ["allreduce", "rs_ag"])
def test_two_ranks_train_the_vit_like_one_process_fed_the_mean_gradient(mode, tmp_path):
    from tests import vit_dp_worker as W
    port = str(29850 + (os.getpid() % 100) + (0 if mode == "allreduce" else 101))
    outs = [str(tmp_path / f"rank{r}.pt") for r in (0, 1)]
    env = dict(os.environ, PYTHONPATH=ROOT)
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "vit_dp_worker.py"), str(r), "2", port, mode, outs[r]],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in (0, 1)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace")[-3000:])
    assert all(p.returncode == 0 for p in procs), "\n----\n".join(logs)
    s0, s1 = (torch.load(o) for o in outs)
    ref, ref_losses, model = _reference(torch.device("cuda:0"))
    st = model.store
    for k in ("p", "m", "v"):
        assert torch.equal(s0[k], s1[k]), k                        # the ranks agree ...
        assert torch.equal(s0[k], ref[k]), (k, (s0[k] - ref[k]).abs().max().item())     # ... with the one-process result
    assert s0["steps"] == s1["steps"] == ref["steps"]
    assert s0["losses"] == ref_losses[0] and s1["losses"] == ref_losses[1]
    assert s0["steps"]["visual_encoder"] == W.N_STEPS and s0["steps"]["ln_vision"] == W.N_STEPS
    assert s0["steps"]["VEInstructor"] == W.N_STEPS - 1           # unused by every rank at step 1
    # the ViT and ln_vision masters moved, and their moments are populated over the whole range
    fresh, _ = W.build_model(torch.device("cuda:0"))
    for module in ("visual_encoder", "ln_vision"):
        for decays in (True, False):
            rng = st.module_range(module, decays)
            if rng is None:
                continue
            a, b = rng
            assert (fresh.store.flat_p[a:b].cpu() - s0["p"][a:b]).abs().max().item() > 1e-6, (module, decays)
            assert float(s0["v"][a:b].max()) > 0
    # exchange geometry: the cuts are multiples of 4 * world, the ViT lies behind the tokenizer's early segment, and in rs_ag
    # each rank owned (and updated the moments of) half of every segment, the ViT's included
    segs = s0["segments"]
    assert segs == s1["segments"] and len(segs) == 3 and all(lo % 8 == 0 and hi % 8 == 0 for lo, hi in segs)
    tok = st.module_range("VETokenizer", True)
    k = [i for i, (lo, hi) in enumerate(segs) if tok[0] <= lo and hi <= tok[1]]
    assert len(k) == 1
    a, b = st.module_range("visual_encoder", True)
    assert segs[-1][0] <= a and b <= segs[-1][1] and k[0] != len(segs) - 1
    if mode == "rs_ag":
        assert not s0["complete_before_gather"] and not s1["complete_before_gather"]
        for (lo, hi), (a0, b0), (a1, b1) in zip(segs, s0["shards"], s1["shards"]):
            assert a0 == lo and b0 == a1 and b1 == hi and (b0 - a0) % 4 == 0
        (a0, b0), (a1, b1) = s0["shards"][-1], s1["shards"][-1]
        assert a < b0 and a1 < b                                   # both ranks hold a part of the ViT's moments
    else:
        assert s0["complete_before_gather"]
