"""Gradient clipping and the non-finite guard under data parallelism: two ranks on ONE GPU over gloo (tests/grad_clip_dp_worker.py,
the set-up of tests/test_dp_gpu.py) with a max_grad_norm small enough that every step clips.  In 'allreduce' every rank norms the
whole reduced gradient; in 'rs_ag' each rank norms the slices it owns, the per-rank fp64 sums travel in a world-long vector and
every rank finalises from the same slots in rank order -- so both ranks derive the same control block bit for bit.  That vector
goes through torch.distributed or, on the context path (the stand-in RCCL of tests/fake_rccl), through an all-gather verb."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_NORM = 1e-2


def _reference(dev):
    """One process: per step both ranks' forward + backward, the two [gradients | use flags] buffers added, one update with
    grad_scale = 1/2 under the same clip (the pattern of test_dp_gpu._reference)."""
    from myriad_amd.myriad import GradClip
    from tests import dp_common as C
    model, cfg = C.build_model(dev)
    st = model.store
    for i in range(C.N_STEPS):
        gs = []
        for r in (0, 1):
            model.lora.base_seed = C.BASE_SEED + r
            model.lora.step_seed = i
            model.fixed_stage = C.STAGES[r][i]
            with torch.no_grad():
                model._forward_impl(C.batch(r, i, cfg["vocab"], dev), True)
                model.backward()
            torch.cuda.synchronize()
            gs.append(st.flat_g_comm.clone())
        st.flat_g_comm.copy_(gs[0] + gs[1])
        st.adamw_step(C.LRS[i], 0.05, grad_scale=0.5, clip=GradClip(MAX_NORM, True))
    snap = C.snapshot(model)
    snap["ctl"] = st.ctl.cpu().clone()
    return snap


@pytest.fixture(scope="module")
def reference():
    return _reference(torch.device("cuda:0"))


@pytest.fixture(scope="module")
def fake_rccl(tmp_path_factory):
    """The stand-in RCCL of tests/fake_rccl, built with hipcc (host code only), as tests/test_dp_gpu.py does."""
    out = str(tmp_path_factory.mktemp("fake_rccl") / "libfake_rccl.so")
    src = os.path.join(ROOT, "tests", "fake_rccl", "fake_rccl.cpp")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-shared", "-fPIC", "-o", out, src])
    return out


def _bits(t):
    return t.view(torch.int64)


CASES = [("allreduce", "torch"), ("rs_ag", "torch"), ("rs_ag", "ctx")]


@pytest.mark.parametrize("mode,collective", CASES, ids=["-".join(c) for c in CASES])
def test_two_ranks_clip_alike_and_skip_together(mode, collective, tmp_path, reference, fake_rccl):
    """Both ranks end with identical p, m, v, step counts and control-block bits, equal to the single-process update of the summed
    gradient.  ('rs_ag' adds the squares in another order than one process does -- per rank, then over ranks -- so there ctl[1],
    the norm, is compared to 1e-14 relative instead of bit for bit; s is that norm's function rounded to fp32, 2^-24 apart, and
    the parameters are compared bit for bit.)  Then a NaN in rank 1's gradient: both ranks skip, in both modes."""
    from tests import dp_common as C
    port = str(29900 + (os.getpid() % 200) + 7 * CASES.index((mode, collective)))
    outs = [str(tmp_path / f"rank{r}.pt") for r in (0, 1)]
    env = dict(os.environ, PYTHONPATH=ROOT)
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "grad_clip_dp_worker.py"), str(r), "2", port, mode, outs[r],
                               repr(MAX_NORM), collective, fake_rccl], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in (0, 1)]
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
    r0, r1 = (torch.load(o) for o in outs)
    for when in ("clean", "after"):
        a, b = r0[when], r1[when]
        for k in ("p", "m", "v"):
            assert torch.equal(a[k], b[k]), (when, k)
        assert a["steps"] == b["steps"]
        assert torch.equal(_bits(a["ctl"]), _bits(b["ctl"])), (when, a["ctl"], b["ctl"])
    assert r0["calls"] == r1["calls"] == {"adamw_pieces": 0, "adamw_module": 0}       # nothing was updated ahead of the norm
    # every step clipped, none was skipped, and the result is the single-process one
    a = r0["clean"]
    assert a["stats"]["applied"] and a["stats"]["skipped_steps"] == 0 and a["stats"]["clip_scale"] < 0.5
    for k in ("p", "m", "v"):
        assert torch.equal(a[k], reference[k]), (k, (a[k] - reference[k]).abs().max().item())
    assert a["steps"] == reference["steps"] and a["steps"]["VEInstructor"] == C.N_STEPS - 1
    got, want = a["ctl"].tolist(), reference["ctl"].tolist()
    assert got[0] == want[0] and got[2:] == want[2:]
    assert got[1] == want[1] if mode == "allreduce" else abs(got[1] - want[1]) <= 1e-14 * want[1]
    # the NaN step: nothing moved on either rank, the count went up by one
    b = r0["after"]
    for k in ("p", "m", "v"):
        assert torch.equal(a[k], b[k]), k
    assert a["steps"] == b["steps"]
    assert not b["stats"]["applied"] and b["stats"]["skipped_steps"] == 1 and r1["after"]["stats"]["skipped_steps"] == 1
