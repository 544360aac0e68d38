"""One data-parallel rank of tests/test_grad_clip_dp_gpu.py: `python tests/grad_clip_dp_worker.py RANK WORLD PORT MODE OUT MAX_NORM [COLLECTIVE RCCL_LIB]`.
As tests/dp_worker.py -- every rank on cuda:0, the process group gloo, the exchange overlapped, through torch.distributed
(COLLECTIVE = torch) or the mh_ctx verbs bound to the stand-in RCCL of tests/fake_rccl (ctx) -- with
train_step(max_grad_norm=MAX_NORM, skip_nonfinite=True): the three steps of tests/dp_common.py, a snapshot, then ONE more step in
which rank 1's gradient holds a NaN (planted behind its backward, in the LoRA range, which the exchange has not started yet), and
a second snapshot."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world, port, mode, out, max_norm = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5], float(sys.argv[6])
    collective = sys.argv[7] if len(sys.argv) > 7 else "torch"
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                      MYRIAD_DIST_BACKEND="gloo", MYRIAD_SINGLE_DEVICE="1", MYRIAD_DP_COLLECTIVE=collective, MYRIAD_DP_GRAD_DTYPE="f32")
    if collective == "ctx":
        os.environ["MYRIAD_RCCL_LIB"] = sys.argv[8]
    import torch
    from myriad_amd.runner import DataParallel, init_distributed
    from tests import dp_common as C
    r, w, local = init_distributed()
    assert (r, w, local) == (rank, world, 0)
    dev = torch.device("cuda:0")
    model, cfg = C.build_model(dev)
    model.lora.base_seed = C.BASE_SEED + rank
    dp = DataParallel(dev, mode=mode)
    assert dp.world == world and dp.side is not None and (dp.ctx is not None) == (collective == "ctx")
    n = C.N_STEPS + 1
    batches = [C.batch(rank, i, cfg["vocab"], dev) for i in range(n)]
    stages = C.STAGES[rank] + [1]
    calls = {"adamw_pieces": 0, "adamw_module": 0}                # the early update forms: neither may run while clipping is on
    for name in calls:
        def wrapped(*a, _real=getattr(model.store, name), _name=name, **k):
            calls[_name] += 1
            return _real(*a, **k)
        setattr(model.store, name, wrapped)

    def snap():
        s = C.snapshot(model)
        s["ctl"] = model.store.ctl.cpu().clone()
        s["stats"] = model.grad_stats()
        return s

    def step(i):
        model.fixed_stage = stages[i]
        nxt = batches[i + 1] if i + 1 < n else None
        return float(model.train_step(batches[i], C.LRS[i % 3], 0.05, dp=dp, world=world, next_samples=nxt, max_grad_norm=max_norm,
                                      skip_nonfinite=True))
    losses = [step(i) for i in range(C.N_STEPS)]
    model.finish_update()
    if mode == "rs_ag":
        dp.gather_state(model.store)
    clean = snap()
    if rank == 1:
        at, real = model.store.module_range("lora", True)[0], model._finish_backward

        def poisoned():
            real()
            model.store.flat_g[at] = math.nan
        model._finish_backward = poisoned
    step(C.N_STEPS)
    model.finish_update()
    if mode == "rs_ag":
        dp.gather_state(model.store)
    torch.save(dict(clean=clean, after=snap(), losses=losses, calls=calls), out)
    dp.barrier()


if __name__ == "__main__":
    main()
