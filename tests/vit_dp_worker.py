"""One data-parallel rank of tests/test_vit_finetune_dp_gpu.py: `python tests/vit_dp_worker.py RANK WORLD PORT MODE OUT`, and the
model / batches / stages that test shares with its ranks.  As tests/dp_worker.py: every rank sits on cuda:0, the process group is
gloo, the exchange goes through runner.DataParallel with the overlap on -- here with a trainable ViT (freeze_vit: False), so the
flat buffer carries visual_encoder.* and ln_vision.* behind the map tokenizer's early segment, rs_ag shards their Adam moments, and
the parameters gathered after the update are what the next step's refresh reads."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# prompt stage per rank per step: ragged use of VETokenizer / VEInstructor as in tests/dp_common.py; the ViT is used by every step
STAGES = {0: [1, 0, 2], 1: [2, 0, 1]}
N_STEPS = 3
LRS = [1e-3, 8e-4, 6e-4]


def build_model(dev):
    import torch
    from myriad_amd.myriad import MyriadHIP
    from myriad_amd.synthetic import SyntheticWeights, full_config
    cfg = full_config(vit_depth=2, qf_layers=2, llm_layers=1, vocab=1024)
    torch.manual_seed(1234)                         # trainable init (identical on every rank, as DDP broadcasts rank 0's)
    w = SyntheticWeights(cfg, dev, seed=7, big_dtype=torch.float32)
    return MyriadHIP(w, dict(fixed_stage=1, fixed_taskstage=0, freeze_vit=False), device=dev), cfg


def main():
    rank, world, port, mode, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                      MYRIAD_DIST_BACKEND="gloo", MYRIAD_SINGLE_DEVICE="1", MYRIAD_DP_COLLECTIVE="torch", MYRIAD_DP_GRAD_DTYPE="f32")
    import torch
    from myriad_amd.runner import DataParallel, init_distributed
    from tests import dp_common as C
    r, w, local = init_distributed()
    assert (r, w, local) == (rank, world, 0)
    dev = torch.device("cuda:0")
    model, cfg = build_model(dev)
    assert model.train_vit
    dp = DataParallel(dev, mode=mode)
    assert dp.world == world and dp.side is not None
    batches = [C.batch(rank, i, cfg["vocab"], dev) for i in range(N_STEPS)]
    losses = []
    for i in range(N_STEPS):
        model.fixed_stage = STAGES[rank][i]
        nxt = batches[i + 1] if i + 1 < N_STEPS else None
        losses.append(model.train_step(batches[i], LRS[i], 0.05, dp=dp, world=world, overlap=True, next_samples=nxt))
    model.finish_update()
    segs, shards = dp.segments(model.store.total), dp.shards(model.store.total)
    complete_before_gather = model.store.moments_complete
    if mode == "rs_ag":
        dp.gather_state(model.store)
    snap = C.snapshot(model)
    snap.update(losses=[float(l) for l in losses], segments=segs, shards=shards, complete_before_gather=complete_before_gather)
    torch.save(snap, out)
    dp.barrier()


if __name__ == "__main__":
    main()
