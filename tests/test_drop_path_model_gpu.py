"""drop_path_rate in the whole model (tiny synthetic MyriadHIP, freeze_vit: False, vit_precision: fp32, drop_path_rate 0.5 behind
vit_drop_path: True): the per-step draw is reproducible from drop_path_seed, a different seed trains differently, gradient
checkpointing and accumulation reuse the step's bits, and evaluation / generate() never drop."""
import pytest
import torch

from myriad_amd.eva_vit import drop_path_keep_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
DEPTH, RATE = 3, 0.5


def _tiny(drop_seed=11, rate=RATE, **extra):
    from myriad_amd.myriad import MyriadHIP
    from myriad_amd.synthetic import SyntheticWeights, full_config
    cfg = full_config(vit_depth=DEPTH, qf_layers=2, llm_layers=1, vocab=1024)
    w = SyntheticWeights(cfg, DEV, seed=7, arch="myriad", big_dtype=F32)
    model = MyriadHIP.from_config(dict(weights=w, device=DEV, fixed_stage=1, fixed_taskstage=0, freeze_vit=False,
                                       vit_precision="fp32", drop_path_rate=rate, vit_drop_path=True, drop_path_seed=drop_seed,
                                       **extra))
    return cfg, model


def _samples(vocab, seed=3):
    from tests import golden_utils as gu
    image, maps, before, after, tgt, tmask = gu.synthetic_batch(2, vocab, seed=seed)
    return dict(image=image, anomaly_maps=maps, oneshot_anomaly_maps=maps, before_ids=before, after_ids=after,
                target_ids=tgt, target_mask=tmask)


def _two_steps(model, batches, **kw):
    model.train()
    losses = [float(model.train_step(b, lr=1e-3, **kw)) for b in batches]
    model.finish_update()
    torch.cuda.synchronize()
    return losses


def _bits(seed, step, micro=0):
    return drop_path_keep_bits(seed, 0, step, micro, DEPTH, 2, RATE)


def test_same_seed_same_run_other_seed_other_run():
    # the two seeds' draws differ in the first step, and seed 11 drops something in it (a host fact, checked here)
    assert not torch.equal(_bits(11, 0), _bits(12, 0)) and not bool(_bits(11, 0).all())
    cfg, a = _tiny(11)
    _, b = _tiny(11)
    _, c = _tiny(12)
    _, d = _tiny(11, use_grad_checkpoint=True)
    assert a.drop_path_rate == RATE and a.drop_path_seed == 11 and d.vit_checkpoint
    batches = [_samples(cfg["vocab"], seed=20 + i) for i in range(2)]
    la, lb, lc, ld = (_two_steps(m, batches) for m in (a, b, c, d))
    assert a.drop_path_step == 2 and a._drop_micro == 0
    assert a.vit.last_drop_stats["branch_rows_run"] == int(_bits(11, 1).sum()) * a.vit.last_drop_stats["branch_rows_dense"] // (4 * DEPTH)
    assert la == lb and torch.equal(a.store.flat_p, b.store.flat_p)
    assert la == ld and torch.equal(a.store.flat_p, d.store.flat_p)            # recomputation reuses the step's bits
    assert la != lc and not torch.equal(a.store.flat_p, c.store.flat_p)


def test_accumulation_draws_per_micro_step_and_evaluation_never_drops():
    assert not torch.equal(_bits(11, 0, 0), _bits(11, 0, 1))
    cfg, a = _tiny(11)
    _, b = _tiny(11)
    _, z = _tiny(11, rate=0)
    assert z.drop_path_rate == 0.0
    batches = [_samples(cfg["vocab"], seed=30 + i) for i in range(2)]
    la = _two_steps(a, batches, accum_grad_iters=2)
    lb = _two_steps(b, batches, accum_grad_iters=2)
    assert la == lb and torch.equal(a.store.flat_p, b.store.flat_p)
    assert a.drop_path_step == 1 and a._drop_micro == 0                          # one update; the window's two forwards were micro 0, 1
    # evaluation and generate(): the weights of the rate-0 model, then the same loss and the same tokens
    z.load_state_dict(a.state_dict())
    a.eval(); z.eval()
    s = batches[0]
    with torch.no_grad():
        assert float(a(s)["loss"]) == float(z(s)["loss"])
    ia = a.generate(s, max_new_tokens=6)["token_ids"]
    iz = z.generate(s, max_new_tokens=6)["token_ids"]
    assert [list(map(int, r)) for r in ia] == [list(map(int, r)) for r in iz]
    assert a._drop_micro == 0                                                    # nothing was drawn
