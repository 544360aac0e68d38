"""The stochastic-depth row kernels (drop_path.hip) element by element against float64, outputs poisoned first.

Bounds (tests/fp64_bounds.py):
    residual scatter   h_out = fma(scale, y, h): one rounding, u32 |h_out|; a dropped row keeps h's bits (torch.equal).
    LayerNorm          of the h_out the kernel wrote (the values it holds in registers): layernorm_ref_bound's y_bf16_bound.
    LayerNorm backward layernorm_ref_bound's dx_bound on the kept rows (the same expressions as layernorm_bwd_kernel);
                       a dropped row keeps dres's bits.  The bf16 copy is bf16(out_scale * dx) of the dx the kernel wrote: one
                       fp32 product (u32) and the bf16 rounding.
    parameter grads    layernorm_param_grads_ref_bound over the compact rows (16 rows a block, blocks in order: the same
                       summation structure as mh_layernorm_param_grads with M = K N rows).
    gather-scale       bf16(scale * src): u32 and the bf16 rounding.
Shapes: the LayerNorm widths of tests/test_row_kernels_edges_gpu.py (1408 = the ViT; 2048 / 4096 are where the kernels change
their register tiling), B = 4 samples of N = 1, 3, 257 rows; keep sets none, all, first, last, {0, 2}; scales 1 and 1 / 0.6."""
import pytest
import torch

from myriad_amd import _lib, ops
from tests import fp64_bounds as fb
from tests.fp64_bounds import U32, assert_untouched, assert_within, poisoned, poisoned_allocations

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
B = 4
NORM_D = [4, 252, 256, 1028, 1408, 4096, 4100, 8192]
ROWS = [1, 3, 257]
KEEPS = [[], [0, 1, 2, 3], [0], [3], [0, 2]]
SCALES = [1.0, 1.0 / 0.6]
EPS = 1e-6


def dev(t):
    return t.to(DEV)


def _map(samples):
    return ops.DropPathMap.from_keep([b in samples for b in range(B)])


def _rows(samples, N):
    """Row indices of the samples' rows in the full [B*N, D] stream, in compact order."""
    return torch.cat([torch.arange(s * N, (s + 1) * N) for s in samples] + [torch.zeros(0, dtype=torch.int64)]).to(DEV)


def _other(samples):
    return [b for b in range(B) if b not in samples]


def _show(name, ratio):
    print(f"RATIO {name} {ratio:.3g}")


@pytest.mark.parametrize("D", NORM_D)
@pytest.mark.parametrize("N", ROWS)
def test_residual_scatter_layernorm(N, D, monkeypatch):
    M = B * N
    h, w, bb = dev(fb.norm_rows(M, D, seed=100 + D)), dev(fb.norm_weight(D, seed=200 + D)), dev(0.1 * fb.rnd(D, seed=500 + D))
    for ki, kin in enumerate(KEEPS):
        for si, scale in enumerate(SCALES):
            kout = KEEPS[(ki + si + 1) % len(KEEPS)]
            y = dev(fb.rnd(len(kin) * N, D, seed=300 + D + ki)) if kin else None
            with poisoned_allocations(monkeypatch):
                if kin:
                    if kout:
                        h_out, xn = ops.drop_path_residual_layernorm(h, y, _map(kin), scale, N, w, bb, EPS,
                                                                     keep_out=None if len(kout) == B and si else _map(kout))
                    else:                                           # the form without the norm (the last block's fc2)
                        h_out, xn = ops.drop_path_residual_layernorm(h, y, _map(kin), scale, N)
                elif kout:                                          # no branch: the norm of the stream itself, compact
                    h_out, xn = ops.drop_path_residual_layernorm(h, None, None, scale, N, w, bb, EPS, keep_out=_map(kout),
                                                                 want_h=False)
                else:
                    continue
            torch.cuda.synchronize()
            what = f"keep_in {kin} keep_out {kout} scale {scale:.3g}"
            if kin:
                rk, rd = _rows(kin, N), _rows(_other(kin), N)
                ref = h.double()
                ref[rk] = ref[rk] + fb.f32_value(scale) * y.double()
                assert torch.equal(h_out[rd], h[rd]), f"{what}: a dropped row changed"
                _show("residual f32", assert_within(h_out, ref, U32 * ref.abs() + 2.0 ** -149, f"h_out ({what})"))
            else:
                assert h_out is None
                h_out = h
            if kout:
                ro = _rows(kout, N)
                assert tuple(xn.shape) == (len(kout) * N, D) and xn.dtype == BF16
                r = fb.layernorm_ref_bound(h_out[ro], w, bb, EPS)
                _show("layernorm bf16", assert_within(xn, r["y"], r["y_bf16_bound"], f"xn ({what})"))
            else:
                assert xn is None


@pytest.mark.parametrize("D", NORM_D)
@pytest.mark.parametrize("N", ROWS)
def test_layernorm_backward_scatter(N, D, monkeypatch):
    M = B * N
    x, w = dev(fb.norm_rows(M, D, seed=100 + D)), dev(fb.norm_weight(D, seed=200 + D))
    dres = dev(fb.rnd(M, D, seed=400 + D))
    for ki, kin in enumerate(KEEPS[1:]):
        for si, scale in enumerate(SCALES):
            kout = KEEPS[(ki + si + 1) % len(KEEPS)]
            dy = dev(fb.rnd(len(kin) * N, D, seed=300 + D + ki))
            with poisoned_allocations(monkeypatch):
                dx, dxb = ops.drop_path_layernorm_bwd(dy, x, w, EPS, dres, _map(kin), N,
                                                      keep_out=(None if len(kout) == B and si else _map(kout)) if kout else None,
                                                      out_scale=scale, want_bf16=bool(kout))
            torch.cuda.synchronize()
            what = f"keep_in {kin} keep_out {kout} scale {scale:.3g}"
            rk, rd = _rows(kin, N), _rows(_other(kin), N)
            assert torch.equal(dx[rd], dres[rd]), f"{what}: a dropped row's gradient changed"
            r = fb.layernorm_ref_bound(x[rk], w, None, EPS, dy=dy, dres=dres[rk])
            _show("layernorm_bwd f32", assert_within(dx[rk], r["dx"], r["dx_bound"], f"dx ({what})"))
            if kout:
                ro = _rows(kout, N)
                assert tuple(dxb.shape) == (len(kout) * N, D) and dxb.dtype == BF16
                ref = fb.f32_value(scale) * dx[ro].double()
                _show("scaled gradient bf16", assert_within(dxb, ref, fb.bf16_out(ref, U32 * ref.abs() + 2.0 ** -149),
                                                             f"dx bf16 ({what})"))
            else:
                assert dxb is None


@pytest.mark.parametrize("D", NORM_D)
@pytest.mark.parametrize("N", ROWS)
def test_layernorm_param_grads_over_kept_rows(N, D, monkeypatch):
    M = B * N
    x = dev(fb.norm_rows(M, D, seed=100 + D))
    for ki, kin in enumerate(KEEPS[1:]):
        dy, dy2 = dev(fb.rnd(len(kin) * N, D, seed=300 + D + ki)), dev(fb.rnd(len(kin) * N, D, seed=350 + D + ki))
        dg, db = poisoned((D,), F32, DEV), poisoned((D,), F32, DEV)
        if D > 4096:                                                # a column block is held in registers
            with pytest.raises(ValueError):
                ops.drop_path_layernorm_param_grads(dy, x, EPS, _map(kin), N, dg, db)
            torch.cuda.synchronize()
            assert_untouched(dg), assert_untouched(db)
            continue
        with poisoned_allocations(monkeypatch):
            ops.drop_path_layernorm_param_grads(dy, x, EPS, _map(kin), N, dg, db)
        torch.cuda.synchronize()
        rg, eg, rb, eb = fb.layernorm_param_grads_ref_bound(dy, x[_rows(kin, N)], EPS)
        _show("dgamma", assert_within(dg, rg, eg, f"dgamma (keep {kin})"))
        _show("dbeta", assert_within(db, rb, eb, f"dbeta (keep {kin})"))
        # the accumulate form: one rounded sum of two single calls
        dg2, db2 = poisoned((D,), F32, DEV), poisoned((D,), F32, DEV)
        acc_g, acc_b = dg.clone(), db.clone()
        with poisoned_allocations(monkeypatch):
            ops.drop_path_layernorm_param_grads(dy2, x, EPS, _map(kin), N, dg2, db2)
            ops.drop_path_layernorm_param_grads(dy2, x, EPS, _map(kin), N, acc_g, acc_b, accumulate=True)
        torch.cuda.synchronize()
        assert torch.equal(acc_g, dg + dg2) and torch.equal(acc_b, db + db2)


@pytest.mark.parametrize("N,D", [(1, 4), (3, 1408), (257, 1408), (3, 8192)])
def test_gather_scale(N, D, monkeypatch):
    src = dev(fb.norm_rows(B * N, D, seed=7 + D))
    for kout in KEEPS[1:]:
        for scale in SCALES:
            with poisoned_allocations(monkeypatch):
                got = ops.drop_path_gather_scale(src, _map(kout), scale, N)
            torch.cuda.synchronize()
            ref = fb.f32_value(scale) * src[_rows(kout, N)].double()
            assert_within(got, ref, fb.bf16_out(ref, U32 * ref.abs() + 2.0 ** -149), f"gather_scale keep {kout}")
    with poisoned_allocations(monkeypatch):
        full = ops.drop_path_gather_scale(src, None, 1.0, N)
    torch.cuda.synchronize()
    assert torch.equal(full, ops.to_bf16(src))


class _NoLaunch:
    """Stands in for the library: any drop-path entry reached means a wrapper let a bad argument through."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.startswith("mh_drop_path") and not name.endswith("_ws_floats"):
            raise AssertionError(f"{name} was reached")
        return getattr(self._lib, name)


def test_wrappers_refuse_before_any_launch(monkeypatch):
    N, D = 3, 64
    M = B * N
    h, w, bb = dev(fb.rnd(M, D, seed=1)), dev(fb.norm_weight(D, seed=2)), dev(fb.rnd(D, seed=3))
    y2, y3 = dev(fb.rnd(2 * N, D, seed=4)), dev(fb.rnd(3 * N, D, seed=5))
    dg, db = poisoned((D,), F32, DEV), poisoned((D,), F32, DEV)
    lib = ops._L()
    monkeypatch.setattr(ops, "_L", lambda: _NoLaunch(lib))
    ok = [0, -1, 1, -1]
    bad_maps = [[0, 0, -1, -1], [0, 2, -1, -1], [1, -1, -1, -1], [0, -1, 4, -1], [0, -2, 1, -1], [0, -1, 1], [0, -1, 1, -1, -1],
                torch.tensor(ok, dtype=torch.int32, device=DEV), [0.0, -1.0, 1.0, -1.0]]
    for m in bad_maps:
        with pytest.raises(ValueError):
            ops.drop_path_residual_layernorm(h, y2, m, 1.0, N, w, bb, EPS)
        with pytest.raises(ValueError):
            ops.drop_path_residual_layernorm(h, y2, ok, 1.0, N, w, bb, EPS, keep_out=m)
        with pytest.raises(ValueError):
            ops.drop_path_layernorm_bwd(y2, h, w, EPS, h.clone(), m, N)
        with pytest.raises(ValueError):
            ops.drop_path_layernorm_bwd(y2, h, w, EPS, h.clone(), ok, N, keep_out=m)
        with pytest.raises(ValueError):
            ops.drop_path_gather_scale(h, m, 1.0, N)
        with pytest.raises(ValueError):
            ops.drop_path_layernorm_param_grads(y2, h, EPS, m, N, dg, db)
    calls = [
        lambda: ops.drop_path_residual_layernorm(h, y3, ok, 1.0, N, w, bb, EPS),                   # |Kset| N != rows of y
        lambda: ops.drop_path_residual_layernorm(h, y2.to(BF16), ok, 1.0, N, w, bb, EPS),          # y must be f32
        lambda: ops.drop_path_residual_layernorm(h, y2[:, :60], ok, 1.0, N, w, bb, EPS),
        lambda: ops.drop_path_residual_layernorm(h, y2, ok, 1.0, 5, w, bb, EPS),                   # rows no multiple of N
        lambda: ops.drop_path_residual_layernorm(h, y2, ok, 1.0, N, w, None, EPS),
        lambda: ops.drop_path_residual_layernorm(h, y2, ok, 1.0, N, w[:60], bb[:60], EPS),
        lambda: ops.drop_path_residual_layernorm(h, y2, ok, 1.0, N, keep_out=ok),                  # a map for a norm that is not run
        lambda: ops.drop_path_residual_layernorm(h, None, ok, 1.0, N, w, bb, EPS),                 # a map without a branch
        lambda: ops.drop_path_residual_layernorm(h, None, None, 1.0, N),                           # nothing to do
        lambda: ops.drop_path_residual_layernorm(h, y2, ok, 1.0, N, w, bb, EPS, keep_out=[-1] * 4),
        lambda: ops.drop_path_residual_layernorm(h.cpu(), y2, ok, 1.0, N, w, bb, EPS),
        lambda: ops.drop_path_residual_layernorm(dev(fb.rnd(M, 66, seed=6)), dev(fb.rnd(2 * N, 66, seed=7)), ok, 1.0, N),   # D % 4
        lambda: ops.drop_path_layernorm_bwd(y3, h, w, EPS, h.clone(), ok, N),
        lambda: ops.drop_path_layernorm_bwd(y2, h, w, EPS, h[:6], ok, N),
        lambda: ops.drop_path_layernorm_bwd(y2, h, w, EPS, h.clone(), [-1] * 4, N),
        lambda: ops.drop_path_layernorm_bwd(y2, h, w, EPS, h.clone(), ok, N, keep_out=ok, want_bf16=False),
        lambda: ops.drop_path_gather_scale(h, [-1] * 4, 1.0, N),
        lambda: ops.drop_path_gather_scale(h.to(BF16), ok, 1.0, N),
        lambda: ops.drop_path_layernorm_param_grads(y3, h, EPS, ok, N, dg, db),
        lambda: ops.drop_path_layernorm_param_grads(y2, h, EPS, ok, N, dg[:60], db),
        lambda: ops.drop_path_layernorm_param_grads(y2, h, EPS, [-1] * 4, N, dg, db),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was accepted")
    torch.cuda.synchronize()
    assert_untouched(dg), assert_untouched(db)


def test_launchers_check_the_map_themselves():
    """The C entry points read the host map before they launch: a map the wrappers would have refused is MH_ERR_ARG, more than
    64 samples MH_ERR_UNSUPPORTED, and no output is written."""
    N, D = 3, 64
    M = B * N
    L = ops._L()
    s = torch.cuda.current_stream().cuda_stream
    h, w, bb = dev(fb.rnd(M, D, seed=1)), dev(fb.norm_weight(D, seed=2)), dev(fb.rnd(D, seed=3))
    y = dev(fb.rnd(2 * N, D, seed=4))
    h_out, xn, dxb = poisoned((M, D), F32, DEV), poisoned((M, D), BF16, DEV), poisoned((M, D), BF16, DEV)
    dg, db, ws = poisoned((D,), F32, DEV), poisoned((D,), F32, DEV), poisoned((4096,), F32, DEV)
    p = lambda t: t.data_ptr()
    for slot, K in (([0, 0, -1, -1], 2), ([0, 2, -1, -1], 2), ([0, -1, 1, -1], 3), ([0, -1, 1, -1], 1), ([0, -1, 5, -1], 2),
                    ([0, -3, 1, -1], 2), ([-1] * 4, 0)):
        m = torch.tensor(slot, dtype=torch.int32)
        assert L.mh_drop_path_residual_layernorm(p(h), p(y), p(m), K, 1.0, p(w), p(bb), None, B, p(h_out), p(xn), B, N, D, EPS, s) == -1
        assert L.mh_drop_path_residual_layernorm(p(h), None, None, 0, 1.0, p(w), p(bb), p(m), K, None, p(xn), B, N, D, EPS, s) == -1
        assert L.mh_drop_path_layernorm_bwd(p(y), p(h), p(w), p(h), p(m), K, None, B, 1.0, p(h_out), p(dxb), B, N, D, EPS, s) == -1
        assert L.mh_drop_path_gather_scale(p(h), p(m), K, 1.0, p(dxb), B, N, D, s) == -1
        assert L.mh_drop_path_layernorm_param_grads(p(y), p(h), p(m), K, p(dg), p(db), B, N, D, EPS, 0, p(ws), 4096, s) == -1
    ok = torch.tensor([0, -1, 1, -1], dtype=torch.int32)
    assert L.mh_drop_path_residual_layernorm(p(h), p(y), p(ok), 2, 1.0, p(w), p(bb), None, B, p(h), p(xn), B, N, D, EPS, s) == -1   # in place
    assert L.mh_drop_path_layernorm_param_grads(p(y), p(h), p(ok), 2, p(dg), p(db), B, N, D, EPS, 0, p(ws), 8, s) == -1   # short scratch
    big = torch.arange(65, dtype=torch.int32)
    assert L.mh_drop_path_gather_scale(p(h), p(big), 65, 1.0, p(dxb), 65, 1, D, s) == -3
    assert L.mh_drop_path_gather_scale(p(h), p(ok), 2, 1.0, p(dxb), B, N, 66, s) == -1
    torch.cuda.synchronize()
    for t in (h_out, xn, dxb, dg, db, ws):
        assert_untouched(t)
    with pytest.raises(_lib.MyriadHipError):
        _lib.check(-3, "mh_drop_path_gather_scale")
