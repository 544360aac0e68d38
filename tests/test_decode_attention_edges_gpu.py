"""The one-query decode attention kernels against fp64 at their edges, element by element, under the bound derived from their own
operation order (tests/fp64_bounds.py: decode_attn_ref_bound -- fp32 probabilities, no u16 term on P|V|):

    attn_decode_kernel<ROWS>      mh_attn_decode_rope, mh_attn_decode_rope_rows, mh_attn_fwd with Sq = 1 (and its lse)
    attn_decode_split_kernel + attn_decode_combine_kernel      mh_attn_decode_rope_split, mh_attn_decode_rope_split_rows
    attn_decode_draft_kernel      mh_attn_decode_rope_draft, mh_attn_decode_rope_draft_rows -- directly, not through the one-row kernel

Every other decode test ties kernels to each other by bit equality (the draft kernel and the ragged one-row segments to the
one-row kernel, the fused rotary form to the unfused pair); this file is what that chain rests on.

Harness (class Launch).  Every entry is called through the C ABI with strides the wrappers cannot express: qkv rows with an
8-column border (ld_qkv = 3W + 8), cache rows of 2W + 8 columns and a batch stride with 16 elements of slack inside one
NaN-poisoned buffer, the output in a poisoned window (ldo = W + 4, a poisoned row above and below).  Cache rows at and past
kv_len[b] hold the NaN poison pattern -- one key too many is a NaN, not a small error -- except the row the launch appends.  After
every launch: the border and the k / v columns of qkv hold their bits; every bit of the cache buffer outside the appended rows
is unchanged; the appended v has its source's bits; the rotated q (where the kernel writes it back) and the appended k equal
fb.rope_bf16 outside its one-ulp ambiguity mask.  The attention reference is then computed from the device's own rotated q and
the cache after the launch, so the output carries no ambiguity term; the split kernels do not write q back and take q_err.

Lengths follow the kernels' constants (fb.DECODE_LENS: OQ_WAVES = 16 waves, the 128-key score pass in two 64-key halves, the 64-lane
softmax stride, the 8 x 16 unrolled PV group, first taken at 113 keys, and its remainder): each edge at, one below and one
above; no key (a zero row, lse = -inf); fewer keys than waves; T_cap == kv_len for 1, 64, 65; kv_len = T_cap + 5 (clamped);
T_cap = 257 (no multiple of 64) and 8192.  Chunks 128 / 256 / 512 at one key, CH - 1, CH, CH + 1, 2 CH, 2 CH + 1 and T_cap;
K = 1 / 3 / 8 = DRAFT_MAX_K draft rows whose keys come from the cache, the LDS copies and both in one pass.

mh_attn_fwd differs from the two fused entries in its refusals: D % 8 != 0 and D > 128 are MH_ERR_UNSUPPORTED there, and
Sk = 8193 is not refused (the tiled kernel takes it), so that case is asked of the fused entries only.

Largest err / bound seen on the MI355X (recorded, not asserted; every test prints its kernel's running figure):
    attn_decode_kernel (three entries) o 0.994, lse 0.266;  attn_decode_split_kernel + combine o 0.952;  attn_decode_draft_kernel o 0.980.
The output's own bf16 rounding reaches 1.0 of the bound at the bottom of a binade, so the o figures are that rounding; what the
fp32 terms of the bound catch is shown by the mutants of tests/test_fp64_bounds_cpu.py.
"""
import functools

import pytest
import torch

from myriad_amd import _lib, ops
from tests import fp64_bounds as fb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
NINF = float("-inf")
MH_OK, MH_ERR_ARG, MH_ERR_UNSUPPORTED = 0, -1, -3
WORST = {}


def _bits(t):
    return t.view(torch.int16)


def _i32(x):
    return torch.tensor(list(x), dtype=I32, device=DEV)


def _record(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    return ratio


def _report(*kernels):
    for kn in kernels:
        print(f"[decode-bound] {kn}: largest err / bound so far {WORST.get(kn, 0.0):.3f}")


class Launch:
    """The device buffers of one launch (module docstring).  qkv_h [R, 3W + 8], cache_h [B, T, 2W] bf16 on the host (left
    unchanged); valid[b]: cache rows of batch b that hold data, the rest stays poison."""

    def __init__(self, qkv_h, cache_h, cos_h, sin_h, H, D, T, valid):
        self.H, self.D, self.T, self.W, self.R, self.B = H, D, T, H * D, qkv_h.shape[0], len(valid)
        W = self.W
        assert qkv_h.shape[1] == 3 * W + 8
        self.qkv = qkv_h.to(DEV).contiguous()
        self.ld_qkv, self.ldc, self.ldo = 3 * W + 8, 2 * W + 8, W + 4
        self.bs = T * self.ldc + 16
        self.flat = fb.poisoned((self.B * self.bs,), BF16, DEV)
        self.cache = self._view(self.flat)
        for b, n in enumerate(valid):
            self.cache[b, :n] = cache_h[b, :n].to(DEV)
        self.obuf = fb.poisoned((self.R + 2, self.ldo), BF16, DEV)
        self.out = self.obuf[1:self.R + 1, :W]
        self.cos, self.sin = cos_h.to(DEV).contiguous(), sin_h.to(DEV).contiguous()
        self.scale = D ** -0.5
        self.qkv0, self.flat0 = self.qkv.clone(), self.flat.clone()

    def _view(self, flat):
        return torch.as_strided(flat, (self.B, self.T, 2 * self.W), (self.bs, self.ldc, 1))

    def out_ptr(self, row=0):
        return self.obuf[1 + row:].data_ptr()

    def fresh_out(self):
        fb.poison_(self.obuf)

    def check_side_effects(self, rot_pos, q_rows, appends, what):
        """rot_pos [R]: the rotary position of every qkv row (any value for a row nothing rotates); q_rows: the rows whose q the
        kernel rotates in place; appends [(b, cache row, qkv row)].  Returns the uncertainty masks (q, k) of the rotated rows."""
        H, D, W = self.H, self.D, self.W
        q_rows = list(q_rows)
        assert torch.equal(_bits(self.qkv[:, W:]), _bits(self.qkv0[:, W:])), f"{what}: the k / v columns or the border of qkv changed"
        qr, qe, kr, ke = fb.decode_rope_pair(self.qkv0, H, D, rot_pos, self.cos, self.sin)
        rot = torch.zeros(self.R, dtype=torch.bool, device=DEV)
        rot[torch.tensor(q_rows, dtype=torch.long, device=DEV)] = True
        assert torch.equal(_bits(self.qkv[~rot, :W]), _bits(self.qkv0[~rot, :W])), f"{what}: q of a row the kernel must not rotate changed"
        if q_rows:
            fb.assert_within(self.qkv[rot, :W].reshape(-1, H, D), qr[rot], qe[rot], f"{what}: q rotated in place")
        chk = self.flat.clone()
        chk_v, v0 = self._view(chk), self._view(self.flat0)
        for b, row, r in appends:
            fb.assert_within(self.cache[b, row, :W].view(H, D), kr[r], ke[r], f"{what}: appended k, batch {b} cache row {row}")
            assert torch.equal(_bits(self.cache[b, row, W:]), _bits(self.qkv0[r, 2 * W:3 * W])), f"{what}: appended v, batch {b}"
            chk_v[b, row] = v0[b, row]
        assert torch.equal(_bits(chk), _bits(self.flat0)), f"{what}: a cache bit outside the appended rows changed"
        fb.assert_untouched(self.obuf[0], f"{what}: the row above out")
        fb.assert_untouched(self.obuf[self.R + 1], f"{what}: the row below out")
        fb.assert_untouched(self.obuf[:, W:], f"{what}: the columns past W of out")
        return qe[rot], ke[torch.tensor([r for _, _, r in appends], dtype=torch.long, device=DEV)]

    def check_output(self, kernel, grp, lens, what, chunk=None, q=None, q_err=None, lse=None):
        """out (and lse [R, H]) against decode_attn_ref_bound of the device's rotated q (or q / q_err) and the cache as the launch
        left it; grp[r]: the cache batch of qkv row r, lens[r]: its key count (0: an exactly zero row, lse = -inf)."""
        H, D, W, T, R = self.H, self.D, self.W, self.T, self.R
        kv = self.cache.reshape(self.B, T, 2, H, D)[list(grp)]
        k, v = kv[:, :, 0].transpose(1, 2), kv[:, :, 1].transpose(1, 2)
        if q is None:
            q = self.qkv[:, :W].reshape(R, H, D)
        r = fb.decode_attn_ref_bound(q, k, v, self.scale, lens, q_err=q_err, chunk=chunk)
        ratio = fb.assert_within(self.out.reshape(R, H, D), r["o"], r["o_bound"], f"{what}: o")
        _record(kernel, ratio)
        if lse is not None:
            dead = r["lse"] == NINF
            assert bool((lse[dead] == NINF).all()), f"{what}: lse of a row without a key must be -inf"
            z = torch.zeros_like(r["lse"])
            ratio = fb.assert_within(torch.where(dead, z.float(), lse), torch.where(dead, z, r["lse"]), r["lse_bound"], f"{what}: lse")
            _record(kernel + " lse", ratio)
        return r


def _L():
    return _lib.load()


def _p(t):
    return None if t is None else t.data_ptr()


def _call_rope(c, pos, pos_dev, kv_len, **over):
    a = dict(ld_qkv=c.ld_qkv, bs=c.bs, ldc=c.ldc, ldo=c.ldo, B=c.R, H=c.H, D=c.D, T=c.T)
    a.update(over)
    return _L().mh_attn_decode_rope(_p(c.qkv), a["ld_qkv"], _p(c.flat), a["bs"], a["ldc"], _p(pos), _p(pos_dev), _p(kv_len), _p(c.cos),
                                    _p(c.sin), c.out_ptr(), a["ldo"], a["B"], a["H"], a["D"], a["T"], c.scale, ops._s())


def _call_rows(c, pos, kv_len, live, **over):
    a = dict(ld_qkv=c.ld_qkv, bs=c.bs, ldc=c.ldc, ldo=c.ldo, B=c.R, H=c.H, D=c.D, T=c.T)
    a.update(over)
    return _L().mh_attn_decode_rope_rows(_p(c.qkv), a["ld_qkv"], _p(c.flat), a["bs"], a["ldc"], _p(pos), _p(kv_len), _p(live), _p(c.cos),
                                         _p(c.sin), c.out_ptr(), a["ldo"], a["B"], a["H"], a["D"], a["T"], c.scale, ops._s())


def _call_fwd(c, lse, kv_len, Sk, causal, b0=0, B=None, **over):
    """mh_attn_fwd with Sq = 1 on batch rows b0 .. b0 + B - 1: q = the q columns of qkv, k | v = the cache rows."""
    a = dict(ldq=c.ld_qkv, ldk=c.ldc, ldv=c.ldc, ldo=c.ldo, H=c.H, D=c.D)
    a.update(over)
    B = c.R - b0 if B is None else B
    e = 2                                                                              # bytes per bf16
    return _L().mh_attn_fwd(_p(c.qkv) + b0 * c.ld_qkv * e, _p(c.flat) + b0 * c.bs * e, _p(c.flat) + (b0 * c.bs + c.W) * e, c.out_ptr(b0),
                            None if lse is None else _p(lse) + b0 * c.H * 4, None, None if kv_len is None else _p(kv_len) + b0 * 4,
                            B, a["H"], 1, Sk, a["D"], c.ld_qkv, a["ldq"], c.bs, a["ldk"], c.bs, a["ldv"], a["ldo"], a["ldo"], c.scale,
                            causal, ops._s())


def _share(masks, what):
    fb.assert_rope_exempt_share(torch.cat([m.reshape(-1, m.shape[-1]) for m in masks]), what)


# ----------------------------------------------------------------------------------------------------------- one-row kernel
@functools.lru_cache(maxsize=None)
def _host_case(D, H, T):
    return fb.decode_attn_inputs(3, H, D, T, fb.decode_seed(D, H))


def _run_rope(D, H, T, lens, pos, inputs=None, kernel="attn_decode_kernel"):
    """mh_attn_decode_rope: every row appends at the shared cache row (the shortest row's last key), rotary at its own pos."""
    ns = [min(n, T) for n in lens]
    app = max(min(ns) - 1, 0)
    c = Launch(*(inputs or _host_case(D, H, T)), H, D, T, ns)
    rc = _call_rope(c, _i32(pos), _i32([app]), _i32(lens))
    torch.cuda.synchronize()
    assert rc == MH_OK
    what = f"decode_rope D={D} H={H} T_cap={T} kv_len={lens}"
    qe, ke = c.check_side_effects(pos, range(c.R), [(b, app, b) for b in range(c.R)], what)     # one append per batch row
    c.check_output(kernel, range(c.R), lens, what)
    return qe, ke


@pytest.mark.parametrize("H", fb.DECODE_HS)
@pytest.mark.parametrize("D", fb.DECODE_DS)
def test_decode_rope_over_the_length_grid(D, H):
    qs, ks = zip(*[_run_rope(D, H, T, lens, pos) for T, lens, pos in fb.decode_launches()])
    _share(qs, "q"), _share(ks, "appended k")
    _report("attn_decode_kernel")


@pytest.mark.parametrize("H", fb.DECODE_HS)
@pytest.mark.parametrize("D", fb.DECODE_DS)
def test_decode_rope_rows_over_the_length_grid_with_an_idle_row(D, H):
    qs, ks = [], []
    for T, lens, pos in fb.decode_launches():
        for live in ([1, 1, 1], [1, 0, 1]) if lens[0] == 63 else ([1, 1, 1],):
            ns = [min(n, T) for n in lens]
            c = Launch(*_host_case(D, H, T), H, D, T, ns)
            rc = _call_rows(c, _i32(pos), _i32(lens), _i32(live))
            torch.cuda.synchronize()
            assert rc == MH_OK
            what = f"decode_rope_rows D={D} H={H} T_cap={T} kv_len={lens} live={live}"
            on = [b for b in range(3) if live[b]]
            qe, ke = c.check_side_effects(pos, on, [(b, pos[b], b) for b in on], what)
            c.check_output("attn_decode_kernel", range(3), [n if live[b] else 0 for b, n in enumerate(lens)], what)
            if all(live):
                qs.append(qe), ks.append(ke)
    _share(qs, "q"), _share(ks, "appended k")
    _report("attn_decode_kernel")


@pytest.mark.parametrize("H", fb.DECODE_HS)
@pytest.mark.parametrize("D", fb.DECODE_DS)
def test_attn_fwd_with_one_query_over_the_length_grid_and_its_lse(D, H):
    """mh_attn_fwd(Sq = 1): with kv_len (Sk = T_cap, causal 0 and 1) and without (one batch row per launch, Sk = its length,
    causal alternating).  Nothing is rotated or appended: qkv and the cache keep every bit."""
    for T, lens, pos in fb.decode_launches():
        ns = [min(n, T) for n in lens]
        c = Launch(*_host_case(D, H, T), H, D, T, ns)
        kvl = _i32(lens)
        for mode in ("kv_len causal=0", "kv_len causal=1", "Sk"):
            c.fresh_out()
            lbuf = fb.poisoned((3 * H + 8,), F32, DEV)
            lse = lbuf[4:4 + 3 * H]
            if mode == "Sk":
                rows = [b for b in range(3) if ns[b] > 0]
                for b in rows:
                    assert _call_fwd(c, lse, None, ns[b], b % 2, b0=b, B=1) == MH_OK
            else:
                rows = [0, 1, 2]
                assert _call_fwd(c, lse, kvl, T, int(mode[-1])) == MH_OK
            torch.cuda.synchronize()
            what = f"attn_fwd Sq=1 D={D} H={H} T_cap={T} kv_len={lens} ({mode})"
            c.check_side_effects(pos, [], [], what)
            fb.assert_untouched(lbuf[:4], what + ": before lse"), fb.assert_untouched(lbuf[4 + 3 * H:], what + ": past lse")
            if len(rows) < 3:                                                          # the rows no launch covered: still poison
                skipped = [b for b in range(3) if b not in rows]
                fb.assert_untouched(c.out[skipped], what + ": out of a row no launch covered")
                fb.assert_untouched(lse.view(3, H)[skipped], what + ": lse of a row no launch covered")
                c.out[skipped] = 0
                lse.view(3, H)[skipped] = NINF
            c.check_output("attn_decode_kernel", range(3), lens, what, lse=lse.view(3, H))
    _report("attn_decode_kernel", "attn_decode_kernel lse")


def test_decode_rope_at_8192_keys():
    D, H, T = 128, 1, 8192
    inputs = fb.decode_attn_inputs(1, H, D, T, fb.decode_seed(D, H) + 5)
    qe, ke = _run_rope(D, H, T, [T], [T - 1], inputs=inputs)
    _share([qe], "q"), _share([ke], "appended k")
    _report("attn_decode_kernel")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", fb.DECODE_EDGE_KINDS)
def test_decode_rope_score_and_value_edges(kind, D):
    H, T, lens = 2, fb.DECODE_T, fb.DECODE_EDGE_LENS
    pos = [n - 1 for n in lens]
    inputs = fb.decode_edge_inputs(kind, 3, H, D, T, fb.decode_seed(D, H) + 7, pos)
    qe, ke = _run_rope(D, H, T, lens, pos, inputs=inputs)
    if kind != "q_zero":
        _share([qe], "q")
    _share([ke], "appended k")
    _report("attn_decode_kernel")


# ------------------------------------------------------------------------------------------------------------ split kernels
def _call_split(c, rows_form, pos, pos_dev, kv_len, live, part, chunk, **over):
    a = dict(ld_qkv=c.ld_qkv, bs=c.bs, ldc=c.ldc, ldo=c.ldo, H=c.H)
    a.update(over)
    L = _L()
    if rows_form:
        return L.mh_attn_decode_rope_split_rows(_p(c.qkv), a["ld_qkv"], _p(c.flat), a["bs"], a["ldc"], _p(pos), _p(kv_len), _p(live),
                                                _p(c.cos), _p(c.sin), c.out_ptr(), a["ldo"], _p(part), part.numel(), c.R, a["H"], c.D,
                                                c.T, chunk, c.scale, ops._s())
    return L.mh_attn_decode_rope_split(_p(c.qkv), a["ld_qkv"], _p(c.flat), a["bs"], a["ldc"], _p(pos), _p(pos_dev), _p(kv_len), _p(c.cos),
                                       _p(c.sin), c.out_ptr(), a["ldo"], _p(part), part.numel(), c.R, a["H"], c.D, c.T, chunk, c.scale,
                                       ops._s())


def _run_split(D, chunk, lens, pos, rows_form, inputs, app=None, what=""):
    H, T = fb.SPLIT_HEADS, fb.split_t_cap(chunk)
    c = Launch(*inputs, H, D, T, lens)
    part = ops.attn_decode_split_ws(c.R, H, T, DEV, chunk=chunk).fill_(float("nan"))
    live = _i32([1] * c.R)
    rc = _call_split(c, rows_form, _i32(pos), None if rows_form else _i32([app]), _i32(lens), live, part, chunk)
    torch.cuda.synchronize()
    assert rc == MH_OK
    what = f"split{'_rows' if rows_form else ''} D={D} chunk={chunk} kv_len={lens} pos={pos} {what}"
    appends = [(b, pos[b] if rows_form else app, b) for b in range(c.R)]
    _, ke = c.check_side_effects(pos, [], appends, what)
    qr, qe, _, _ = fb.decode_rope_pair(c.qkv0, H, D, pos, c.cos, c.sin)
    c.check_output("attn_decode_split_kernel + combine", range(c.R), lens, what, chunk=chunk, q=qr, q_err=qe)
    return qe, ke


@pytest.mark.parametrize("D", fb.SPLIT_DS)
@pytest.mark.parametrize("chunk", fb.SPLIT_CHUNKS)
def test_split_kernels_over_the_length_grid(chunk, D):
    H, T, seed = fb.SPLIT_HEADS, fb.split_t_cap(chunk), fb.split_seed(D, chunk)
    qs, ks = [], []
    for variant, lens, pos in fb.split_launches(chunk):
        qe, ke = _run_split(D, chunk, lens, pos, True, fb.decode_attn_inputs(len(lens), H, D, T, seed), what=variant)
        if variant == "edge":
            qs.append(qe), ks.append(ke)
    _share(qs, "q"), _share(ks, "appended k")
    # the shared-row entry: the second edge launch's rows, all appending at the shortest row's last key
    _, lens, pos = fb.split_launches(chunk)[1]
    _run_split(D, chunk, lens, pos, False, fb.decode_attn_inputs(len(lens), H, D, T, seed), app=min(lens) - 1)
    # a spike of 80 in the second chunk: the other chunks' m_c - M is near -80
    inputs = fb.decode_edge_inputs("spike_50", len(lens), H, D, T, seed, pos, spike_row=chunk + 5, spike=80.0)
    _run_split(D, chunk, lens, pos, True, inputs, what="spike in chunk 1")
    _report("attn_decode_split_kernel + combine")


# ------------------------------------------------------------------------------------------------------------ draft kernels
@pytest.mark.parametrize("D", fb.DRAFT_DS)
@pytest.mark.parametrize("K", fb.DRAFT_KS)
def test_draft_kernels_against_fp64_row_by_row(K, D):
    """Row j of group g is held to the one-row bound at len = p0 + j + 1, from the device's rotated q and the cache after the
    launch (rows p0 .. p0 + j of it were appended by sibling workgroups of the same launch).  Rows form: nrow < K."""
    H, T, G = fb.DRAFT_HEADS, fb.DECODE_T, 3
    qkv_h, cache_h, cos, sin = fb.decode_attn_inputs(G * K, H, D, T, fb.draft_seed(D, K))
    qs, ks = [], []
    for p0 in fb.draft_p0(K):
        for nrow in (None, [K, max(1, K - 1), 1]):
            c = Launch(qkv_h, cache_h[:G], cos, sin, H, D, T, p0)
            pos_d, live_d, nrow_d = _i32(p0), _i32([1] * G), _i32(nrow or [K] * G)        # named: alive until the launch has run
            args = (_p(c.qkv), c.ld_qkv, _p(c.flat), c.bs, c.ldc, _p(pos_d), _p(live_d))
            tail = (_p(c.cos), _p(c.sin), c.out_ptr(), c.ldo, G, K, H, D, T, c.scale, ops._s())
            if nrow is None:
                rc = _L().mh_attn_decode_rope_draft(*args, *tail)
            else:
                rc = _L().mh_attn_decode_rope_draft_rows(*args, _p(nrow_d), *tail)
            torch.cuda.synchronize()
            assert rc == MH_OK
            what = f"draft K={K} D={D} p0={p0} nrow={nrow}"
            rows = [(g, j) for g in range(G) for j in range(K)]
            on = [g * K + j for g, j in rows if nrow is None or j < nrow[g]]
            rot_pos = [p0[g] + j for g, j in rows]
            qe, ke = c.check_side_effects(rot_pos, on, [(r // K, rot_pos[r], r) for r in on], what)
            lens = [rot_pos[r] + 1 if r in on else 0 for r in range(G * K)]
            c.check_output("attn_decode_draft_kernel", [g for g, _ in rows], lens, what)
            if nrow is None:
                qs.append(qe), ks.append(ke)
    _share(qs, "q"), _share(ks, "appended k")
    _report("attn_decode_draft_kernel")


# ---------------------------------------------------------------------------------------------------------------- refusals
def _refusal_case(H=2, D=16, T=64, B=2):
    qkv_h, cache_h, cos, sin = fb.decode_attn_inputs(B, H, D, T, 321)
    return Launch(qkv_h, cache_h, cos, sin, H, D, T, [T] * B)


def _nothing_written(c, what):
    torch.cuda.synchronize()
    assert torch.equal(_bits(c.qkv), _bits(c.qkv0)), what + ": qkv written by a refused call"
    assert torch.equal(_bits(c.flat), _bits(c.flat0)), what + ": cache written by a refused call"
    fb.assert_untouched(c.obuf, what + ": out written by a refused call")


# (what, the buffers' shape, the arguments that replace the true ones): every buffer covers its true shape, so a call that
# was not refused would still stay inside them
FUSED_REFUSALS = [
    ("D % 8 != 0", {}, dict(D=12)),
    ("D > 128", dict(H=1, D=136), {}),
    ("T_cap = 8193", dict(H=1, D=8, T=8193, B=1), {}),
    ("ld_qkv % 8", {}, dict(ld_qkv=3 * 32 + 12)),
    ("ld_cache % 8", {}, dict(ldc=2 * 32 + 4)),
    ("cache_bstride % 8", {}, dict(bs=64 * (2 * 32 + 8) + 12)),
    ("ldo % 4", {}, dict(ldo=32 + 2)),
    ("ld_qkv < 3HD", {}, dict(ld_qkv=3 * 32 - 8)),
    ("ld_cache < 2HD", {}, dict(ldc=2 * 32 - 8)),
    ("ldo < HD", {}, dict(ldo=32 - 4)),
    ("H = 0", {}, dict(H=0)),
    ("H < 0", {}, dict(H=-1)),
]


@pytest.mark.parametrize("what,shape,over", FUSED_REFUSALS, ids=[r[0] for r in FUSED_REFUSALS])
def test_fused_one_row_entries_refuse_on_their_return_code_and_write_nothing(what, shape, over):
    c = _refusal_case(**shape)
    z, n, live = _i32([0] * c.R), _i32([1] * c.R), _i32([1] * c.R)
    if not shape:
        assert _call_rope(c, z, z[:1], n) == MH_OK and _call_rows(c, z, n, live) == MH_OK      # the base arguments are accepted
        c = _refusal_case()
    assert _call_rope(c, z, z[:1], n, **over) == MH_ERR_ARG, what
    _nothing_written(c, "mh_attn_decode_rope, " + what)
    assert _call_rows(c, z, n, live, **over) == MH_ERR_ARG, what
    _nothing_written(c, "mh_attn_decode_rope_rows, " + what)


FWD_REFUSALS = [
    ("D % 8 != 0", {}, dict(D=12), MH_ERR_UNSUPPORTED),
    ("D > 128", dict(H=1, D=136), {}, MH_ERR_UNSUPPORTED),
    ("ldq % 8", {}, dict(ldq=3 * 32 + 12), MH_ERR_ARG),
    ("ldk % 8", {}, dict(ldk=2 * 32 + 4), MH_ERR_ARG),
    ("ldv % 8", {}, dict(ldv=2 * 32 + 4), MH_ERR_ARG),
    ("ldo % 4", {}, dict(ldo=32 + 2), MH_ERR_ARG),
    ("H = 0", {}, dict(H=0), MH_ERR_ARG),
    ("H < 0", {}, dict(H=-1), MH_ERR_ARG),
]


@pytest.mark.parametrize("what,shape,over,code", FWD_REFUSALS, ids=[r[0] for r in FWD_REFUSALS])
def test_attn_fwd_with_one_query_refuses_on_its_return_code_and_writes_nothing(what, shape, over, code):
    c = _refusal_case(**shape)
    n = _i32([c.T] * c.R)
    lse = fb.poisoned((c.R * max(c.H, 1),), F32, DEV)
    if not shape:
        assert _call_fwd(c, lse, n, c.T, 0) == MH_OK
        c, lse = _refusal_case(), fb.poison_(lse)
    assert _call_fwd(c, lse, n, c.T, 0, **over) == code, what
    _nothing_written(c, "mh_attn_fwd, " + what)
    fb.assert_untouched(lse, "mh_attn_fwd, " + what + ": lse")


STRIDE_REFUSALS = [("ld_qkv < 3HD", dict(ld_qkv=3 * 32 - 8)), ("ld_cache < 2HD", dict(ldc=2 * 32 - 8)), ("ldo < HD", dict(ldo=32 - 4)),
                   ("H = 0", dict(H=0)), ("H < 0", dict(H=-1))]


@pytest.mark.parametrize("what,over", STRIDE_REFUSALS, ids=[r[0] for r in STRIDE_REFUSALS])
def test_split_and_draft_entries_refuse_short_strides_and_no_heads(what, over):
    c = _refusal_case()
    z, n, live = _i32([0] * c.R), _i32([1] * c.R), _i32([1] * c.R)
    part = ops.attn_decode_split_ws(c.R, c.H, c.T, DEV, chunk=128).fill_(float("nan"))
    for rows_form in (False, True):
        assert _call_split(c, rows_form, z, z[:1], n, live, part, 128, **over) == MH_ERR_ARG, what
        _nothing_written(c, f"split (rows {rows_form}), " + what)
        assert bool(part.isnan().all()), what + ": a partial record written by a refused call"
    a = dict(ld_qkv=c.ld_qkv, ldc=c.ldc, ldo=c.ldo, H=c.H)
    a.update(over)
    K = 1
    for nrow in (None, n):
        args = (_p(c.qkv), a["ld_qkv"], _p(c.flat), c.bs, a["ldc"], _p(z), _p(live))
        tail = (_p(c.cos), _p(c.sin), c.out_ptr(), a["ldo"], c.R, K, a["H"], c.D, c.T, c.scale, ops._s())
        rc = _L().mh_attn_decode_rope_draft(*args, *tail) if nrow is None else _L().mh_attn_decode_rope_draft_rows(*args, _p(nrow), *tail)
        assert rc == MH_ERR_ARG, what
        _nothing_written(c, f"draft (rows {nrow is not None}), " + what)
