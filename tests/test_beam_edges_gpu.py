"""mh_beam_topk and mh_beam_reorder_kv at their edges, against tests/beam_topk_ref.py: exact indices (ties, non-finite rows and
the ban included), every score within its per-element bound, every output a window inside a poisoned buffer, logit rows padded
with NaN and with +inf, caches cut from the middle of poisoned allocations, the refusals of the C ABI and of the wrappers.
tests/test_beam_edges_cpu.py holds the reference itself to account (decisive random cases, hand-written tie answers)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myriad_amd import _lib, ops  # noqa: E402
from tests import beam_topk_ref as BR  # noqa: E402
from tests.fp64_bounds import assert_frame_untouched, assert_untouched, poisoned, untouched  # noqa: E402

DEV = "cuda"
F32, I32, BF16 = torch.float32, torch.int32, torch.bfloat16
PAD = 8                       # elements in front of and behind every window
LDL_EXTRA = 5                 # logit columns past V, filled with what a row must never read
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3


def _win(n, dtype):
    """(buffer, window): n contiguous elements inside a poisoned [1, n + 2 PAD] buffer."""
    buf = poisoned((1, n + 2 * PAD), dtype, DEV)
    return buf, buf[0, PAD:PAD + n]


def _frames_untouched(wins, what):
    for name, (buf, w) in wins.items():
        assert_frame_untouched(buf, slice(0, 1), slice(PAD, PAD + w.numel()), f"{what} {name}")


def _all_untouched(wins, what):
    for name, (buf, _) in wins.items():
        assert_untouched(buf, f"{what} {name}")


def _topk_buffers(R, B, K):
    return dict(part_s=_win(R * K, F32), part_i=_win(R * K, I32), out_s=_win(B * K, F32), out_i=_win(B * K, I32))


def _device_logits(c, fill):
    host = torch.full((c.logits.shape[0], c.V + LDL_EXTRA), fill, dtype=F32)
    host[:, :c.V] = c.logits
    return host, host.to(DEV)


def _launch(c, fill, ban=None):
    """One ops.beam_topk of a case; (out_s [B, K], out_i [B, K], part_s [R, K], part_i [R, K]) on the host, after the checks
    every launch gets: frames untouched, inputs unchanged, every owned element written."""
    R, K = c.logits.shape[0], c.K
    host, dev = _device_logits(c, fill)
    sbuf, scores = _win(R, F32)
    scores.copy_(c.scores)
    wins = _topk_buffers(R, c.B, K)
    ops.beam_topk(dev[:, :c.V], scores, wins["part_s"][1], wins["part_i"][1], wins["out_s"][1], wins["out_i"][1], c.B, c.nb,
                  ban_id=c.ban if ban is None else ban)
    torch.cuda.synchronize()
    _frames_untouched(dict(wins, scores=(sbuf, scores)), c.name)
    assert torch.equal(dev.cpu().view(I32), host.view(I32)) and torch.equal(scores.cpu().view(I32), c.scores.view(I32))
    for name, (_, w) in wins.items():
        assert not bool(untouched(w).any()), f"{c.name}: {name} has elements nothing wrote"
    return (wins["out_s"][1].cpu().view(c.B, K), wins["out_i"][1].cpu().view(c.B, K).long(),
            wins["part_s"][1].cpu().view(R, K), wins["part_i"][1].cpu().view(R, K).long())


def _bits(t):
    return t.contiguous().view(I32)


def _check(c, got, ban=None):
    """Everything a case asks of one launch's result; returns the worst error-to-bound ratio of out_s."""
    out_s, out_i, part_s, part_i = got
    r, K, V = BR.ref(c.name), c.K, c.V
    ban = c.ban if ban is None else ban
    assert not bool((out_i == BR.PLACEHOLDER).any()) and not bool((part_i == BR.PLACEHOLDER).any())
    assert not bool(torch.isnan(out_s).any()) and not bool(torch.isnan(part_s).any())
    assert torch.equal(out_i, r.idx), (c.name, out_i, r.idx)
    worst = BR.check_scores(out_s, torch.gather(r.s64, 1, r.idx), torch.gather(r.bound, 1, r.idx), c.name)
    assert bool((out_s[:, :-1] >= out_s[:, 1:]).all()), (c.name, out_s)
    # the row records: tokens of the row, each once, best first, never the banned one
    assert bool(((part_i >= 0) & (part_i < V)).all())
    assert all(len(set(row)) == K for row in part_i.tolist())
    assert bool((part_s[:, :-1] >= part_s[:, 1:]).all())
    if 0 <= ban < V:
        assert not bool((out_i % V == ban).any()) and not bool((part_i == ban).any())
    if c.rpi == 1:                                                      # one row per item: the record is the row's
        assert torch.equal(part_i, out_i) and torch.equal(_bits(part_s), _bits(out_s))
    if c.want is not None:
        assert np.array_equal(out_i.numpy(), c.want), (c.name, out_i, c.want)
    for row, toks in c.part_want.items():
        assert part_i[row].tolist() == list(toks), (c.name, row, part_i[row], toks)
    for b, k0, k1 in c.bit_equal:
        assert bool((_bits(out_s[b, k0:k1]) == _bits(out_s[b, k0:k0 + 1])).all()), (c.name, b, k0, k1, out_s[b])
    if c.exact_s is not None:
        assert np.array_equal(out_s.numpy().view(np.int32), c.exact_s.view(np.int32)), (c.name, out_s)
    return worst


def _run_both_fills(name):
    c = BR.case(name)
    worst = 0.0
    for fill in (float("nan"), float("inf")):                           # a read past V poisons the row maximum or the sum
        worst = max(worst, _check(c, _launch(c, fill)))
    print(f"{name}: worst |out_s - s64| / bound = {worst:.3f}")


@pytest.mark.parametrize("name", BR.names("rand"))
def test_topk_accuracy_and_order(name):
    _run_both_fills(name)


@pytest.mark.parametrize("name", BR.names("tie", "const", "rows"))
def test_topk_ties(name):
    _run_both_fills(name)


@pytest.mark.parametrize("name", BR.names("nonfinite"))
def test_topk_non_finite(name):
    _run_both_fills(name)
    c = BR.case(name)
    if c.twin is not None:                                              # row 1 never ranks: no flat index of row 1 in the record
        out_i = _launch(c, float("nan"))[1]
        assert not bool(((out_i // c.V) == 1).any())


@pytest.mark.parametrize("name", BR.names("ban"))
def test_topk_ban(name):
    _run_both_fills(name)
    c = BR.case(name)
    if c.twin is not None:                                              # a ban outside [0, V) bans nothing
        assert torch.equal(BR.ref(name).idx, BR.ref(c.twin).idx)
    if name == "ban-argmax":
        assert bool((c.logits.argmax(1) == c.ban).all())


# ---------------------------------------------------------------------------------------------------------------- advance
def _abi_args(c, dev, scores, wins, pos=None, kvlen=None, n_adv=0):
    p = lambda t: None if t is None else t.data_ptr()                   # noqa: E731
    return [p(dev), dev.stride(0), p(scores), p(wins["part_s"][1]), p(wins["part_i"][1]), p(wins["out_s"][1]), p(wins["out_i"][1]),
            c.B, c.rpi, c.nb, c.V, c.ban, p(pos), p(kvlen), n_adv, torch.cuda.current_stream().cuda_stream]


@pytest.mark.parametrize("n_adv", [1, 9, 300])
def test_topk_advances_exactly_the_rows_it_is_given(n_adv):
    c = BR.case("rand-nb3-B3-rpi3-V1023")
    _, dev = _device_logits(c, float("nan"))
    scores = c.scores.to(DEV)
    wins = _topk_buffers(9, c.B, c.K)
    pbuf, pos = _win(n_adv, I32)
    kbuf, kvlen = _win(n_adv, I32)
    pos0, kv0 = torch.arange(n_adv, dtype=I32) * 3 + 7, torch.arange(n_adv, dtype=I32) + 100
    pos.copy_(pos0)
    kvlen.copy_(kv0)
    ops.beam_topk(dev[:, :c.V], scores, wins["part_s"][1], wins["part_i"][1], wins["out_s"][1], wins["out_i"][1], c.B, c.nb,
                  ban_id=c.ban, pos=pos, kvlen=kvlen)
    torch.cuda.synchronize()
    assert torch.equal(pos.cpu(), pos0 + 1) and torch.equal(kvlen.cpu(), kv0 + 1)
    _frames_untouched(dict(wins, pos=(pbuf, pos), kvlen=(kbuf, kvlen)), "advance")
    assert torch.equal(wins["out_i"][1].cpu().view(c.B, c.K).long(), BR.ref(c.name).idx)
    # one of the two alone advances nothing (the step's record is still written); B = 0 does nothing at all
    L = _lib.load()
    for kw in (dict(pos=pos), dict(kvlen=kvlen)):
        assert L.mh_beam_topk(*_abi_args(c, dev, scores, wins, n_adv=n_adv, **kw)) == OK
    torch.cuda.synchronize()
    assert torch.equal(pos.cpu(), pos0 + 1) and torch.equal(kvlen.cpu(), kv0 + 1)
    wins = _topk_buffers(9, c.B, c.K)
    args = _abi_args(c, dev, scores, wins, pos=pos, kvlen=kvlen, n_adv=n_adv)
    args[7] = 0
    assert L.mh_beam_topk(*args) == OK
    torch.cuda.synchronize()
    _all_untouched(wins, "B = 0")
    assert torch.equal(pos.cpu(), pos0 + 1) and torch.equal(kvlen.cpu(), kv0 + 1)


def test_topk_refusals_leave_every_buffer_untouched():
    c = BR.case("rand-nb3-B3-rpi3-V1023")
    _, dev = _device_logits(c, float("nan"))
    scores = c.scores.to(DEV)
    wins = _topk_buffers(9, c.B, c.K)
    pbuf, pos = _win(9, I32)
    pos.fill_(4)
    L = _lib.load()
    good = _abi_args(c, dev, scores, wins, pos=pos, kvlen=pos, n_adv=0)
    V_AT, LDL_AT, RPI_AT, NB_AT = 10, 1, 8, 9
    refused = [({V_AT: 32769, LDL_AT: 40000}, ERR_UNSUPPORTED), ({V_AT: 5}, ERR_UNSUPPORTED), ({NB_AT: 0}, ERR_UNSUPPORTED),
               ({NB_AT: 9, RPI_AT: 9}, ERR_UNSUPPORTED), ({NB_AT: 9, RPI_AT: 1}, ERR_UNSUPPORTED), ({RPI_AT: 2}, ERR_UNSUPPORTED),
               ({RPI_AT: 0}, ERR_UNSUPPORTED), ({RPI_AT: 4}, ERR_UNSUPPORTED), ({LDL_AT: c.V - 1}, ERR_ARG), ({V_AT: 0}, ERR_ARG)]
    refused += [({at: None}, ERR_ARG) for at in (0, 2, 3, 4, 5, 6)]
    for change, rc in refused:
        args = list(good)
        for at, v in change.items():
            args[at] = v
        assert L.mh_beam_topk(*args) == rc, (change, rc)
    torch.cuda.synchronize()
    _all_untouched(wins, "refusal")
    assert_frame_untouched(pbuf, slice(0, 1), slice(PAD, PAD + 9), "refusal pos")
    assert pos.tolist() == [4] * 9
    assert L.mh_beam_topk(*good) == OK                                   # the unchanged arguments do launch
    torch.cuda.synchronize()
    assert torch.equal(wins["out_i"][1].cpu().view(c.B, c.K).long(), BR.ref(c.name).idx)


def test_beam_topk_wrapper_refuses_short_or_mistyped_buffers():
    c = BR.case("rand-nb3-B3-rpi3-V1023")
    R, K, B = 9, c.K, c.B
    _, dev = _device_logits(c, float("nan"))
    scores = c.scores.to(DEV)
    wins = _topk_buffers(R, B, K)
    pbuf, pos = _win(R, I32)
    pos.fill_(4)
    base = dict(logits=dev[:, :c.V], scores=scores, part_s=wins["part_s"][1], part_i=wins["part_i"][1], out_s=wins["out_s"][1],
                out_i=wins["out_i"][1], B=B, nb=c.nb, pos=None, kvlen=None)
    bad = [dict(logits=dev[:8, :c.V]), dict(B=2), dict(B=0),                                            # 8 % 3, 9 % 2, no items
           dict(scores=scores[:R - 1]), dict(part_s=base["part_s"][:R * K - 1]), dict(part_i=base["part_i"][:R * K - 1]),
           dict(out_s=base["out_s"][:B * K - 1]), dict(out_i=base["out_i"][:B * K - 1]),
           dict(logits=dev[:, :c.V].double()), dict(logits=dev.t()[:c.V].t()[:, ::2]), dict(scores=scores.double()),
           dict(part_s=base["part_i"]), dict(part_i=base["part_s"]), dict(out_s=base["out_i"]), dict(out_i=base["out_s"]),
           dict(out_i=torch.zeros(B * K, dtype=torch.long, device=DEV)), dict(scores=c.scores),         # int64; a host tensor
           dict(pos=pos, kvlen=pos[:R - 1]), dict(pos=pos[:R - 1], kvlen=pos), dict(pos=pos), dict(kvlen=pos),
           dict(pos=pos.long(), kvlen=pos.long()), dict(pos=pos, kvlen=pos.float())]
    for change in bad:
        kw = dict(base, **change)
        with pytest.raises(_lib.MyriadHipError):
            ops.beam_topk(kw.pop("logits"), kw.pop("scores"), kw.pop("part_s"), kw.pop("part_i"), kw.pop("out_s"), kw.pop("out_i"),
                          kw.pop("B"), kw.pop("nb"), ban_id=c.ban, **kw)
    torch.cuda.synchronize()
    _all_untouched(wins, "wrapper refusal")
    assert_frame_untouched(pbuf, slice(0, 1), slice(PAD, PAD + R), "wrapper refusal pos")
    assert pos.tolist() == [4] * R


# ---------------------------------------------------------------------------------------------------------------- reorder
CPAD = 64                     # bf16 elements (128 bytes) of poison in front of and behind every layer's cache


class _Caches:
    """L caches [R, T, C] bf16, each a slice from the middle of a poisoned allocation of its own, and their host twins."""

    def __init__(self, L, R, T, C, seed):
        g = torch.Generator().manual_seed(seed)
        self.n, self.allocs, self.views, self.host = R * T * C, [], [], []
        for _ in range(L):
            a = poisoned((self.n + 2 * CPAD,), BF16, DEV)
            h = torch.randn(R, T, C, generator=g).to(BF16)
            v = a[CPAD:CPAD + self.n].view(R, T, C)
            v.copy_(h)
            self.allocs.append(a)
            self.views.append(v)
            self.host.append(h)
        self.table = torch.tensor([v.data_ptr() for v in self.views], dtype=torch.long).to(DEV)

    def check(self, what):
        torch.cuda.synchronize()
        for l, (a, v, h) in enumerate(zip(self.allocs, self.views, self.host)):
            assert_untouched(a[:CPAD], f"{what}: the bytes before layer {l}'s cache")
            assert_untouched(a[CPAD + self.n:], f"{what}: the bytes after layer {l}'s cache")
            got = v.cpu()
            if not torch.equal(got.view(torch.int16), h.view(torch.int16)):
                bad = (got.view(torch.int16) != h.view(torch.int16)).nonzero()
                raise AssertionError(f"{what}: layer {l}: {bad.shape[0]} elements differ, first at (row, position, column) "
                                     f"{tuple(bad[0].tolist())}")


def _i32(*v):
    return torch.tensor(v, dtype=I32).to(DEV)


def _reorder(cs, B, nb, src, lo, hi, what):
    """One launch and its reference: the host twins move on by reorder_ref, the device is compared with them bit for bit."""
    L, (R, T, C) = len(cs.views), cs.views[0].shape
    ops.beam_reorder_kv(cs.table, L, B, nb, T, C, _i32(*src), _i32(lo), _i32(hi))
    cs.host = BR.reorder_ref(cs.host, src, lo, hi, B, nb)
    cs.check(what)


def _mixed_parents(B, nb, turn):
    """duplicate parents, identity rows and a reversal, rotated by `turn`"""
    return [b * nb + [0, j, nb - 1 - j][(b + j + turn) % 3] for b in range(B) for j in range(nb)]


@pytest.mark.parametrize("C", [8, 2048, 2056])       # one cell; a full column block; one live thread in the second block
@pytest.mark.parametrize("T_cap", [70, 1])
def test_reorder_kv_windows(T_cap, C):
    B, nb = 2, 4
    cs = _Caches(2, B * nb, T_cap, C, seed=T_cap * 10000 + C)
    windows = ((-3, 5), (60, T_cap + 9), (T_cap - 1, T_cap), (7, 8), (8, 8), (9, 4))
    for turn, (lo, hi) in enumerate(windows):
        before = [h.clone() for h in cs.host]
        _reorder(cs, B, nb, _mixed_parents(B, nb, turn), lo, hi, f"T_cap={T_cap} C={C} window=({lo}, {hi})")
        a, z = max(lo, 0), min(hi, T_cap)
        moved = any(not torch.equal(h, h0) for h, h0 in zip(cs.host, before))
        assert moved == (a < z)                                          # the reference itself: an empty window moves nothing
        for h, h0 in zip(cs.host, before):
            assert torch.equal(h[:, :a], h0[:, :a]) and torch.equal(h[:, max(a, z):], h0[:, max(a, z):])


def test_reorder_kv_parents():
    T, C, lo, hi = 12, 2056, 2, 11
    # a full 8-cycle in place: every row is read before any is stored
    cs = _Caches(2, 16, T, C, seed=1)
    cycle = [b * 8 + (j + 1) % 8 for b in range(2) for j in range(8)]
    first = [h.clone() for h in cs.host]
    _reorder(cs, 2, 8, cycle, lo, hi, "8-cycle")
    for h, h0 in zip(cs.host, first):
        assert all(torch.equal(h[b * 8 + j, lo:hi], h0[b * 8 + (j + 1) % 8, lo:hi]) for b in range(2) for j in range(8))
    _reorder(cs, 2, 8, [r ^ 1 for r in range(16)], lo, hi, "pair swaps")
    _reorder(cs, 2, 8, [b * 8 + 7 for b in range(2) for _ in range(8)], lo, hi, "all rows from the last row")
    for h in cs.host:
        assert all(torch.equal(h[r, lo:hi], h[r | 7, lo:hi]) for r in range(16))
    # one beam: nothing to reorder, whatever src says
    cs = _Caches(2, 3, T, C, seed=2)
    first = [h.clone() for h in cs.host]
    _reorder(cs, 3, 1, [0, 1, 2], lo, hi, "nb=1 identity")
    _reorder(cs, 3, 1, [1, 2, 0], lo, hi, "nb=1, parents in other items")
    assert all(torch.equal(h, h0) for h, h0 in zip(cs.host, first))
    # parents outside the item: negative, past the last row, a row of the item before and of the item after
    cs = _Caches(2, 12, T, C, seed=3)
    first = [h.clone() for h in cs.host]
    src = [1, 0, 5, 2,   -1, 12, 2, 9,   11, 3, 10, 1 << 30]
    _reorder(cs, 3, 4, src, lo, hi, "foreign parents")
    for h, h0 in zip(cs.host, first):
        assert torch.equal(h[4:8], h0[4:8])                              # item 1: no row has a parent of its own item
        assert all(torch.equal(h[r], h0[r]) for r in (2, 9, 11))         # rows of items 0 and 2 with a foreign parent
        assert torch.equal(h[0, lo:hi], h0[1, lo:hi]) and torch.equal(h[8, lo:hi], h0[11, lo:hi])
        assert torch.equal(h[10], h0[10]) and torch.equal(h[3, lo:hi], h0[2, lo:hi])


def test_reorder_kv_graph_replay_reads_src_lo_hi_from_the_device():
    B, nb, T, C = 2, 4, 70, 2056
    cs = _Caches(2, B * nb, T, C, seed=4)
    src_d, lo_d, hi_d = _i32(*range(B * nb)), _i32(0), _i32(0)
    launch = lambda: ops.beam_reorder_kv(cs.table, 2, B, nb, T, C, src_d, lo_d, hi_d)      # noqa: E731
    launch()                                                            # identity parents, an empty window: changes nothing
    cs.check("warm launch")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    cs.check("capture")
    for turn, (lo, hi) in enumerate(((3, 40), (-2, 9), (66, 99))):
        src = _mixed_parents(B, nb, turn)
        src_d.copy_(torch.tensor(src, dtype=I32))
        lo_d.fill_(lo)
        hi_d.fill_(hi)
        g.replay()
        cs.host = BR.reorder_ref(cs.host, src, lo, hi, B, nb)
        cs.check(f"replay {turn}")


def test_reorder_kv_refusals():
    L_, B, nb, T, C = 2, 2, 4, 6, 16
    cs = _Caches(L_, B * nb, T, C, seed=5)
    src, lo, hi = _i32(*[r ^ 1 for r in range(B * nb)]), _i32(0), _i32(T)
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    good = [cs.table.data_ptr(), L_, B, nb, T, C, src.data_ptr(), lo.data_ptr(), hi.data_ptr(), s]
    for change, rc in (({3: 9}, ERR_UNSUPPORTED), ({3: 0}, ERR_UNSUPPORTED), ({5: 12}, ERR_UNSUPPORTED), ({1: 65536, 2: 1}, ERR_UNSUPPORTED),
                       ({0: None}, ERR_ARG), ({6: None}, ERR_ARG), ({7: None}, ERR_ARG), ({8: None}, ERR_ARG), ({5: 0}, ERR_ARG),
                       ({1: 0}, OK), ({4: 0}, OK), ({2: 0}, OK)):
        args = list(good)
        for at, v in change.items():
            args[at] = v
        assert lib.mh_beam_reorder_kv(*args) == rc, (change, rc)
    cs.check("refusal")
    bad = [dict(src=src[:B * nb - 1]), dict(table=cs.table[:1]), dict(src=src.long()), dict(table=cs.table.int()),
           dict(lo=lo.float()), dict(hi=hi[:0]), dict(src=src.cpu())]
    for change in bad:
        kw = dict(dict(table=cs.table, src=src, lo=lo, hi=hi), **change)
        with pytest.raises(_lib.MyriadHipError):
            ops.beam_reorder_kv(kw["table"], L_, B, nb, T, C, kw["src"], kw["lo"], kw["hi"])
    cs.check("wrapper refusal")
    assert lib.mh_beam_reorder_kv(*good) == OK                           # the unchanged arguments do launch
    cs.host = BR.reorder_ref(cs.host, [r ^ 1 for r in range(B * nb)], 0, T, B, nb)
    cs.check("the accepted launch")
