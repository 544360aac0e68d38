"""The host side of serving several conversations on the decode slots -- no device anywhere: myriad_amd.llama.SessionTable (which
conversation lives in which slot, what its cache holds, what invalidates it), TurnPlanner (which turns share a prefill pass), and
the condition the GPU suite's fp64 test of mh_attn_prefill_ragged_past puts on its inputs."""
import pytest

from myriad_amd.llama import SessionTable, TurnPlanner
from tests import fp64_bounds as fb
from tests.ragged_past_case import H, ONE_ROW_SEGS, SEGS, T_CAP, one_row_inputs, past_inputs


def T(*ids):
    return [("t", i) for i in ids]


STAMP = (1, ("P", "bf16"), None)


def test_rope_exempt_share_of_the_past_kernel_case():
    """Every segment of at least 16 rows leaves at most 1 % of the rotated elements ambiguous and no whole row (measured: 0.34 %
    at worst); a shorter segment is too few elements for a share (at D = 16 the (63, 2) segment has 1 ambiguous element of 64),
    so only "no whole row" is asked of it."""
    assert max(p + n for p, n in SEGS) == T_CAP == max(p + n for p, n in ONE_ROW_SEGS)
    for D, inputs in [(D, f) for D in (16, 128) for f in (past_inputs, one_row_inputs)]:
        qkv, _, seg, _, pos = inputs(D, "cpu")
        cos, sin = fb.rope_tables(D)
        W = H * D
        for r0, n, _, past in seg:
            for i in (0, 1):
                x = qkv[r0:r0 + n, i * W:(i + 1) * W].float().reshape(1, n, H, D).transpose(1, 2)
                unc = fb.rope_bf16(x, pos[r0:r0 + n].long()[None], cos, sin)[1]
                what = f"D={D} past={past} len={n} {'qk'[i]}"
                if n >= 16:
                    fb.assert_rope_exempt_share(unc, what)
                else:
                    assert not bool((unc > 0).all(-1).any()), f"{what}: a whole row is ambiguous"


def test_a_session_is_pinned_to_one_slot_until_closed():
    tab = SessionTable(3)
    assert [tab.begin(s, T(1, 2))[0] for s in ("a", "b", "c")] == [0, 1, 2]
    assert tab.begin("b", T(1, 2, 3))[0] == 1 and tab.slot_of("c") == 2 and len(tab) == 3
    with pytest.raises(ValueError, match="close"):
        tab.begin("d", T(1))
    with pytest.raises(ValueError, match="close"):
        tab.plan([("d", T(1))], STAMP)
    tab.close("b")
    assert "b" not in tab and tab.begin("d", T(1)) == (1, 0, "empty cache")      # the freed slot, nothing cached
    tab.close("nobody")                                              # closing what is not open is nothing
    # an unhashable session (the chat's Conversation dataclass is one) is known by identity
    u, v = [1], [1]
    tab.close("a")
    assert tab.begin(u, T(1))[0] == 0 and u in tab and v not in tab


def test_past_for_extended_edited_rolled_back_and_unchanged_contexts():
    tab = SessionTable(2)
    ctx = T(1, 5, 6, 7)
    assert tab.begin("a", ctx) == (0, 0, "empty cache")
    tab.end("a", ctx, [20, 21, 22])                                  # cached: the context, 20 and 21; the last pick has no KV
    assert tab.keys_of("a") == ctx + T(20, 21)
    ext = ctx + T(20, 21, 22, 9, 9)
    assert tab.begin("a", ext) == (0, 6, None)                       # extended: everything cached is reused
    assert tab.keys_of("a") == []                                    # until end(): the slot is being written
    tab.end("a", ext, [30])
    assert tab.keys_of("a") == ext                                   # a turn that ended on its first pick fed nothing
    assert tab.begin("a", ext) == (0, len(ext) - 1, None)            # unchanged: one row is still prefilled
    tab.end("a", ext, [30, 31])
    edited = ext[:3] + T(99) + ext[4:]
    assert tab.begin("a", edited) == (0, 3, None)                    # edited at row 3
    tab.end("a", edited, [40, 41, 42])
    assert tab.begin("a", edited[:5]) == (0, 4, None)                # rolled back: shorter than the cache, len - 1
    tab.end("a", edited[:5], [50, 51])
    assert tab.begin("a", T(2)) == (0, 0, None)                      # nothing in common: past 0, yet the cache was usable
    # image rows are keys like any other; a reset reason drops the session's rows
    tab.end("a", T(2) + [("i", "dig", 0), ("i", "dig", 1)], [7])
    assert tab.begin("a", T(2) + [("i", "dig", 0), ("i", "other", 1)])[1] == 2
    tab.end("a", T(2, 3, 4), [7])
    assert tab.begin("a", T(2, 3, 4, 5), "window") == (0, 0, "window")
    with pytest.raises(ValueError):
        tab.begin("a", [])


def test_every_stamp_change_drops_all_keys_with_its_reason():
    tab = SessionTable(3)
    ctx = T(1, 2, 3)

    def fill():
        for s in ("a", "b"):
            tab.begin(s, ctx)
            tab.end(s, ctx, [8, 9])

    assert tab.plan([("a", ctx), ("b", ctx)], STAMP) == [(0, 0, "empty cache"), (1, 0, "empty cache")]
    fill()
    assert tab.plan([("a", ctx + T(8, 9))], STAMP) == [(0, 4, None)]              # the same stamp: reuse
    fill()
    moved = (2,) + STAMP[1:]                                         # the caller's weights_version
    assert tab.plan([("b", ctx)], moved) == [(1, 0, "weights changed")]
    tab.end("b", ctx, [8, 9])
    assert tab.plan([("a", ctx), ("c", ctx)], moved) == [(0, 0, "weights changed"), (2, 0, "empty cache")]   # a's were dropped too
    fill()
    kind = (2, ("P", "fp8"), None)                                   # the decode weights' id
    assert tab.plan([("a", ctx), ("b", ctx)], kind) == [(0, 0, "decode weights changed"), (1, 0, "decode weights changed")]
    fill()
    merge = (2, ("P", "fp8"), 7)                                     # the merge id of a merged qkv copy
    assert tab.plan([("a", ctx)], merge) == [(0, 0, "decode weights changed")]
    fill()
    tab.clear()                                                      # SlotDecoder.run overwrote the caches
    assert tab.plan([("a", ctx), ("b", ctx)], merge) == [(0, 0, "empty cache"), (1, 0, "empty cache")]
    assert tab.slot_of("a") == 0 and tab.slot_of("b") == 1           # the sessions stayed pinned through all of it


def test_one_turn_per_session_per_call():
    tab = SessionTable(3)
    with pytest.raises(ValueError, match="one turn per session"):
        tab.plan([("a", T(1)), ("b", T(1)), ("a", T(1, 2))], STAMP)
    assert len(tab) == 0                                             # refused before anything was opened
    conv = [0]                                                       # by identity too
    with pytest.raises(ValueError, match="one turn per session"):
        tab.plan([(conv, T(1)), (conv, T(1))], STAMP)


def test_turns_share_passes_in_list_order_within_the_caps():
    items = [(2, ("x", 40)), (0, ("y", 30)), (1, ("z", 100)), (3, ("w", 10))]
    plan = TurnPlanner(items, prefill_batch=4, prefill_rows=128, length=lambda q: q[1])
    assert plan.next_pass() == items[:2] and plan.next_pass() == items[2:] and plan.next_pass() == []
    assert (plan.passes, plan.packed_rows) == (2, 180)
    solo = TurnPlanner(items, prefill_batch=1, length=lambda q: q[1])
    assert [solo.next_pass() for _ in range(5)] == [[i] for i in items] + [[]]
    long_first = TurnPlanner([(0, ("x", 300)), (1, ("y", 10))], prefill_batch=4, prefill_rows=128, length=lambda q: q[1])
    assert long_first.next_pass() == [(0, ("x", 300))]               # longer than the cap: a pass of its own
    with pytest.raises(ValueError):
        TurnPlanner([], prefill_batch=0)
