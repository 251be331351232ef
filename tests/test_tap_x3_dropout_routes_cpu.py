"""ops.attention_route and the switch BEVR_TAP_X3_DROP (attention dropout on the split-mode tap kernels,
bevr_attn_tap_*_x3_dropout), host only.  Over the grid of tests/test_slab_x3_routes_cpu.py (precisions x S x table width x
dropout) times source in {kv, kv_source, tap_pix} and tap_source in {False, True, "pinned"}:
  * unset or "0": every route, refusal and message is the one with the variable deleted;
  * BEVR_TAP_X3=1 and the new switch on: the routes differ only for BEVR_PREC_BF16X3 with dropout and a tap segment on
    tap_pix -- there the region segment keeps the region dropout kernels, the tap segment runs the three new entry points,
    and the merge is merge_views;
  * BEVR_TAP_X3=0: the new switch changes nothing;
  * tap_pix with dropout has no projected rows of the pinned keys to fall back to: where kv_source's rules would drop the
    split, it raises."""
import itertools

import pytest

from bevrender_amd import _lib, ops
from test_slab_x3_routes_cpu import N, SIDES, SWITCHES, widths

K = ops.K
X3, BF16, F16, F32 = _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16, _lib.PREC_F32
SPLIT = N // 2
REGION_DROP = (K.FWD_DROP, K.BWD_Q_DROP, K.BWD_K_DROP)
NEW = ("bevr_attn_tap_fwd_x3_dropout", "bevr_attn_tap_bwd_q_x3_dropout", "bevr_attn_tap_bwd_k_x3_dropout")
PARENT_MESSAGE = "tap_pix has no attention dropout: pass every key's projected rows and no tap segment"

GRID = list(itertools.product((F32, X3, BF16, F16), SIDES, ("narrow", "wide"), (False, True),
                              ("kv", "kv_source", "tap_pix"), (False, True, "pinned"), (None, SPLIT)))


def route(prec, S, Wt, dropout, source, tap_source, cell_split, in_grid=True):
    """the route, or the message of the ValueError the call raises"""
    try:
        return ops.attention_route(prec, 1, S, Wt, N, cell_split, tap_source, dropout, source, 64, 2,
                                   keys_in_tap_grid=lambda split: in_grid)
    except ValueError as e:
        return str(e)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in SWITCHES + ("BEVR_TAP_X3_DROP",):
        monkeypatch.delenv(name, raising=False)


def test_the_names_are_spelled_once():
    assert (K.TAP_FWD_X3_DROP, K.TAP_BWD_Q_X3_DROP, K.TAP_BWD_K_X3_DROP) == NEW
    assert ops._RUN[K.TAP_FWD_X3_DROP] is ops._tap_fwd and ops._RUN[K.TAP_BWD_Q_X3_DROP] is ops._tap_bwd_q
    assert ops._RUN[K.TAP_BWD_K_X3_DROP] is ops._tap_bwd_k
    assert all(n in _lib.SYMBOLS for n in NEW)


@pytest.mark.parametrize("tap_x3", [None, "0", "1"])
def test_switch_unset_or_zero_is_the_parents_route(monkeypatch, tap_x3):
    if tap_x3 is not None:
        monkeypatch.setenv("BEVR_TAP_X3", tap_x3)
    said = 0
    for key in GRID:
        prec, S, wname, dropout, source, tap_source, cell_split = key
        Wt = widths(S)[wname]
        base = route(prec, S, Wt, dropout, source, tap_source, cell_split)
        monkeypatch.setenv("BEVR_TAP_X3_DROP", "0")
        assert route(prec, S, Wt, dropout, source, tap_source, cell_split) == base, key
        monkeypatch.delenv("BEVR_TAP_X3_DROP")
        # the parent's rule for tap_pix with a mask, written out: always this refusal
        if dropout and source == "tap_pix":
            assert base == PARENT_MESSAGE, key
            said += 1
        if not isinstance(base, str):
            assert not any(n in (sg.fwd, sg.bwd_q, sg.bwd_k) for sg in base.segments for n in NEW), key
    assert said > 0


def test_both_switches_on_change_the_split_modes_tap_pix_route_with_dropout_alone(monkeypatch):
    monkeypatch.setenv("BEVR_TAP_X3", "1")
    changed = raised = 0
    for key in GRID:
        prec, S, wname, dropout, source, tap_source, cell_split = key
        Wt = widths(S)[wname]
        base = route(prec, S, Wt, dropout, source, tap_source, cell_split)
        monkeypatch.setenv("BEVR_TAP_X3_DROP", "1")
        new = route(prec, S, Wt, dropout, source, tap_source, cell_split)
        monkeypatch.delenv("BEVR_TAP_X3_DROP")
        if not (prec == X3 and dropout and source == "tap_pix"):
            assert new == base, key
            continue
        assert base == PARENT_MESSAGE, key
        if tap_source and cell_split is not None and S <= 448:
            segs = [(sg.kind, sg.n0, sg.n1, sg.fwd, sg.bwd_q, sg.bwd_k) for sg in new.segments]
            assert segs == [("region", 0, SPLIT) + REGION_DROP, ("tap", SPLIT, N) + NEW], key
            assert new.merge == "merge_views" and new.split == SPLIT and new.gather is None and not new.kn2, key
            assert new.tap and new.n_core == SPLIT
            changed += 1
        else:
            # no tap segment under kv_source's rules: tap_pix cannot fall back to every key's rows
            assert isinstance(new, str) and new != PARENT_MESSAGE and "tap_pix" in new, key
            raised += 1
    # every side of the grid is within the tap kernels' 448: 5 sides x 2 widths x (True, "pinned")
    assert changed == len(SIDES) * 2 * 2 and raised > 0


def test_without_the_first_switch_the_new_one_changes_nothing(monkeypatch):
    for tap_x3 in (None, "0"):
        if tap_x3 is not None:
            monkeypatch.setenv("BEVR_TAP_X3", tap_x3)
        if ops.tap_supported(X3, 1):          # (the default of BEVR_TAP_X3 was flipped: the unset case is the test above)
            continue
        for key in GRID:
            prec, S, wname, dropout, source, tap_source, cell_split = key
            Wt = widths(S)[wname]
            base = route(prec, S, Wt, dropout, source, tap_source, cell_split)
            monkeypatch.setenv("BEVR_TAP_X3_DROP", "1")
            assert route(prec, S, Wt, dropout, source, tap_source, cell_split) == base, key
            monkeypatch.delenv("BEVR_TAP_X3_DROP")


def test_tap_pix_with_dropout_raises_where_kv_source_would_drop_the_split(monkeypatch):
    monkeypatch.setenv("BEVR_TAP_X3", "1")
    monkeypatch.setenv("BEVR_TAP_X3_DROP", "1")
    Wt = widths(200)["wide"]
    # the checked contract (tap_source=True) fails: a key outside the tap grid
    with pytest.raises(ValueError, match="tap_pix"):
        ops.attention_route(X3, 1, 200, Wt, N, SPLIT, True, True, "tap_pix", 64, 2, keys_in_tap_grid=lambda split: False)
    # ... or no region segment beside it (kv_source's rule: the split is kept only with cell_split > 0)
    with pytest.raises(ValueError, match="tap_pix"):
        ops.attention_route(X3, 1, 200, Wt, N, 0, True, True, "tap_pix", 64, 2, keys_in_tap_grid=lambda split: True)
    # S beyond the tap kernels' 448
    with pytest.raises(ValueError, match="tap_pix"):
        ops.attention_route(X3, 1, 464, widths(464)["wide"], N, SPLIT, "pinned", True, "tap_pix", 64, 2)
    # the same calls on kv_source in bf16 fall back silently to every key on the region dropout kernels
    for S, ts, grid in ((200, True, False), (464, "pinned", True)):
        r = ops.attention_route(BF16, 1, S, widths(S)["wide"], N, SPLIT, ts, True, "kv_source", 64, 2,
                                keys_in_tap_grid=lambda split: grid)
        assert [(sg.kind, sg.n0, sg.n1) for sg in r.segments] == [("region", 0, N)]
    # the promise without the check is not checked: the callback is never called
    def never(split):
        raise AssertionError("tap_source='pinned' is not checked")
    r = ops.attention_route(X3, 1, 200, Wt, N, SPLIT, "pinned", True, "tap_pix", 64, 2, keys_in_tap_grid=never)
    assert r.tap and r.segments[-1].fwd == NEW[0]
    # the checked contract that holds keeps the split
    calls = []
    r = ops.attention_route(X3, 1, 200, Wt, N, SPLIT, True, True, "tap_pix", 64, 2,
                            keys_in_tap_grid=lambda split: calls.append(split) or True)
    assert r.tap and calls == [SPLIT]
    # without a mask the route is what it was: the plain split-mode tap kernels and the fused merge
    r = ops.attention_route(X3, 1, 200, Wt, N, SPLIT, "pinned", False, "tap_pix", 64, 2)
    assert (r.segments[-1].fwd, r.merge) == (K.TAP_FWD, "merge_tap")
