"""ops.attention_route and the switch BEVR_SLAB_X3 (the slab query-side backward in the split-bf16 mode,
bevr_attn_slab_bwd_q_x3), host only.  Unset or "0": every route of every precision is what it was before the entry point
existed -- compared against the rule written out here (expected_bwd_q), not against the function's own output.  "1":
only the bwd_q of the region segment changes, only for BEVR_PREC_BF16X3, S <= 211, SCA-wide tables, no dropout;
BEVR_SLAB=0: never; BEVR_SLAB=2: narrow tables too.  BEVR_SLAB_ROWS does not reach the split mode."""
import dataclasses
import itertools

import pytest

from bevrender_amd import _lib, ops

K = ops.K
X3, BF16, F16, F32 = _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16, _lib.PREC_F32
SIDES = (12, 200, 211, 212, 400)
N = 4096
SWITCHES = ("BEVR_SLAB_X3", "BEVR_SLAB", "BEVR_SLAB_ROWS", "BEVR_GATHER", "BEVR_GATHER_X3", "BEVR_TAP", "BEVR_TAP_X3",
            "BEVR_KNORM", "BEVR_MERGE_TAP", "BEVR_FUSED_KV")


def widths(S):
    """TSA's table (rx = 1 column per BEV column) and an SCA-wide one (rx = 3)"""
    return {"narrow": 2 * S - 1, "wide": 2 * S * 3 - 1}


# (cell_split, tap_source, source): no split; a cell split; a tap segment (split mode: the tap pixels, with BEVR_TAP_X3=1)
def splits(prec):
    tap = dict(cell_split=N // 2, tap_source=True, source="tap_pix" if prec in (X3, F32) else "kv_source")
    return {"none": dict(), "cell": dict(cell_split=N // 2), "tap": tap}


def route(prec, S, Wt, dropout=False, **kw):
    """the route, or the message of the ValueError the call raises (a route a precision does not have)"""
    kw.setdefault("C", 64)
    kw.setdefault("heads", 2)
    try:
        return ops.attention_route(prec, 1, S, Wt, N, dropout=dropout, keys_in_tap_grid=lambda split: True, **kw)
    except ValueError as e:
        return str(e)


def expected_bwd_q(prec, S, Wt, dropout, slab="1", slab_x3="0"):
    """the region segment's bwd_q by the rules of the parent commit, plus the new switch"""
    if dropout:
        return K.BWD_Q_DROP
    wide = slab == "2" or Wt - 1 >= 4 * (S - 1)
    if slab == "0" or S > 211 or not wide:
        return K.BWD_Q
    if prec in (BF16, F16):
        return K.SLAB_BWD_Q
    if prec == X3 and slab_x3 != "0":
        return K.SLAB_BWD_Q_X3
    return K.BWD_Q


def region(r):
    return next((sg for sg in r.segments if sg.kind == "region"), None)


GRID = [(prec, S, wname, sname, dropout) for prec, S, wname, sname, dropout in
        itertools.product((F32, X3, BF16, F16), SIDES, ("narrow", "wide"), ("none", "cell", "tap"), (False, True))]


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("tap_x3", [None, "1"])
def test_switch_off_is_the_parents_route(monkeypatch, tap_x3):
    if tap_x3:
        monkeypatch.setenv("BEVR_TAP_X3", tap_x3)
    seen = set()
    for prec, S, wname, sname, dropout in GRID:
        Wt, kw = widths(S)[wname], splits(prec)[sname]
        base = route(prec, S, Wt, dropout, **kw)
        monkeypatch.setenv("BEVR_SLAB_X3", "0")
        assert route(prec, S, Wt, dropout, **kw) == base, (prec, S, wname, sname, dropout)
        monkeypatch.delenv("BEVR_SLAB_X3")
        if isinstance(base, str):
            continue
        assert all(K.SLAB_BWD_Q_X3 not in (sg.fwd, sg.bwd_q, sg.bwd_k) for sg in base.segments)
        rg = region(base)
        if rg is not None:
            assert rg.bwd_q == expected_bwd_q(prec, S, Wt, dropout), (prec, S, wname, sname, dropout, rg)
            seen.add(rg.bwd_q)
    assert seen == {K.BWD_Q, K.BWD_Q_DROP, K.SLAB_BWD_Q}


@pytest.mark.parametrize("slab", [None, "0", "1", "2"])
@pytest.mark.parametrize("tap_x3", [None, "1"])
def test_switch_on_changes_the_split_modes_region_bwd_q_alone(monkeypatch, slab, tap_x3):
    if tap_x3:
        monkeypatch.setenv("BEVR_TAP_X3", tap_x3)
    if slab is not None:
        monkeypatch.setenv("BEVR_SLAB", slab)
    changed = 0
    for prec, S, wname, sname, dropout in GRID:
        Wt, kw = widths(S)[wname], splits(prec)[sname]
        key = (prec, S, wname, sname, dropout, slab)
        base = route(prec, S, Wt, dropout, **kw)
        monkeypatch.setenv("BEVR_SLAB_X3", "1")
        new = route(prec, S, Wt, dropout, **kw)
        monkeypatch.delenv("BEVR_SLAB_X3")
        if isinstance(base, str):
            assert new == base, key
            continue
        rg = region(base)
        want = rg is not None and expected_bwd_q(prec, S, Wt, dropout, slab or "1", "1") == K.SLAB_BWD_Q_X3
        if not want:
            assert new == base, key
            continue
        # the conditions, spelled out
        assert prec == X3 and S <= 211 and not dropout and slab != "0" and (wname == "wide" or slab == "2"), key
        assert rg.bwd_q == K.BWD_Q, key
        segs = tuple(dataclasses.replace(sg, bwd_q=K.SLAB_BWD_Q_X3) if sg.kind == "region" else sg for sg in base.segments)
        assert new == dataclasses.replace(base, segments=segs), key
        changed += 1
    # 3 sides x the widths the slab takes x every split that leaves a region segment
    assert (changed > 0) == (slab != "0"), changed
    if slab == "2":
        assert changed >= 3 * 2 * 2
    elif slab != "0":
        assert changed >= 3 * 2


def test_slab_supported_and_the_row_band_switch(monkeypatch):
    Wt = widths(200)["wide"]
    assert not ops.slab_supported(X3, 200, Wt)
    monkeypatch.setenv("BEVR_SLAB_X3", "0")
    assert not ops.slab_supported(X3, 200, Wt)
    monkeypatch.setenv("BEVR_SLAB_X3", "1")
    assert ops.slab_supported(X3, 200, Wt) and ops.slab_supported(X3, 211, widths(211)["wide"]) and ops.slab_supported(X3, 12)
    assert not ops.slab_supported(X3, 212, widths(212)["wide"])
    assert not ops.slab_supported(X3, 200, widths(200)["narrow"])
    assert not ops.slab_supported(F32, 200, Wt)
    assert ops.slab_supported(BF16, 200, Wt) and ops.slab_supported(F16, 200, Wt)
    # BEVR_SLAB_ROWS does not reach the split mode: larger sides keep the query-tile kernel, smaller ones the new route
    for rows in ("1", "2"):
        monkeypatch.setenv("BEVR_SLAB_ROWS", rows)
        assert not ops.slab_rows_supported(X3, 400, widths(400)["wide"])
        assert region(route(X3, 400, widths(400)["wide"])).bwd_q == K.BWD_Q
        assert region(route(X3, 200, Wt)).bwd_q == K.SLAB_BWD_Q_X3
    monkeypatch.delenv("BEVR_SLAB_ROWS")
    monkeypatch.setenv("BEVR_SLAB", "0")
    assert not ops.slab_supported(X3, 200, Wt)
    monkeypatch.setenv("BEVR_SLAB", "2")
    assert ops.slab_supported(X3, 200, widths(200)["narrow"])
    assert region(route(X3, 200, widths(200)["narrow"])).bwd_q == K.SLAB_BWD_Q_X3
    # dropout keeps the query-tile dropout kernel
    assert region(route(X3, 200, Wt, dropout=True)).bwd_q == K.BWD_Q_DROP
