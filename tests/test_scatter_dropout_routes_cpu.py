"""BEVR_SCATTER_DROP, without a GPU: what ops.attention_route decides for a call with a keep mask -- unset, every row of
the table is the one it was (the region dropout kernels, no gather forward); set, the region segment of the 16-bit modes
takes the gather forward and the slab bwd_q with the mask where gather_supported / slab_supported hold -- as literals
over precision, grid side, table width, BEVR_GATHER / BEVR_SLAB and a tap segment; the library's new symbols; and the new entry points' error codes, case by case and as a table."""
import ctypes
import hashlib
import json
import os
import sys

import pytest
import torch

from bevrender_amd import _lib, ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import capi_error_table as gen  # noqa: E402

F32, X3, BF16, F16 = _lib.PREC_F32, _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16
PRECS = (F32, X3, BF16, F16)
SIDES = (40, 200, 211, 212, 400)        # the slab route ends at 211; the gather forward runs as bands at 400
SWITCHES = ("BEVR_GATHER", "BEVR_SLAB", "BEVR_SLAB_ROWS", "BEVR_KNORM", "BEVR_MERGE_TAP", "BEVR_TAP", "BEVR_TAP_X3",
            "BEVR_TAP_X3_DROP", "BEVR_GATHER_X3", "BEVR_SLAB_X3", "BEVR_SCATTER_DROP")
FWD_DROP, BWD_Q_DROP, BWD_K_DROP = "bevr_attn_fwd_dropout", "bevr_attn_bwd_q_dropout", "bevr_attn_bwd_k_dropout"
GATHER_DROP, SLAB_DROP = "bevr_attn_gather_fwd_dropout", "bevr_attn_slab_bwd_q_dropout"
TAP_DROP = ("bevr_attn_tap_fwd_dropout", "bevr_attn_tap_bwd_q_dropout", "bevr_attn_tap_bwd_k_dropout")
NEW_SYMBOLS = (GATHER_DROP, "bevr_attn_slab_drop_ws_bytes", "bevr_attn_slab_drop_prep", SLAB_DROP)
NK, SPLIT = 4096, 1024


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def tsa(S):
    return 2 * S - 1


def sca(S):     # depth 4
    return 2 * S * 4 - 1


def route(prec, S, Wt, tap):
    """a call with a keep mask; tap: the keys [SPLIT, NK) pinned, beside a fused K | V source (16-bit modes)"""
    if tap:
        return ops.attention_route(prec, 1, S, Wt, NK, SPLIT, "pinned", True, "kv_source", 64, 2)
    return ops.attention_route(prec, 1, S, Wt, NK, None, False, True, "kv", 64, 2)


def region_of(r):
    assert r.segments[0].kind == "region" and r.segments[0].n0 == 0
    return r.segments[0]


def test_names_are_spelled_once():
    assert ops.K.GATHER_DROP == GATHER_DROP and ops.K.SLAB_BWD_Q_DROP == SLAB_DROP
    assert ops.SCATTER_DROP_DEFAULT == "0"
    assert ops._RUN[GATHER_DROP] is ops._fwd_gather_drop and ops._RUN[SLAB_DROP] is ops._bwd_q_slab_drop


@pytest.mark.parametrize("value", [None, "0"])
@pytest.mark.parametrize("tap", [False, True])
@pytest.mark.parametrize("wide", [True, False])
@pytest.mark.parametrize("S", SIDES)
@pytest.mark.parametrize("prec", PRECS)
def test_switch_unset_keeps_every_dropout_row(monkeypatch, prec, S, wide, tap, value):
    if value is not None:
        monkeypatch.setenv("BEVR_SCATTER_DROP", value)
    if tap and prec in (F32, X3):
        tap = False      # no fused source / no mask on that mode's tap kernels by default: the split is dropped anyway
    for slab in (None, "0", "2"):
        if slab is None:
            monkeypatch.delenv("BEVR_SLAB", raising=False)
        else:
            monkeypatch.setenv("BEVR_SLAB", slab)
        r = route(prec, S, sca(S) if wide else tsa(S), tap)
        sg = region_of(r)
        assert (sg.fwd, sg.bwd_q, sg.bwd_k) == (FWD_DROP, BWD_Q_DROP, BWD_K_DROP)
        assert r.gather is None and r.kn2 is False
        assert sg.n1 == (SPLIT if tap else NK)
        if tap:
            assert (r.segments[1].fwd, r.segments[1].bwd_q, r.segments[1].bwd_k) == TAP_DROP


def expected(prec, S, wide, gather_sw, slab_sw):
    """the rows of the issue, from the limits themselves (224-row window, 211-row slab column, SCA-wide tables)"""
    sixteen = prec in (BF16, F16)
    gather = None
    if sixteen and gather_sw != "0" and S <= 448:
        gather = "whole" if S <= 224 else "bands"
    slab = sixteen and slab_sw != "0" and S <= 211 and (wide or slab_sw == "2")
    return (GATHER_DROP if gather else FWD_DROP, SLAB_DROP if slab else BWD_Q_DROP, BWD_K_DROP), gather


@pytest.mark.parametrize("tap", [False, True])
@pytest.mark.parametrize("slab_sw", [None, "0", "2"])
@pytest.mark.parametrize("gather_sw", [None, "0"])
@pytest.mark.parametrize("wide", [True, False])
@pytest.mark.parametrize("S", SIDES)
@pytest.mark.parametrize("prec", PRECS)
def test_switch_set_routes_the_region_segment(monkeypatch, prec, S, wide, gather_sw, slab_sw, tap):
    monkeypatch.setenv("BEVR_SCATTER_DROP", "1")
    if gather_sw is not None:
        monkeypatch.setenv("BEVR_GATHER", gather_sw)
    if slab_sw is not None:
        monkeypatch.setenv("BEVR_SLAB", slab_sw)
    if tap and prec in (F32, X3):
        tap = False
    r = route(prec, S, sca(S) if wide else tsa(S), tap)
    sg = region_of(r)
    want, gather = expected(prec, S, wide, gather_sw, slab_sw)
    assert (sg.fwd, sg.bwd_q, sg.bwd_k) == want
    assert r.gather == gather
    assert r.kn2 is (tap and gather is not None)          # the fused source hands the gather forward its K norm bound
    assert r.merge == "merge_views"                         # (the fused merge assumes a kept mass of 1)
    assert sg.n1 == (SPLIT if tap else NK)
    if tap:
        assert (r.segments[1].kind, r.segments[1].n0, r.segments[1].n1) == ("tap", SPLIT, NK)
        assert (r.segments[1].fwd, r.segments[1].bwd_q, r.segments[1].bwd_k) == TAP_DROP
    else:
        assert len(r.segments) == 1


def test_literal_rows(monkeypatch):
    """a few rows spelled out, independent of `expected`"""
    monkeypatch.setenv("BEVR_SCATTER_DROP", "1")
    sg = region_of(route(BF16, 200, sca(200), True))
    assert (sg.fwd, sg.bwd_q, sg.bwd_k) == (GATHER_DROP, SLAB_DROP, BWD_K_DROP)
    sg = region_of(route(F16, 212, sca(212), False))
    assert (sg.fwd, sg.bwd_q) == (GATHER_DROP, BWD_Q_DROP)
    r = route(BF16, 400, sca(400), False)
    assert r.gather == "bands" and region_of(r).bwd_q == BWD_Q_DROP
    sg = region_of(route(BF16, 200, tsa(200), False))          # TSA-wide: the slab route declines ...
    assert (sg.fwd, sg.bwd_q) == (GATHER_DROP, BWD_Q_DROP)
    monkeypatch.setenv("BEVR_SLAB", "2")                        # ... unless forced
    assert region_of(route(BF16, 200, tsa(200), False)).bwd_q == SLAB_DROP
    monkeypatch.setenv("BEVR_SLAB_ROWS", "2")                   # the row-band slab has no mask
    assert region_of(route(BF16, 400, sca(400), False)).bwd_q == BWD_Q_DROP
    for prec in (F32, X3):
        sg = region_of(route(prec, 200, sca(200), False))
        assert (sg.fwd, sg.bwd_q, sg.bwd_k) == (FWD_DROP, BWD_Q_DROP, BWD_K_DROP)


def test_without_a_mask_the_switch_changes_nothing(monkeypatch):
    rows = [(p, S, w) for p in PRECS for S in SIDES for w in (True, False)]
    before = [ops.attention_route(p, 1, S, sca(S) if w else tsa(S), NK) for p, S, w in rows]
    monkeypatch.setenv("BEVR_SCATTER_DROP", "1")
    after = [ops.attention_route(p, 1, S, sca(S) if w else tsa(S), NK) for p, S, w in rows]
    assert before == after


def test_library_exports_the_new_symbols():
    """header, binding and library agree on the four new entry points (tests/test_capi_symbols.py checks the prototypes)"""
    assert set(NEW_SYMBOLS) <= set(_lib.SYMBOLS)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} has not been built")
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    bound = _lib.lib()
    assert len(bound.bevr_attn_gather_fwd_dropout.argtypes) == 15
    assert len(bound.bevr_attn_slab_bwd_q_dropout.argtypes) == 15
    assert ctypes.sizeof(bound.bevr_attn_slab_drop_ws_bytes.restype) == ctypes.sizeof(ctypes.c_size_t)


# ---- the contracts of the new entry points: every violation returns its code before anything is launched ----
E_NULL, E_SHAPE, E_PRECISION, E_ALIGN = -1, -2, -3, -4
P = ctypes.c_void_p(0x10000)          # a 16-byte aligned, never dereferenced "device pointer"
ODD = ctypes.c_void_p(0x10004)
THR = int(round(0.3 * 65536))


def desc(S=200, precision=BF16, **over):
    d = ops.AttnGeom(n_prob=2, q_div=1, heads=2, groups=1, S=S, N=100, Wt=2 * S * 3 - 1, precision=precision).desc()
    for k, v in over.items():
        setattr(d, k, v)
    return d


def gather_drop(d, row0, n_rows, thr=THR, ptrs=None):
    a = [P] * 9 if ptrs is None else ptrs          # Q K V key_ws table_pk mref O LSE flags
    return _lib.lib().bevr_attn_gather_fwd_dropout(ctypes.byref(d), *a, row0, n_rows, thr, 7, None)


def slab_drop(d, thr=THR, ptrs=None):
    a = [P] * 11 if ptrs is None else ptrs         # Q Ks Vs slab_ws table_pair dO LSE delta grad_scale dQ dtable
    return _lib.lib().bevr_attn_slab_bwd_q_dropout(ctypes.byref(d), *a, thr, 7, None)


def test_gather_dropout_contract():
    for prec in (BF16, F16):
        d = desc(precision=prec)
        assert gather_drop(d, 0, 200, thr=65536) == E_SHAPE                    # p = 1
        for row0, n in [(0, 225), (8, 4), (-16, 32), (0, 0), (0, 201), (192, 9), (200, 1)]:
            assert gather_drop(d, row0, n) == E_SHAPE, (row0, n)
        for i in range(9):
            a = [P] * 9
            a[i] = None
            assert gather_drop(d, 0, 200, ptrs=a) == E_NULL, i
        assert gather_drop(d, 0, 200, ptrs=[ODD] + [P] * 8) == E_ALIGN
        for S in (21, 200, 232, 400, 448):        # every band ops launches passes the range check
            for r0, n in ops.gather_bands(S):
                assert gather_drop(desc(S=S, precision=prec), r0, n, ptrs=[None] + [P] * 8) == E_NULL
    for prec in (F32, X3, 9):
        assert gather_drop(desc(precision=prec), 0, 200) == E_PRECISION, prec
    assert gather_drop(desc(Sp=16), 0, 200) == E_SHAPE


def test_slab_dropout_contract():
    L = _lib.lib()
    for prec in (BF16, F16):
        d = desc(precision=prec)
        assert slab_drop(d, thr=65536) == E_SHAPE
        for i in range(11):
            a = [P] * 11
            a[i] = None
            assert slab_drop(d, ptrs=a) == E_NULL, i
        assert slab_drop(d, ptrs=[ODD] + [P] * 10) == E_ALIGN
        assert slab_drop(desc(S=212, precision=prec)) == E_SHAPE               # the one-band kernel ends at 211
        # the workspace of its own prep: the size and the checks of bevr_attn_slab_ws_bytes / _slab_prep
        assert L.bevr_attn_slab_drop_ws_bytes(ctypes.byref(d)) == L.bevr_attn_slab_ws_bytes(ctypes.byref(d)) > 0
        assert L.bevr_attn_slab_drop_ws_bytes(ctypes.byref(desc(S=212, precision=prec))) == 0
        assert L.bevr_attn_slab_drop_prep(ctypes.byref(d), None, P, P, P, None) == E_NULL
        assert L.bevr_attn_slab_drop_prep(ctypes.byref(d), P, P, P, ODD, None) == E_ALIGN
        assert L.bevr_attn_slab_drop_prep(ctypes.byref(desc(S=212, precision=prec)), P, P, P, P, None) == E_SHAPE
    for prec in (F32, X3):
        assert slab_drop(desc(precision=prec)) == E_PRECISION, prec
        assert L.bevr_attn_slab_drop_prep(ctypes.byref(desc(precision=prec)), P, P, P, P, None) == E_PRECISION
        assert L.bevr_attn_slab_drop_ws_bytes(ctypes.byref(desc(precision=prec))) == 0


# ---- the new entry points' error codes as a table: one defect and every pair of defects of different classes, the cases
# of tools/capi_error_table.py, held against tests/golden/scatter_dropout_error_codes.json (the recorded table of the
# earlier entry points, tests/golden/capi_error_codes.json, stays what it is) ----
with open(gen.later_table("scatter_dropout")) as _f:
    GOLDEN = json.load(_f)
no_device = pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="the accepted cases go on to a launch with made-up pointers: harmless with no device (the first runtime call "
           "fails), not something to do on a GPU that others share")


def test_the_two_tables_cover_every_entry_point_once():
    L = _lib.lib()
    mine = gen.entry_points(L, "scatter_dropout")
    assert GOLDEN["abi"] == _lib.ABI_VERSION
    assert sorted(GOLDEN["entry_points"]) == sorted(mine) == sorted(n for n in NEW_SYMBOLS if not n.endswith("_ws_bytes"))
    with open(gen.TABLE) as f:
        recorded = json.load(f)["entry_points"]
    assert sorted(recorded) == sorted(gen.entry_points(L)) and not set(recorded) & set(mine)


@no_device
@pytest.mark.parametrize("name", sorted(GOLDEN["entry_points"]))
def test_codes_and_their_order(name):
    want = GOLDEN["entry_points"][name]
    cs = gen.cases(_lib.lib(), name)
    assert len(cs) == want["cases"] == len(want["codes"])
    assert hashlib.sha256("\n".join(n for n, _ in cs).encode()).hexdigest() == want["names_sha256"]
    got = "".join(call() for _, call in cs)
    wrong = [(n, w, g) for (n, _), w, g in zip(cs, want["codes"], got) if w != g]
    assert not wrong, f"{len(wrong)} of {len(cs)} cases differ (case, recorded, now): {wrong[:8]}"
