"""The split-bf16 slab bwd_q with a keep mask, without a GPU: what ops.attention_route decides for a call with a mask
under BEVR_SLAB_X3 and BEVR_SCATTER_DROP -- the new name exactly where both are on, the mode is bf16x3, S <= 211,
BEVR_SLAB != 0 and the table is SCA-wide (or BEVR_SLAB=2), every other cell what it is with both unset -- as literals over
precision, grid side, table width and the three switches, and with a tap segment; the library's three new symbols; the
new entry points' error codes, case by case and as a table."""
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
SIDES = (40, 200, 211, 212, 400)        # the one-band slab column ends at 211
SWITCHES = ("BEVR_GATHER", "BEVR_SLAB", "BEVR_SLAB_ROWS", "BEVR_KNORM", "BEVR_MERGE_TAP", "BEVR_TAP", "BEVR_TAP_X3",
            "BEVR_TAP_X3_DROP", "BEVR_GATHER_X3", "BEVR_SLAB_X3", "BEVR_SCATTER_DROP", "BEVR_KV_WSPLIT")
FWD_DROP, BWD_Q_DROP, BWD_K_DROP = "bevr_attn_fwd_dropout", "bevr_attn_bwd_q_dropout", "bevr_attn_bwd_k_dropout"
SLAB_X3_DROP = "bevr_attn_slab_bwd_q_x3_dropout"
TAP_X3_DROP = ("bevr_attn_tap_fwd_x3_dropout", "bevr_attn_tap_bwd_q_x3_dropout", "bevr_attn_tap_bwd_k_x3_dropout")
NEW_SYMBOLS = ("bevr_attn_slab_x3_drop_ws_bytes", "bevr_attn_slab_x3_drop_prep", SLAB_X3_DROP)
NK, SPLIT = 4096, 1024


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def tsa(S):
    return 2 * S - 1


def sca(S):     # depth 4
    return 2 * S * 4 - 1


def masked(prec, S, Wt):
    """a call with a keep mask on projected rows: one region segment"""
    return ops.attention_route(prec, 1, S, Wt, NK, None, False, True, "kv", 64, 2)


def setenv(monkeypatch, **values):
    for k, v in values.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def test_names_are_spelled_once():
    assert ops.K.SLAB_BWD_Q_X3_DROP == SLAB_X3_DROP
    assert ops._RUN[SLAB_X3_DROP] is ops._bwd_q_slab_drop
    assert ops.SLAB_X3_DEFAULT == ops.SCATTER_DROP_DEFAULT == "0"


@pytest.mark.parametrize("scatter", [None, "0", "1"])
@pytest.mark.parametrize("x3", [None, "0", "1"])
@pytest.mark.parametrize("slab", [None, "0", "2"])
@pytest.mark.parametrize("wide", [True, False])
@pytest.mark.parametrize("S", SIDES)
@pytest.mark.parametrize("prec", PRECS)
def test_the_route_with_a_mask(monkeypatch, prec, S, wide, slab, x3, scatter):
    Wt = sca(S) if wide else tsa(S)
    setenv(monkeypatch, BEVR_SLAB=slab)
    base = masked(prec, S, Wt)                               # both switches unset
    assert len(base.segments) == 1
    assert (base.segments[0].fwd, base.segments[0].bwd_q, base.segments[0].bwd_k) == (FWD_DROP, BWD_Q_DROP, BWD_K_DROP)
    setenv(monkeypatch, BEVR_SCATTER_DROP=scatter)
    scatter_alone = masked(prec, S, Wt)                      # what BEVR_SCATTER_DROP alone gives the row
    setenv(monkeypatch, BEVR_SLAB_X3=x3)
    r = masked(prec, S, Wt)
    new = prec == X3 and S <= 211 and x3 == "1" and scatter == "1" and slab != "0" and (wide or slab == "2")
    if new:
        sg = r.segments[0]
        assert len(r.segments) == 1 and (sg.kind, sg.n0, sg.n1) == ("region", 0, NK)
        assert (sg.fwd, sg.bwd_q, sg.bwd_k) == (FWD_DROP, SLAB_X3_DROP, BWD_K_DROP)
        assert r.gather is None and r.kn2 is False and r.merge == "merge_views" and r.split == NK and r.wsplit is False
    elif prec in (BF16, F16):
        assert r == scatter_alone                            # BEVR_SLAB_X3 is nothing to the 16-bit rows
    else:
        assert r == base
    assert (r.segments[0].bwd_q == SLAB_X3_DROP) is new


def test_literal_rows(monkeypatch):
    """a few rows spelled out"""
    setenv(monkeypatch, BEVR_SLAB_X3="1", BEVR_SCATTER_DROP="1")
    assert masked(X3, 200, sca(200)).segments[0].bwd_q == SLAB_X3_DROP
    assert masked(X3, 211, sca(211)).segments[0].bwd_q == SLAB_X3_DROP
    assert masked(X3, 212, sca(212)).segments[0].bwd_q == BWD_Q_DROP
    assert masked(X3, 200, tsa(200)).segments[0].bwd_q == BWD_Q_DROP           # TSA-wide: the slab route declines ...
    assert masked(F32, 200, sca(200)).segments[0].bwd_q == BWD_Q_DROP
    assert masked(BF16, 200, sca(200)).segments[0].bwd_q == "bevr_attn_slab_bwd_q_dropout"
    setenv(monkeypatch, BEVR_SLAB="2")                                          # ... unless forced
    assert masked(X3, 200, tsa(200)).segments[0].bwd_q == SLAB_X3_DROP
    setenv(monkeypatch, BEVR_SLAB="0")
    assert masked(X3, 200, sca(200)).segments[0].bwd_q == BWD_Q_DROP
    setenv(monkeypatch, BEVR_SLAB=None, BEVR_SLAB_X3=None)                      # one switch is not enough
    assert masked(X3, 200, sca(200)).segments[0].bwd_q == BWD_Q_DROP
    setenv(monkeypatch, BEVR_SLAB_X3="1", BEVR_SCATTER_DROP=None)
    assert masked(X3, 200, sca(200)).segments[0].bwd_q == BWD_Q_DROP


@pytest.mark.parametrize("S", [40, 200, 211])
def test_with_a_tap_segment(monkeypatch, S):
    setenv(monkeypatch, BEVR_TAP_X3="1", BEVR_TAP_X3_DROP="1", BEVR_SLAB_X3="1", BEVR_SCATTER_DROP="1")
    r = ops.attention_route(X3, 1, S, sca(S), NK, SPLIT, "pinned", True, "tap_pix", 64, 2)
    assert [(s.kind, s.n0, s.n1) for s in r.segments] == [("region", 0, SPLIT), ("tap", SPLIT, NK)]
    assert (r.segments[0].fwd, r.segments[0].bwd_q, r.segments[0].bwd_k) == (FWD_DROP, SLAB_X3_DROP, BWD_K_DROP)
    assert (r.segments[1].fwd, r.segments[1].bwd_q, r.segments[1].bwd_k) == TAP_X3_DROP
    assert r.merge == "merge_views" and r.gather is None and r.kn2 is False and r.split == SPLIT
    setenv(monkeypatch, BEVR_SCATTER_DROP=None)             # the parent's route: the one difference
    p = ops.attention_route(X3, 1, S, sca(S), NK, SPLIT, "pinned", True, "tap_pix", 64, 2)
    assert p.segments[0].bwd_q == BWD_Q_DROP and p.segments[1] == r.segments[1]
    assert (p.split, p.gather, p.kn2, p.merge, p.wsplit) == (r.split, r.gather, r.kn2, r.merge, r.wsplit)


def test_without_a_mask_the_two_switches_give_what_slab_x3_alone_gives(monkeypatch):
    rows = [(p, S, w) for p in PRECS for S in SIDES for w in (True, False)]
    setenv(monkeypatch, BEVR_SLAB_X3="1")
    before = [ops.attention_route(p, 1, S, sca(S) if w else tsa(S), NK) for p, S, w in rows]
    setenv(monkeypatch, BEVR_SCATTER_DROP="1")
    after = [ops.attention_route(p, 1, S, sca(S) if w else tsa(S), NK) for p, S, w in rows]
    assert before == after
    assert any(r.segments[0].bwd_q == "bevr_attn_slab_bwd_q_x3" for r in after)


def test_the_split_gather_switch_leaves_the_masked_forward(monkeypatch):
    setenv(monkeypatch, BEVR_GATHER_X3="1", BEVR_SLAB_X3="1", BEVR_SCATTER_DROP="1")
    for S in SIDES:
        r = masked(X3, S, sca(S))
        assert r.segments[0].fwd == FWD_DROP and r.gather is None
        assert r.segments[0].bwd_q == (SLAB_X3_DROP if S <= 211 else BWD_Q_DROP)


def test_the_row_band_switch_keeps_the_query_tile_kernel(monkeypatch):
    setenv(monkeypatch, BEVR_SLAB_ROWS="2", BEVR_SLAB_X3="1", BEVR_SCATTER_DROP="1")
    assert masked(X3, 400, sca(400)).segments[0].bwd_q == BWD_Q_DROP
    assert masked(BF16, 400, sca(400)).segments[0].bwd_q == BWD_Q_DROP


def test_library_exports_the_new_symbols():
    assert set(NEW_SYMBOLS) <= set(_lib.SYMBOLS)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} has not been built")
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    bound = _lib.lib()
    assert len(bound.bevr_attn_slab_bwd_q_x3_dropout.argtypes) == 15
    assert len(bound.bevr_attn_slab_x3_drop_prep.argtypes) == 6
    assert ctypes.sizeof(bound.bevr_attn_slab_x3_drop_ws_bytes.restype) == ctypes.sizeof(ctypes.c_size_t)


# ---- the contract of the new entry points: every violation returns its code before anything is launched ----
E_NULL, E_SHAPE, E_PRECISION, E_ALIGN = -1, -2, -3, -4
P = ctypes.c_void_p(0x10000)          # a 16-byte aligned, never dereferenced "device pointer"
ODD = ctypes.c_void_p(0x10004)
THR = int(round(0.3 * 65536))


def desc(S=200, precision=X3, **over):
    d = ops.AttnGeom(n_prob=2, q_div=1, heads=2, groups=1, S=S, N=100, Wt=2 * S * 3 - 1, precision=precision).desc()
    for k, v in over.items():
        setattr(d, k, v)
    return d


def slab_x3_drop(d, thr=THR, ptrs=None):
    a = [P] * 11 if ptrs is None else ptrs         # Q Ks Vs slab_ws table_pair dO LSE delta grad_scale dQ dtable
    return _lib.lib().bevr_attn_slab_bwd_q_x3_dropout(ctypes.byref(d), *a, thr, 7, None)


def test_workspace_is_the_unmasked_kernels():
    L = _lib.lib()
    for S in (40, 200, 211):
        d = desc(S=S)
        assert L.bevr_attn_slab_x3_drop_ws_bytes(ctypes.byref(d)) == L.bevr_attn_slab_x3_ws_bytes(ctypes.byref(d)) > 0
    assert L.bevr_attn_slab_x3_drop_ws_bytes(ctypes.byref(desc(S=212))) == 0
    for prec in (F32, BF16, F16):
        assert L.bevr_attn_slab_x3_drop_ws_bytes(ctypes.byref(desc(precision=prec))) == 0
    assert L.bevr_attn_slab_x3_drop_ws_bytes(None) == 0


def test_slab_x3_dropout_contract():
    L = _lib.lib()
    d = desc()
    assert slab_x3_drop(d, thr=65536) == E_SHAPE                               # p = 1
    assert slab_x3_drop(d, thr=1 << 20) == E_SHAPE
    assert _lib.lib().bevr_attn_slab_bwd_q_x3_dropout(None, *([P] * 11), THR, 7, None) == E_NULL
    for i in range(11):
        a = [P] * 11
        a[i] = None
        assert slab_x3_drop(d, ptrs=a) == E_NULL, i
    assert slab_x3_drop(d, ptrs=[ODD] + [P] * 10) == E_ALIGN                  # a misaligned Q
    assert slab_x3_drop(desc(S=212)) == E_SHAPE                                # the one-band kernel ends at 211
    assert slab_x3_drop(desc(Sp=16)) == E_SHAPE
    # the order: nulls before the precision before the shape before the alignment
    assert slab_x3_drop(desc(precision=BF16), ptrs=[None] + [P] * 10) == E_NULL
    assert slab_x3_drop(desc(S=212, precision=BF16)) == E_PRECISION
    assert slab_x3_drop(desc(S=212), ptrs=[ODD] + [P] * 10) == E_SHAPE
    for prec in (F32, BF16, F16, 9):
        assert slab_x3_drop(desc(precision=prec)) == E_PRECISION, prec
        assert L.bevr_attn_slab_x3_drop_prep(ctypes.byref(desc(precision=prec)), P, P, P, P, None) == E_PRECISION, prec
    # the prep: the checks of bevr_attn_slab_x3_prep
    for i in range(4):
        a = [P] * 4
        a[i] = None
        assert L.bevr_attn_slab_x3_drop_prep(ctypes.byref(d), *a, None) == E_NULL, i
    assert L.bevr_attn_slab_x3_drop_prep(ctypes.byref(d), P, P, P, ODD, None) == E_ALIGN
    assert L.bevr_attn_slab_x3_drop_prep(ctypes.byref(desc(S=212)), P, P, P, P, None) == E_SHAPE
    assert L.bevr_attn_slab_x3_drop_prep(None, P, P, P, P, None) == E_NULL


# ---- the new entry points' error codes as a table: one defect and every pair of defects of different classes, the cases
# of tools/capi_error_table.py, held against tests/golden/slab_x3_dropout_error_codes.json (the recorded tables of the
# earlier entry points stay what they are) ----
with open(gen.later_table("slab_x3_dropout")) as _f:
    GOLDEN = json.load(_f)
no_device = pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="the accepted cases go on to a launch with made-up pointers: harmless with no device (the first runtime call "
           "fails), not something to do on a GPU that others share")


def test_the_tables_cover_every_entry_point_once():
    L = _lib.lib()
    mine = gen.entry_points(L, "slab_x3_dropout")
    assert GOLDEN["abi"] == _lib.ABI_VERSION
    assert sorted(GOLDEN["entry_points"]) == sorted(mine) == sorted(n for n in NEW_SYMBOLS if not n.endswith("_ws_bytes"))
    with open(gen.TABLE) as f:
        recorded = set(json.load(f)["entry_points"])
    with open(gen.later_table("scatter_dropout")) as f:
        scatter = set(json.load(f)["entry_points"])
    assert not recorded & set(mine) and not scatter & set(mine)
    assert sorted(recorded) == sorted(gen.entry_points(L))


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
