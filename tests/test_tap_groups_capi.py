"""The tap entry points for two channel groups (include/bevrender_hip.h: bevr_attn_tap_g2_*) are bound, exported, and
check their arguments before anything is launched (no GPU needed); their error codes as a table
(tools/capi_error_table.py, group "tap_groups")."""
import ctypes
import hashlib
import json
import os
import sys

import pytest
import torch

from bevrender_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import capi_error_table as gen  # noqa: E402

NAMES = ("bevr_attn_tap_g2_ws_bytes", "bevr_attn_tap_g2_prep", "bevr_attn_tap_g2_fwd", "bevr_attn_tap_g2_bwd_q",
         "bevr_attn_tap_g2_bwd_k")
E_NULL, E_SHAPE, E_PRECISION, E_ALIGN = -1, -2, -3, -4
ONE, ODD = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004)      # never dereferenced: every check comes before a launch


def _desc(heads=2, groups=2, precision=_lib.PREC_BF16):
    L = _lib.lib()
    d = _lib.AttnDesc()
    d.S, d.Wt = 24, 143
    assert L.bevr_attn_table_dims(ctypes.byref(d)) == 0
    d.n_prob, d.q_div, d.heads, d.groups, d.N, d.Np, d.precision = 2, 1, heads, groups, 500, 512, precision
    return L, d


def _calls(L, d, p=ONE, ws=ONE):
    """the four launching entry points with every pointer `p` and the workspace `ws`"""
    dp = ctypes.byref(d)
    return {"prep": L.bevr_attn_tap_g2_prep(dp, p, p, p, p, ws, None),
            "fwd": L.bevr_attn_tap_g2_fwd(dp, p, ws, p, p, p, p, None),
            "bwd_q": L.bevr_attn_tap_g2_bwd_q(dp, p, p, ws, p, p, p, None),
            "bwd_k": L.bevr_attn_tap_g2_bwd_k(dp, p, p, ws, p, p, p, p, p, None)}


def test_the_five_names_are_bound_and_exported_and_the_abi_version_stays():
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.SYMBOLS and hasattr(L, n)
    assert L.bevr_abi_version() == 6 == _lib.ABI_VERSION


def test_the_workspace_holds_records_boxes_and_the_second_position_per_group_row():
    L, d = _desc()
    rows = d.n_prob * 2
    assert L.bevr_attn_tap_g2_ws_bytes(ctypes.byref(d)) == rows * (d.Np * 16 + (d.Np // 32) * 16 + d.Np * 8)
    d.Np = 500                                  # not a multiple of 64: no descriptor
    assert L.bevr_attn_tap_g2_ws_bytes(ctypes.byref(d)) == 0
    assert L.bevr_attn_tap_g2_ws_bytes(None) == 0


def test_one_group_more_than_two_and_odd_heads_are_shape_errors():
    for heads, groups in ((2, 1), (4, 4), (4, 1)):
        L, d = _desc(heads, groups)
        assert set(_calls(L, d).values()) == {E_SHAPE}, (heads, groups)
    # (an odd number of heads with two groups is no descriptor at all: heads % groups)
    L, d = _desc(3, 2)
    assert set(_calls(L, d).values()) == {E_SHAPE}
    L, d = _desc(2, 2)
    d.heads, d.groups = 3, 3
    assert set(_calls(L, d).values()) == {E_SHAPE}


def test_the_one_group_entry_points_keep_refusing_two_groups():
    L, d = _desc()
    dp = ctypes.byref(d)
    assert L.bevr_attn_tap_prep(dp, ONE, ONE, ONE, ONE, ONE, None) == E_SHAPE
    assert L.bevr_attn_tap_fwd(dp, ONE, ONE, ONE, ONE, ONE, ONE, None) == E_SHAPE
    assert L.bevr_attn_tap_bwd_q(dp, ONE, ONE, ONE, ONE, ONE, ONE, None) == E_SHAPE
    assert L.bevr_attn_tap_bwd_k(dp, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, None) == E_SHAPE


def test_f32_and_split_bf16_are_precision_errors():
    """(every call here is a rejected one: an accepted call would go on to a launch with made-up pointers.  The
    preparation does not look at the precision -- the table below has that case, where no device is present)"""
    for prec in (_lib.PREC_F32, _lib.PREC_BF16X3, 9):
        L, d = _desc(precision=prec)
        dp = ctypes.byref(d)
        assert L.bevr_attn_tap_g2_fwd(dp, ONE, ONE, ONE, ONE, ONE, ONE, None) == E_PRECISION
        assert L.bevr_attn_tap_g2_bwd_q(dp, ONE, ONE, ONE, ONE, ONE, ONE, None) == E_PRECISION
        assert L.bevr_attn_tap_g2_bwd_k(dp, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, None) == E_PRECISION


def test_null_then_shape_then_alignment_then_precision():
    L, d = _desc()
    dp = ctypes.byref(d)
    assert set(_calls(L, d, p=None, ws=None).values()) == {E_NULL}
    assert L.bevr_attn_tap_g2_prep(None, ONE, ONE, ONE, ONE, ONE, None) == E_NULL
    assert L.bevr_attn_tap_g2_fwd(dp, ONE, ONE, ONE, ONE, ONE, None, None) == E_NULL          # flags
    assert L.bevr_attn_tap_g2_bwd_k(dp, ONE, ONE, ONE, ONE, ONE, ONE, ONE, None, None) == E_NULL   # dkey_x
    assert set(_calls(L, d, ws=ODD).values()) == {E_ALIGN}
    # null beats shape, shape beats alignment, alignment beats precision: the order of the one-group entry points
    L, d1 = _desc(2, 1)
    assert set(_calls(L, d1, p=None, ws=None).values()) == {E_NULL}
    assert set(_calls(L, d1, ws=ODD).values()) == {E_SHAPE}
    L, d3 = _desc(precision=_lib.PREC_F32)
    r = _calls(L, d3, ws=ODD)
    assert r["fwd"] == r["bwd_q"] == r["bwd_k"] == E_ALIGN


# ---- the error codes as a table: tools/capi_error_table.py's cases on a base descriptor with groups == 2, held against
# tests/golden/tap_groups_error_codes.json (the recorded table of the earlier entry points stays what it is) ----
with open(gen.later_table("tap_groups")) as _f:
    GOLDEN = json.load(_f)
no_device = pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="the accepted cases go on to a launch with made-up pointers: harmless with no device (the first runtime call "
           "fails), not something to do on a GPU that others share")


def test_the_table_of_the_group_covers_its_entry_points_and_no_other():
    L = _lib.lib()
    mine = gen.entry_points(L, "tap_groups")
    assert GOLDEN["abi"] == _lib.ABI_VERSION
    assert sorted(GOLDEN["entry_points"]) == sorted(mine) == sorted(n for n in NAMES if not n.endswith("_ws_bytes"))
    with open(gen.TABLE) as f:
        recorded = json.load(f)["entry_points"]
    assert sorted(recorded) == sorted(gen.entry_points(L)) and not set(recorded) & set(mine)
    assert gen.base_of("bevr_attn_tap_g2_fwd")["groups"] == 2 and gen.base_of("bevr_attn_tap_fwd")["groups"] == 1


@no_device
@pytest.mark.parametrize("name", sorted(GOLDEN["entry_points"]))
def test_codes_and_their_order(name):
    want = GOLDEN["entry_points"][name]
    cs = gen.cases(_lib.lib(), name)
    assert len(cs) == want["cases"] == len(want["codes"])
    assert hashlib.sha256("\n".join(n for n, _ in cs).encode()).hexdigest() == want["names_sha256"]
    got = "".join(call() for _, call in cs)
    bad = [(cs[i][0], got[i], want["codes"][i]) for i in range(len(cs)) if got[i] != want["codes"][i]]
    assert not bad, bad[:10]
