"""The split-bf16 row-band slab backward's C ABI without a GPU (include/bevrender_hip.h: bevr_attn_slab_x3_rows_ws_bytes,
_slab_x3_rows_prep, bevr_attn_slab_bwd_q_x3_rows): the symbols are declared, bound and exported; every contract violation
returns its code before anything is launched (fake non-NULL pointers are never dereferenced), in the order NULL,
precision, shape (the side, then the band), alignment; every band ops.slab_bands cuts is accepted; the older slab entry
points keep their contracts."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from bevrender_amd import _lib, ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import capi_error_table as gen  # noqa: E402

E_NULL, E_SHAPE, E_PRECISION, E_ALIGN = -1, -2, -3, -4
P = C.c_void_p(0x10000)          # a 16-byte aligned, never dereferenced "device pointer"
ODD = C.c_void_p(0x10004)        # misaligned
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bevr_attn_slab_x3_rows_ws_bytes", "bevr_attn_slab_x3_rows_prep", "bevr_attn_slab_bwd_q_x3_rows")
F32, X3, BF16, F16 = _lib.PREC_F32, _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16
OTHERS = (F32, BF16, F16)


def desc(S=400, precision=X3, **over):
    d = ops.AttnGeom(n_prob=2, q_div=1, heads=2, groups=1, S=S, N=100, Wt=2 * S * 3 - 1, precision=precision).desc()
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def rows(L, d, row0, n_rows, ptrs=None):
    a = [P] * 11 if ptrs is None else ptrs         # Q Ks Vs slab_ws table_pair dO LSE delta grad_scale dQ dtable
    return L.bevr_attn_slab_bwd_q_x3_rows(C.byref(d), *a, row0, n_rows, None)


def range_passes(L, d, row0, n_rows):
    """a misaligned Q is reported after the shape: E_ALIGN says the row range was accepted"""
    return rows(L, d, row0, n_rows, [ODD] + [P] * 10) == E_ALIGN


def test_symbols_are_declared_bound_and_exported(L):
    header = open(os.path.join(ROOT, "include", "bevrender_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, ret, nargs in zip(NEW, ("size_t", "int", "int"), (1, 6, 15)):
        assert name in _lib.SYMBOLS
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), header), name
        assert re.search(r"\bT %s$" % name, out, re.M), name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert L.bevr_attn_slab_x3_rows_ws_bytes.restype is C.c_size_t
    assert L.bevr_attn_slab_x3_rows_prep.restype is C.c_int and L.bevr_attn_slab_bwd_q_x3_rows.restype is C.c_int
    assert L.bevr_attn_slab_bwd_q_x3_rows.argtypes == L.bevr_attn_slab_bwd_q_rows.argtypes
    assert L.bevr_attn_slab_x3_rows_prep.argtypes == L.bevr_attn_slab_rows_prep.argtypes
    assert L.bevr_abi_version() == 6          # additive: no new version


def test_precision_and_side_contract(L):
    prep = lambda d: L.bevr_attn_slab_x3_rows_prep(C.byref(d), P, P, P, P, None)          # noqa: E731
    for prec in OTHERS:
        assert rows(L, desc(precision=prec), 0, 217) == E_PRECISION
        assert rows(L, desc(S=12, precision=prec), 0, 12) == E_PRECISION
        assert rows(L, desc(S=449, precision=prec), 0, 218) == E_PRECISION          # the precision before the shape
        assert prep(desc(precision=prec)) == E_PRECISION
    assert rows(L, desc(S=449), 0, 217) == E_SHAPE
    assert prep(desc(S=449)) == E_SHAPE
    assert range_passes(L, desc(S=448), 0, 155)
    assert range_passes(L, desc(S=2), 0, 2)          # small sides too: the 832-row pitch
    # a valid side, every operand in place, an unaligned workspace: the prep got as far as its last check
    assert L.bevr_attn_slab_x3_rows_prep(C.byref(desc()), P, P, P, ODD, None) == E_ALIGN


@pytest.mark.parametrize("S", [12, 218, 400, 448])
def test_row_range_contract(L, S):
    d = desc(S=S)
    bad = [(0, 218), (30, 31), (-31, 31), (0, 0), (0, -5), (0, S + 1), (S, 1), (0, 1 << 30), (1 << 30, 31)]
    if S > 30:
        bad.append((0, 30))          # a band that does not end the column is whole row blocks
    for row0, n in bad:
        assert rows(L, d, row0, n) == E_SHAPE, (S, row0, n)
    good = [(0, min(S, 217))] if S <= 217 else [(0, 217), (31, 186), (31 * ((S - 1) // 31), S - 31 * ((S - 1) // 31)), (S - S % 31 - 31, 31)]
    for row0, n in good:
        assert range_passes(L, d, row0, n), (S, row0, n)


def test_null_and_misaligned_operands_in_the_contracts_order(L):
    d = desc()
    for i in range(11):
        a = [P] * 11
        a[i] = None
        assert rows(L, d, 0, 217, a) == E_NULL, i
    for i in (0, 1, 2, 3, 4, 5, 9):          # Q, Ks, Vs, slab_ws, table_pair, dO, dQ: as bevr_attn_slab_bwd_q checks them
        a = [P] * 11
        a[i] = ODD
        assert rows(L, d, 0, 217, a) == E_ALIGN, i
    # NULL, precision, shape (the side, then the band), alignment
    assert rows(L, desc(precision=BF16), 0, 218, [None] + [P] * 10) == E_NULL
    assert rows(L, desc(precision=BF16), 0, 218, [ODD] + [P] * 10) == E_PRECISION
    assert rows(L, desc(S=449), 0, 217, [ODD] + [P] * 10) == E_SHAPE
    assert rows(L, d, 0, 218, [ODD] + [P] * 10) == E_SHAPE
    assert rows(L, d, 0, 217, [ODD] + [P] * 10) == E_ALIGN
    for i in range(4):
        a = [P] * 4
        a[i] = None
        assert L.bevr_attn_slab_x3_rows_prep(C.byref(d), *a, None) == E_NULL, i
    for over in (dict(Sp=16), dict(Np=101), dict(Ht=20), dict(heads=3, groups=2), dict(Hp=7)):
        assert rows(L, desc(**over), 0, 217) == E_SHAPE, over


def test_workspace_sizes(L):
    ws = lambda **k: L.bevr_attn_slab_x3_rows_ws_bytes(C.byref(desc(**k)))          # noqa: E731
    for S in (12, 211, 212, 400, 403, 404, 448):
        assert ws(S=S) > 0, S
    assert ws(S=449) == 0
    for prec in OTHERS:
        for S in (12, 400, 449):
            assert ws(S=S, precision=prec) == 0, (prec, S)
    # a narrower slab means more slabs: 7 owned columns against the one-band kernel's 15, 6 on the taller pitch
    d = desc(S=200)
    assert ws(S=200) > L.bevr_attn_slab_x3_ws_bytes(C.byref(d)) > 0
    d16 = desc(S=400, precision=BF16)
    assert ws(S=400) > L.bevr_attn_slab_rows_ws_bytes(C.byref(d16)) > 0          # 7 columns against the 16-bit unit's 12


def test_every_band_of_every_side_is_accepted(L):
    """S = 1 .. 448.  (S = 1 is no side of any attention descriptor: bevr_attn_table_dims and with it every entry point
    answer BEVR_E_SHAPE to S < 2 -- the table's column step divides by S - 1, tests/test_capi_symbols.py pins it -- so its
    one band is checked on the host side and the entry point's answer is the descriptor's.)"""
    assert ops.slab_bands(1) == [(0, 1)] and rows(L, desc(S=1), 0, 1, [ODD] + [P] * 10) == E_SHAPE
    for S in range(2, 449):
        bands = ops.slab_bands(S)
        assert sum(n for _, n in bands) == S and bands[0][0] == 0
        d = desc(S=S)
        for r0, n in bands:
            assert range_passes(L, d, r0, n), (S, r0, n)
    for blocks in (1, 2):          # the bands the GPU tests force
        for S in (33, 40, 63, 70):
            for r0, n in ops.slab_bands(S, blocks):
                assert range_passes(L, desc(S=S), r0, n), (S, blocks, r0, n)


# ---- the new entry points' error codes as a table: one defect and every pair of defects of different classes, the cases
# of tools/capi_error_table.py, held against tests/golden/slab_x3_rows_error_codes.json (the recorded tables of the earlier
# entry points stay what they are) ----
with open(gen.later_table("slab_x3_rows")) as _f:
    GOLDEN = json.load(_f)
no_device = pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="the accepted cases go on to a launch with made-up pointers: harmless with no device (the first runtime call "
           "fails), not something to do on a GPU that others share")


def test_the_tables_cover_every_entry_point_once(L):
    mine = gen.entry_points(L, "slab_x3_rows")
    assert GOLDEN["abi"] == _lib.ABI_VERSION
    assert sorted(GOLDEN["entry_points"]) == sorted(mine) == sorted(n for n in NEW if not n.endswith("_ws_bytes"))
    with open(gen.TABLE) as f:
        recorded = set(json.load(f)["entry_points"])
    assert not recorded & set(mine) and sorted(recorded) == sorted(gen.entry_points(L))
    for group in gen.LATER:
        if group != "slab_x3_rows":
            with open(gen.later_table(group)) as f:
                assert not set(json.load(f)["entry_points"]) & set(mine), group


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
    assert got == want["codes"]


def test_the_older_slab_entry_points_keep_their_contracts(L):
    eleven = [P] * 11
    # the 16-bit band kernel answers the split mode with BEVR_E_PRECISION, and its workspace with 0
    assert L.bevr_attn_slab_bwd_q_rows(C.byref(desc()), *eleven, 0, 217, None) == E_PRECISION
    assert L.bevr_attn_slab_rows_prep(C.byref(desc()), P, P, P, P, None) == E_PRECISION
    assert L.bevr_attn_slab_rows_ws_bytes(C.byref(desc())) == 0
    # the one-band split kernel ends at S = 211
    assert L.bevr_attn_slab_bwd_q_x3(C.byref(desc(S=212)), *eleven, None) == E_SHAPE
    assert L.bevr_attn_slab_bwd_q_x3(C.byref(desc(S=211)), *([ODD] + [P] * 10), None) == E_ALIGN
    assert L.bevr_attn_slab_x3_prep(C.byref(desc(S=212)), P, P, P, P, None) == E_SHAPE
    assert L.bevr_attn_slab_x3_ws_bytes(C.byref(desc(S=212))) == 0 and L.bevr_attn_slab_x3_ws_bytes(C.byref(desc(S=211))) > 0
    assert L.bevr_attn_slab_x3_drop_ws_bytes(C.byref(desc(S=212))) == 0
    assert L.bevr_attn_slab_bwd_q_x3_dropout(C.byref(desc(S=212)), *eleven, 6554, 1, None) == E_SHAPE
    for prec in (BF16, F16):
        assert L.bevr_attn_slab_bwd_q_x3(C.byref(desc(S=40, precision=prec)), *eleven, None) == E_PRECISION
        assert L.bevr_attn_slab_bwd_q(C.byref(desc(S=212, precision=prec)), *eleven, None) == E_SHAPE
        assert L.bevr_attn_slab_bwd_q_rows(C.byref(desc(precision=prec)), *([ODD] + [P] * 10), 0, 217, None) == E_ALIGN
    assert L.bevr_attn_slab_bwd_q(C.byref(desc(S=40)), *eleven, None) == E_PRECISION
