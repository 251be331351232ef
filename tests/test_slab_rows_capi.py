"""The row-band slab backward's C ABI without a GPU (include/bevrender_hip.h: bevr_attn_slab_rows_ws_bytes, _slab_rows_prep,
bevr_attn_slab_bwd_q_rows): the symbols are declared, bound and exported; every contract violation returns its code
before anything is launched (fake non-NULL pointers are never dereferenced); ops.slab_bands cuts every supported side
into bands the entry point accepts; the one-band entry points keep their contract."""
import ctypes as C
import os
import re
import subprocess

import pytest

from bevrender_amd import _lib, ops

E_NULL, E_SHAPE, E_PRECISION, E_ALIGN = -1, -2, -3, -4
P = C.c_void_p(0x10000)          # a 16-byte aligned, never dereferenced "device pointer"
ODD = C.c_void_p(0x10004)        # misaligned
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bevr_attn_slab_rows_ws_bytes", "bevr_attn_slab_rows_prep", "bevr_attn_slab_bwd_q_rows")
BF16, F16 = _lib.PREC_BF16, _lib.PREC_F16


def desc(S=400, precision=BF16, **over):
    d = ops.AttnGeom(n_prob=2, q_div=1, heads=2, groups=1, S=S, N=100, Wt=2 * S * 3 - 1, precision=precision).desc()
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def rows(L, d, row0, n_rows, ptrs=None):
    a = [P] * 11 if ptrs is None else ptrs         # Q Ks Vs slab_ws table_pair dO LSE delta grad_scale dQ dtable
    return L.bevr_attn_slab_bwd_q_rows(C.byref(d), *a, row0, n_rows, None)


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
    assert L.bevr_attn_slab_rows_ws_bytes.restype is C.c_size_t
    assert L.bevr_attn_slab_rows_prep.restype is C.c_int and L.bevr_attn_slab_bwd_q_rows.restype is C.c_int
    assert L.bevr_abi_version() == 6          # additive: no new version


def test_precision_and_side_contract(L):
    prep = lambda d: L.bevr_attn_slab_rows_prep(C.byref(d), P, P, P, P, None)
    for prec in (_lib.PREC_F32, _lib.PREC_BF16X3):
        assert rows(L, desc(precision=prec), 0, 217) == E_PRECISION
        assert rows(L, desc(S=12, precision=prec), 0, 12) == E_PRECISION
        assert prep(desc(precision=prec)) == E_PRECISION
    for prec in (BF16, F16):
        assert rows(L, desc(S=449, precision=prec), 0, 217) == E_SHAPE
        assert prep(desc(S=449, precision=prec)) == E_SHAPE
        assert range_passes(L, desc(S=448, precision=prec), 0, 155)
        assert range_passes(L, desc(S=2, precision=prec), 0, 2)          # small sides too: the 832-row pitch
    # a valid range, every operand in place, an unaligned workspace: the prep got as far as its last check
    assert L.bevr_attn_slab_rows_prep(C.byref(desc()), P, P, P, ODD, None) == E_ALIGN


@pytest.mark.parametrize("prec", [BF16, F16])
@pytest.mark.parametrize("S", [12, 218, 400, 448])
def test_row_range_contract(L, prec, S):
    d = desc(S=S, precision=prec)
    bad = [(0, 218), (30, 31), (-31, 31), (0, 0), (0, -5), (0, S + 1), (S, 1), (0, 1 << 30), (1 << 30, 31)]
    if S > 30:
        bad.append((0, 30))          # a band that does not end the column is whole row blocks
    for row0, n in bad:
        assert rows(L, d, row0, n) == E_SHAPE, (S, row0, n)
    # and the good ones next to them
    good = [(0, min(S, 217))] if S <= 217 else [(0, 217), (31, 186), (31 * ((S - 1) // 31), S - 31 * ((S - 1) // 31)), (S - S % 31 - 31, 31)]
    for row0, n in good:
        assert range_passes(L, d, row0, n), (S, row0, n)


def test_null_and_misaligned_operands(L):
    d = desc()
    for i in range(11):
        a = [P] * 11
        a[i] = None
        assert rows(L, d, 0, 217, a) == E_NULL, i
    for i in (0, 1, 2, 3, 4, 5, 9):          # Q, Ks, Vs, slab_ws, table_pair, dO, dQ: as bevr_attn_slab_bwd_q checks them
        a = [P] * 11
        a[i] = ODD
        assert rows(L, d, 0, 217, a) == E_ALIGN, i
    # the order of bevr_attn_slab_bwd_q: NULL, precision, shape (the side, then the range), alignment
    assert rows(L, desc(precision=_lib.PREC_F32), 0, 218, [None] + [P] * 10) == E_NULL
    assert rows(L, desc(precision=_lib.PREC_F32), 0, 218, [ODD] + [P] * 10) == E_PRECISION
    assert rows(L, d, 0, 218, [ODD] + [P] * 10) == E_SHAPE
    for i in range(4):
        a = [P] * 4
        a[i] = None
        assert L.bevr_attn_slab_rows_prep(C.byref(d), *a, None) == E_NULL, i
    for over in (dict(Sp=16), dict(Np=101), dict(Ht=20), dict(heads=3, groups=2), dict(Hp=7)):
        assert rows(L, desc(**over), 0, 217) == E_SHAPE, over


def test_workspace_sizes_and_the_one_band_contract(L):
    for prec in (BF16, F16):
        for S in (12, 400, 403, 404, 448):
            assert L.bevr_attn_slab_rows_ws_bytes(C.byref(desc(S=S, precision=prec))) > 0, (prec, S)
        assert L.bevr_attn_slab_rows_ws_bytes(C.byref(desc(S=449, precision=prec))) == 0
        # the one-band entry points are what they were
        assert L.bevr_attn_slab_ws_bytes(C.byref(desc(S=400, precision=prec))) == 0
        assert L.bevr_attn_slab_ws_bytes(C.byref(desc(S=212, precision=prec))) == 0
        assert L.bevr_attn_slab_ws_bytes(C.byref(desc(S=211, precision=prec))) > 0
        assert L.bevr_attn_slab_bwd_q(C.byref(desc(S=212, precision=prec)), *([P] * 11), None) == E_SHAPE
        assert L.bevr_attn_slab_bwd_q(C.byref(desc(S=211, precision=prec)), *([ODD] + [P] * 10), None) == E_ALIGN
        assert L.bevr_attn_slab_prep(C.byref(desc(S=212, precision=prec)), P, P, P, P, None) == E_SHAPE
    for prec in (_lib.PREC_F32, _lib.PREC_BF16X3):
        assert L.bevr_attn_slab_rows_ws_bytes(C.byref(desc(precision=prec))) == 0
    # a narrower slab means more slabs: the tall workspace of a side both kernels take is the larger one
    d = desc(S=200)
    assert L.bevr_attn_slab_rows_ws_bytes(C.byref(d)) > L.bevr_attn_slab_ws_bytes(C.byref(d)) > 0


def test_bands_cover_every_supported_side(L):
    """Every S <= 448: bands of at most 7 row blocks that start on a row block, tile [0, S) in order, as few as seven
    workers allow, each accepted by the entry point's own range check."""
    assert ops.SLAB_BAND_BLOCKS == 7
    for S in range(2, 449):
        bands = ops.slab_bands(S)
        assert len(bands) == -(-(-(-S // 31)) // 7), S
        nxt = 0
        for r0, n in bands:
            assert r0 == nxt and r0 % 31 == 0 and 1 <= n <= 217, (S, bands)
            nxt = r0 + n
        assert nxt == S
        d = desc(S=S, precision=F16 if S % 2 else BF16)
        for r0, n in bands:
            assert range_passes(L, d, r0, n), (S, r0, n)
    assert ops.slab_bands(400) == [(0, 217), (217, 183)]
    assert ops.slab_bands(448) == [(0, 155), (155, 155), (310, 138)]
    assert ops.slab_bands(217) == [(0, 217)] and ops.slab_bands(218) == [(0, 124), (124, 94)]
    assert ops.slab_bands(70, max_blocks=1) == [(0, 31), (31, 31), (62, 8)]
    assert ops.slab_bands(70, max_blocks=2) == [(0, 62), (62, 8)]
