"""The row-range gather forward's C ABI without a GPU (include/bevrender_hip.h: bevr_attn_gather_fwd_rows): the symbol is
declared, bound and exported; every contract violation returns its code before anything is launched (fake non-NULL
pointers are never dereferenced); ops.gather_supported and ops.gather_bands are what the routing documents."""
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


def desc(S=400, precision=_lib.PREC_BF16, **over):
    d = ops.AttnGeom(n_prob=2, q_div=1, heads=2, groups=1, S=S, N=100, Wt=2 * S * 3 - 1, precision=precision).desc()
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def rows(L, d, row0, n_rows, ptrs=None):
    a = [P] * 9 if ptrs is None else ptrs          # Q K V key_ws table_pk mref O LSE flags
    return L.bevr_attn_gather_fwd_rows(C.byref(d), *a, row0, n_rows, None)


def test_symbol_is_declared_bound_and_exported(L):
    assert "bevr_attn_gather_fwd_rows" in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "bevrender_hip.h")).read()
    assert re.search(r"\bint\s+bevr_attn_gather_fwd_rows\s*\(", header)
    fn = L.bevr_attn_gather_fwd_rows
    assert fn.restype is C.c_int and len(fn.argtypes) == 13
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT bevr_attn_gather_fwd_rows$", out, re.M)
    assert L.bevr_abi_version() == 6          # additive: no new version


def test_precision_contract(L):
    for prec in (_lib.PREC_F32, _lib.PREC_BF16X3):
        assert rows(L, desc(precision=prec), 0, 208) == E_PRECISION
        assert rows(L, desc(S=12, precision=prec), 0, 12) == E_PRECISION
    assert rows(L, desc(precision=9), 0, 208) == E_PRECISION
    # the whole-column entry point keeps its contract: F32 is a precision error, S = 230 a shape error in both 16-bit modes
    whole = lambda d: L.bevr_attn_gather_fwd(C.byref(d), *([P] * 9), None)
    assert whole(desc(S=12, precision=_lib.PREC_F32)) == E_PRECISION
    assert whole(desc(S=12, precision=_lib.PREC_BF16X3)) == E_PRECISION
    for prec in (_lib.PREC_BF16, _lib.PREC_F16):
        assert whole(desc(S=230, precision=prec)) == E_SHAPE


@pytest.mark.parametrize("prec", [_lib.PREC_BF16, _lib.PREC_F16])
@pytest.mark.parametrize("S", [12, 200, 400, 448])
def test_row_range_contract(L, prec, S):
    d = desc(S=S, precision=prec)
    bad = [(0, 225), (8, 4), (-16, 32), (0, 0), (0, -5), (0, S + 1), (16 * ((S - 1) // 16), 17), (S, 1),
           (16, S), (0, 1 << 30), (1 << 30, 16)]
    for row0, n in bad:
        assert rows(L, d, row0, n) == E_SHAPE, (S, row0, n)


def test_bad_descriptor_null_and_misaligned_pointers(L):
    for over in (dict(Sp=16), dict(Np=101), dict(Ht=20), dict(heads=3, groups=2), dict(Hp=7)):
        assert rows(L, desc(**over), 0, 208) == E_SHAPE, over
    d = desc()
    for i in range(9):
        a = [P] * 9
        a[i] = None
        assert rows(L, d, 0, 208, a) == E_NULL, i
    for i in (0, 1, 2, 3, 6):          # Q, K, V, key_ws, O: 16-byte aligned, as bevr_attn_gather_fwd checks them
        a = [P] * 9
        a[i] = ODD
        assert rows(L, d, 0, 208, a) == E_ALIGN, i
    # the order of the existing entry point: pointers before precision and shape
    assert rows(L, desc(precision=_lib.PREC_F32), 0, 225, [None] + [P] * 8) == E_NULL
    assert rows(L, desc(precision=_lib.PREC_F32), 0, 225, [ODD] + [P] * 8) == E_ALIGN
    assert rows(L, desc(precision=_lib.PREC_F32), 0, 225) == E_PRECISION


def test_gather_supported(monkeypatch):
    monkeypatch.delenv("BEVR_GATHER", raising=False)
    F32, BF16, F16, X3 = _lib.PREC_F32, _lib.PREC_BF16, _lib.PREC_F16, _lib.PREC_BF16X3
    for prec, S in ((F16, 200), (F16, 400), (BF16, 400), (BF16, 448), (BF16, 200), (F16, 448), (BF16, 8)):
        assert ops.gather_supported(prec, S), (prec, S)
    for prec, S in ((BF16, 449), (F16, 449), (F32, 200), (X3, 200), (F32, 400)):
        assert not ops.gather_supported(prec, S), (prec, S)
    monkeypatch.setenv("BEVR_GATHER", "0")
    for prec, S in ((F16, 200), (F16, 400), (BF16, 400), (BF16, 200)):
        assert not ops.gather_supported(prec, S)


def test_bands_cover_every_supported_side(L):
    """Every S <= 448: bands of at most 224 rows that start at multiples of 16, tile [0, S) in order, and pass the entry
    point's own range check up to the (null) operands; one band (the whole-column entry point) up to 224."""
    for S in range(2, 449):
        bands = ops.gather_bands(S)
        assert len(bands) == (1 if S <= 224 else 2), S
        nxt = 0
        for r0, n in bands:
            assert r0 == nxt and r0 % 16 == 0 and 1 <= n <= 224, (S, bands)
            nxt = r0 + n
        assert nxt == S
    assert ops.gather_bands(400) == [(0, 208), (208, 192)]          # 13 + 12 row blocks: two per wave, seven waves
    assert ops.gather_bands(448) == [(0, 224), (224, 224)]
    d = desc(S=400)
    for r0, n in ops.gather_bands(400):
        assert rows(L, d, r0, n, [None] + [P] * 8) == E_NULL        # past the descriptor; the range is checked after
        assert rows(L, d, r0, n + 224) == E_SHAPE
