"""The split-bf16 slab backward's C ABI without a GPU (include/bevrender_hip.h: bevr_attn_slab_x3_ws_bytes, _slab_x3_prep,
bevr_attn_slab_bwd_q_x3): the symbols are declared, bound and exported; the precision contract holds both ways (the new
entry points take BEVR_PREC_BF16X3 alone, the 16-bit slab entry points keep refusing it); every contract violation
returns its code before anything is launched (fake non-NULL pointers are never dereferenced)."""
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
NEW = ("bevr_attn_slab_x3_ws_bytes", "bevr_attn_slab_x3_prep", "bevr_attn_slab_bwd_q_x3")
X3, BF16, F16, F32 = _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16, _lib.PREC_F32


def desc(S=200, precision=X3, **over):
    d = ops.AttnGeom(n_prob=2, q_div=1, heads=2, groups=1, S=S, N=100, Wt=2 * S * 3 - 1, precision=precision).desc()
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def bwd(L, d, ptrs=None):
    a = [P] * 11 if ptrs is None else ptrs         # Q Ks Vs slab_ws table_pair dO LSE delta grad_scale dQ dtable
    return L.bevr_attn_slab_bwd_q_x3(C.byref(d), *a, None)


def prep(L, d, ptrs=None):
    a = [P] * 4 if ptrs is None else ptrs          # key_a key_b order slab_ws
    return L.bevr_attn_slab_x3_prep(C.byref(d), *a, None)


def test_symbols_are_declared_bound_and_exported(L):
    header = open(os.path.join(ROOT, "include", "bevrender_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, ret, nargs in zip(NEW, ("size_t", "int", "int"), (1, 6, 13)):
        assert name in _lib.SYMBOLS
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), header), name
        assert re.search(r"\bT %s$" % name, out, re.M), name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert L.bevr_attn_slab_x3_ws_bytes.restype is C.c_size_t
    assert L.bevr_attn_slab_x3_prep.restype is C.c_int and L.bevr_attn_slab_bwd_q_x3.restype is C.c_int
    # the operands of the 16-bit twins, in their order
    assert L.bevr_attn_slab_bwd_q_x3.argtypes == L.bevr_attn_slab_bwd_q.argtypes
    assert L.bevr_attn_slab_x3_prep.argtypes == L.bevr_attn_slab_prep.argtypes
    assert L.bevr_abi_version() == 6          # additive: no new version
    assert ops.K.SLAB_BWD_Q_X3 == NEW[2] and ops._RUN[NEW[2]] is ops._RUN[ops.K.SLAB_BWD_Q]
    assert ops.SLAB_X3_DEFAULT == "0"


def test_precision_contract_both_ways(L):
    # the new entry points: the split mode alone
    for prec in (F32, BF16, F16):
        for S in (12, 200):
            assert bwd(L, desc(S=S, precision=prec)) == E_PRECISION, (prec, S)
            assert prep(L, desc(S=S, precision=prec)) == E_PRECISION, (prec, S)
            assert L.bevr_attn_slab_x3_ws_bytes(C.byref(desc(S=S, precision=prec))) == 0, (prec, S)
    assert bwd(L, desc(), [ODD] + [P] * 10) == E_ALIGN          # accepted as far as the last check
    assert prep(L, desc(), [P, P, P, ODD]) == E_ALIGN
    # the 16-bit entry points keep refusing it, one band or row bands
    d = desc()
    assert L.bevr_attn_slab_bwd_q(C.byref(d), *([P] * 11), None) == E_PRECISION
    assert L.bevr_attn_slab_prep(C.byref(d), P, P, P, P, None) == E_PRECISION
    assert L.bevr_attn_slab_ws_bytes(C.byref(d)) == 0
    assert L.bevr_attn_slab_bwd_q_rows(C.byref(d), *([P] * 11), 0, 200, None) == E_PRECISION
    assert L.bevr_attn_slab_rows_prep(C.byref(d), P, P, P, P, None) == E_PRECISION
    assert L.bevr_attn_slab_rows_ws_bytes(C.byref(d)) == 0
    # and keep taking their own modes
    for prec in (BF16, F16):
        assert L.bevr_attn_slab_bwd_q(C.byref(desc(precision=prec)), *([ODD] + [P] * 10), None) == E_ALIGN
        assert L.bevr_attn_slab_ws_bytes(C.byref(desc(precision=prec))) > 0


def test_workspace_sizes_and_the_side_limit(L):
    assert L.bevr_attn_slab_x3_ws_bytes(C.byref(desc(S=212))) == 0
    assert bwd(L, desc(S=212)) == E_SHAPE and prep(L, desc(S=212)) == E_SHAPE
    assert bwd(L, desc(S=400)) == E_SHAPE
    for S in (211, 200, 12, 9):
        assert L.bevr_attn_slab_x3_ws_bytes(C.byref(desc(S=S))) > 0, S
        assert bwd(L, desc(S=S), [ODD] + [P] * 10) == E_ALIGN, S
    # 16 bytes per cell instead of 12: a narrower slab, more slabs, a larger workspace than the 16-bit kernel's
    assert L.bevr_attn_slab_x3_ws_bytes(C.byref(desc())) > L.bevr_attn_slab_ws_bytes(C.byref(desc(precision=BF16))) > 0


def test_null_and_misaligned_operands(L):
    d = desc()
    for i in range(11):
        a = [P] * 11
        a[i] = None
        assert bwd(L, d, a) == E_NULL, i
    for i in (0, 1, 2, 3, 4, 5, 9):          # Q, Ks, Vs, slab_ws, table_pair, dO, dQ: as bevr_attn_slab_bwd_q checks them
        a = [P] * 11
        a[i] = ODD
        assert bwd(L, d, a) == E_ALIGN, i
    # the order of bevr_attn_slab_bwd_q: NULL, precision, shape, alignment
    assert bwd(L, desc(S=212, precision=BF16), [None] + [P] * 10) == E_NULL
    assert bwd(L, desc(S=212, precision=BF16), [ODD] + [P] * 10) == E_PRECISION
    assert bwd(L, desc(S=212), [ODD] + [P] * 10) == E_SHAPE
    for i in range(4):
        a = [P] * 4
        a[i] = None
        assert prep(L, d, a) == E_NULL, i
    assert prep(L, desc(S=212, precision=BF16), [P, P, P, ODD]) == E_PRECISION
    assert prep(L, desc(S=212), [P, P, P, ODD]) == E_SHAPE
    assert L.bevr_attn_slab_bwd_q_x3(None, *([P] * 11), None) == E_NULL
    for over in (dict(Sp=16), dict(Np=101), dict(Ht=20), dict(heads=3, groups=2), dict(Hp=7)):
        assert bwd(L, desc(**over)) == E_SHAPE, over
        assert L.bevr_attn_slab_x3_ws_bytes(C.byref(desc(**over))) == 0, over
