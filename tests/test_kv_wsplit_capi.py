"""bevr_kv_project_w2 (include/bevrender_hip.h: bevr_kv_project with the weights as two E planes): its refusals, in the
order bevr_kv_project makes them -- NULL pointers, shapes (with lo_exp), the f32-layout modes, alignment.  The checks
come before any launch, so this runs without a GPU (fake non-NULL pointers are never dereferenced); every case is
held against the plain entry point called with the same arguments."""
import ctypes as C

import pytest

from bevrender_amd import _lib

E_NULL, E_SHAPE, E_PRECISION, E_ALIGN = -1, -2, -3, -4
P = C.c_void_p(0x10000)          # a 16-byte aligned, never dereferenced "device pointer"
ODD = C.c_void_p(0x10004)        # misaligned (and 4 mod 8: the positions' own contract)
ARGS = ("feat", "feat_bf16", "pos", "pos_pstride", "W", "bkv", "nb", "Hi", "Wi", "C", "N", "Np", "heads", "c", "precision",
        "Kr", "Vr", "Kt", "Vt", "vnorm2_max", "knorm2_max", "groups", "stream")
GOOD = dict(feat=P, feat_bf16=0, pos=P, pos_pstride=300, W=P, bkv=P, nb=2, Hi=12, Wi=20, C=64, N=300, Np=320, heads=2, c=32,
            precision=_lib.PREC_BF16, Kr=P, Vr=P, Kt=P, Vt=P, vnorm2_max=P, knorm2_max=P, groups=1, stream=None)


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def plain(L, **over):
    a = dict(GOOD, **over)
    return L.bevr_kv_project(*[a[k] for k in ARGS])


def w2(L, lo_exp=0, **over):
    a = dict(GOOD, **over)
    args = [a[k] for k in ARGS]
    args.insert(ARGS.index("W") + 1, lo_exp)
    return L.bevr_kv_project_w2(*args)


def test_symbol_is_bound():
    assert "bevr_kv_project_w2" in _lib.SYMBOLS and "bevr_kv_project" in _lib.SYMBOLS
    L = _lib.lib()
    assert len(L.bevr_kv_project_w2.argtypes) == len(L.bevr_kv_project.argtypes) + 1
    assert L.bevr_abi_version() == 6


NULLS = ["feat", "pos", "W", "Kr", "Vr", "Vt"]
SHAPES = [dict(nb=0), dict(Hi=1), dict(Wi=1), dict(N=0), dict(Np=256), dict(Np=330), dict(heads=0), dict(c=0),
          dict(c=33, heads=2, C=66), dict(C=48), dict(C=72, heads=3, c=24), dict(C=272, heads=17, c=16), dict(pos_pstride=299),
          dict(groups=0), dict(groups=3), dict(groups=32)]
PRECISIONS = [_lib.PREC_F32, _lib.PREC_BF16X3, 9]
ALIGNS = ["feat", "W", "Kr", "Vr", "Vt", "Kt", "pos"]


@pytest.mark.parametrize("name", NULLS)
def test_null_pointers(L, name):
    assert w2(L, **{name: None}) == plain(L, **{name: None}) == E_NULL


def test_optional_pointers_may_be_null(L):
    # bias, transposed K and both norm outputs: a misaligned operand behind them is what is reported
    over = dict(bkv=None, Kt=None, vnorm2_max=None, knorm2_max=None, feat=ODD)
    assert w2(L, **over) == plain(L, **over) == E_ALIGN


@pytest.mark.parametrize("bad", SHAPES, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in SHAPES])
def test_shapes(L, bad):
    assert w2(L, **bad) == plain(L, **bad) == E_SHAPE


@pytest.mark.parametrize("lo_exp", [-1, 25, 1 << 20, -(1 << 31)])
def test_lo_exp_out_of_range_is_a_shape_error(L, lo_exp):
    assert w2(L, lo_exp=lo_exp) == E_SHAPE


@pytest.mark.parametrize("lo_exp", [0, 11, 24])
def test_lo_exp_in_range_passes_the_shape_check(L, lo_exp):
    # ... and the next refusal in line is reported (nothing may be launched on fake pointers)
    assert w2(L, lo_exp=lo_exp, precision=_lib.PREC_F32) == E_PRECISION
    assert w2(L, lo_exp=lo_exp, feat=ODD) == E_ALIGN


@pytest.mark.parametrize("prec", PRECISIONS)
def test_f32_layout_modes_and_unknown_codes(L, prec):
    assert w2(L, precision=prec) == plain(L, precision=prec) == E_PRECISION


@pytest.mark.parametrize("name", ALIGNS)
def test_misaligned_pointers(L, name):
    for prec in (_lib.PREC_BF16, _lib.PREC_F16):
        assert w2(L, precision=prec, **{name: ODD}) == plain(L, precision=prec, **{name: ODD}) == E_ALIGN


def test_order_of_the_checks(L):
    """NULL before shape before precision before alignment, as bevr_kv_project: one call violating two rules reports the
    earlier one."""
    pairs = [
        (dict(feat=None, nb=0), E_NULL), (dict(Vt=None, precision=_lib.PREC_F32), E_NULL), (dict(W=None, Kr=ODD), E_NULL),
        (dict(nb=0, precision=_lib.PREC_F32), E_SHAPE), (dict(Np=330, feat=ODD), E_SHAPE),
        (dict(precision=_lib.PREC_F32, feat=ODD), E_PRECISION), (dict(precision=9, W=ODD), E_PRECISION),
    ]
    for over, want in pairs:
        assert w2(L, **over) == plain(L, **over) == want, over
    # lo_exp belongs to the shape check: after NULL, before precision and alignment
    assert w2(L, lo_exp=25, feat=None) == E_NULL
    assert w2(L, lo_exp=25, precision=_lib.PREC_F32) == E_SHAPE
    assert w2(L, lo_exp=25, feat=ODD) == E_SHAPE
