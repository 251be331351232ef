"""Argument contract of the correlation head's C entry points (include/bevrender_hip.h: bevr_corr_fwd, bevr_corr_bwd,
bevr_recall_rank; csrc/corr.hip).  Every check comes before any launch or memset, so the calls below use fake pointers
that are never dereferenced and run without a GPU, like tests/test_capi_errors.py.

No call here may pass every check: it would reach a launch on a fake pointer.  Where the contract says that a check does
NOT fire (a NULL inverse norm on raw rows, a misaligned pointer into the backward), the call also carries a bad shape:
the NULL checks come first, the shape check second, the forward's alignment check last, so BEVR_E_SHAPE says that the
NULL checks let the call through and, for the backward, that no alignment was looked at before the shape.  The calls that
do succeed with such arguments (return 0, right results) are in tests/test_gpu_corr_shapes.py."""
import ctypes as C

import pytest

from bevrender_amd import _lib

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4
P = C.c_void_p(0x10000)          # a 16-byte aligned, never dereferenced "device pointer"
ODD = C.c_void_p(0x10004)        # misaligned
NUL = None
BAD_SHAPES = [(0, 4, 8), (4, 0, 8), (4, 4, 0), (-1, 4, 8), (4, -3, 8), (4, 4, -8)]


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def fwd(L, cam=P, mp=P, D=P, inc=P, inm=P, n=4, m=6, E=8, normalize=1):
    return L.bevr_corr_fwd(cam, mp, D, inc, inm, n, m, E, normalize, None)


def bwd(L, cam=P, mp=P, D=P, dD=P, inc=P, inm=P, dcam=P, dmap=P, n=4, m=6, E=8, normalize=1):
    return L.bevr_corr_bwd(cam, mp, D, dD, inc, inm, dcam, dmap, n, m, E, normalize, None)


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("arg", ["cam", "mp", "D"])
def test_corr_fwd_null_operand(L, arg, normalize):
    assert fwd(L, normalize=normalize, **{arg: NUL}) == E_NULL
    # the NULL checks come before the shape check
    assert fwd(L, normalize=normalize, n=0, **{arg: NUL}) == E_NULL


@pytest.mark.parametrize("arg", ["inc", "inm"])
def test_corr_fwd_inverse_norms_are_required_only_when_normalising(L, arg):
    assert fwd(L, normalize=1, **{arg: NUL}) == E_NULL
    assert fwd(L, normalize=7, **{arg: NUL}) == E_NULL          # normalize != 0
    # raw rows: the inverse norms are not looked at; the call gets as far as the shape check
    assert fwd(L, normalize=0, n=0, **{arg: NUL}) == E_SHAPE
    assert fwd(L, normalize=0, n=0, inc=NUL, inm=NUL) == E_SHAPE


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("n,m,E", BAD_SHAPES)
def test_corr_fwd_bad_shape(L, n, m, E, normalize):
    assert fwd(L, n=n, m=m, E=E, normalize=normalize) == E_SHAPE
    # the shape check comes before the alignment check
    assert fwd(L, cam=ODD, mp=ODD, n=n, m=m, E=E, normalize=normalize) == E_SHAPE


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("n,m,E", [(4, 6, 8), (1, 1, 4), (64, 64, 1024), (65, 3, 1024), (300, 200, 4096)])
def test_corr_fwd_rows_of_whole_vectors_must_be_aligned(L, n, m, E, normalize):
    """E % 4 == 0: the rows are read as 16-byte vectors on both the one-pass and the general kernels"""
    assert E % 4 == 0
    assert fwd(L, cam=ODD, n=n, m=m, E=E, normalize=normalize) == E_ALIGN
    assert fwd(L, mp=ODD, n=n, m=m, E=E, normalize=normalize) == E_ALIGN
    assert fwd(L, cam=ODD, mp=ODD, n=n, m=m, E=E, normalize=normalize) == E_ALIGN
    for off in (1, 2, 8, 12):
        assert fwd(L, cam=C.c_void_p(0x10000 + off), n=n, m=m, E=E, normalize=normalize) == E_ALIGN


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("arg", ["cam", "mp", "dD", "dcam", "dmap"])
def test_corr_bwd_null_operand(L, arg, normalize):
    assert bwd(L, normalize=normalize, **{arg: NUL}) == E_NULL
    assert bwd(L, normalize=normalize, n=0, **{arg: NUL}) == E_NULL


@pytest.mark.parametrize("arg", ["D", "inc", "inm"])
def test_corr_bwd_forward_results_are_required_only_when_normalising(L, arg):
    assert bwd(L, normalize=1, **{arg: NUL}) == E_NULL
    assert bwd(L, normalize=7, **{arg: NUL}) == E_NULL
    assert bwd(L, normalize=0, n=0, **{arg: NUL}) == E_SHAPE
    assert bwd(L, normalize=0, n=0, D=NUL, inc=NUL, inm=NUL) == E_SHAPE


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("n,m,E", BAD_SHAPES)
def test_corr_bwd_bad_shape(L, n, m, E, normalize):
    assert bwd(L, n=n, m=m, E=E, normalize=normalize) == E_SHAPE


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("E", [8, 7])
def test_corr_bwd_has_no_alignment_error(L, E, normalize):
    """the header's "every alignment": a misaligned pointer only changes the kernels.  Whatever is misaligned, the
    answer is the one the aligned call gets: the backward never looks at alignment before its last check."""
    names = ["cam", "mp", "D", "dD", "inc", "inm", "dcam", "dmap"]
    for arg in names:
        assert bwd(L, n=0, E=E, normalize=normalize, **{arg: ODD}) == E_SHAPE, arg
    assert bwd(L, n=0, E=E, normalize=normalize, **{a: ODD for a in names}) == E_SHAPE
    # and a misaligned pointer is not mistaken for a missing one
    assert bwd(L, E=E, normalize=normalize, cam=ODD, dcam=NUL) == E_NULL


def test_recall_rank_arguments(L):
    assert L.bevr_recall_rank(NUL, P, 8, None) == E_NULL
    assert L.bevr_recall_rank(P, NUL, 8, None) == E_NULL
    assert L.bevr_recall_rank(NUL, NUL, 0, None) == E_NULL
    for n in (0, -1, -(2 ** 31)):
        assert L.bevr_recall_rank(P, P, n, None) == E_SHAPE
        assert L.bevr_recall_rank(ODD, ODD, n, None) == E_SHAPE     # plain float / int32 arrays: no alignment contract


def test_error_codes_have_messages(L):
    for code in (E_NULL, E_SHAPE, E_ALIGN):
        assert L.bevr_strerror(code)
