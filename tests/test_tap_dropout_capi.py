"""The tap dropout entry points (include/bevrender_hip.h: bevr_attn_tap_*_dropout) are bound, exported, and check their
arguments before anything is launched (no GPU needed)."""
import ctypes

from bevrender_amd import _lib

NAMES = ("bevr_attn_tap_fwd_dropout", "bevr_attn_tap_bwd_q_dropout", "bevr_attn_tap_bwd_k_dropout")
E_NULL, E_SHAPE = -1, -2


def _desc():
    L = _lib.lib()
    d = _lib.AttnDesc()
    d.S, d.Wt = 24, 143
    assert L.bevr_attn_table_dims(ctypes.byref(d)) == 0
    d.n_prob, d.q_div, d.heads, d.groups, d.N, d.Np, d.precision = 2, 1, 2, 1, 500, 512, _lib.PREC_BF16
    return L, d


def test_the_three_names_are_bound_and_exported():
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.SYMBOLS
        assert hasattr(L, n)


def test_a_threshold_of_65536_is_rejected_before_any_launch():
    """drop_thr = round(p * 65536) < 65536, as for the region dropout entry points: BEVR_E_SHAPE.  The pointers are
    never dereferenced (16 is no address): the check comes first."""
    L, d = _desc()
    one = ctypes.c_void_p(16)
    dp = ctypes.byref(d)
    assert L.bevr_attn_tap_fwd_dropout(dp, one, one, one, one, one, one, one, 0, 65536, 1, None) == E_SHAPE
    assert L.bevr_attn_tap_bwd_q_dropout(dp, one, one, one, one, one, one, 0, 65536, 1, None) == E_SHAPE
    assert L.bevr_attn_tap_bwd_k_dropout(dp, one, one, one, one, one, one, one, one, 0, 65536, 1, None) == E_SHAPE


def test_null_pointers_are_rejected_before_any_launch():
    L, d = _desc()
    one = ctypes.c_void_p(16)
    dp = ctypes.byref(d)
    thr = 65536 // 4
    assert L.bevr_attn_tap_fwd_dropout(dp, None, None, None, None, None, None, None, 0, thr, 1, None) == E_NULL
    # every operand but lsum given: the new output is checked as the others are
    assert L.bevr_attn_tap_fwd_dropout(dp, one, one, one, one, one, None, one, 0, thr, 1, None) == E_NULL
    assert L.bevr_attn_tap_bwd_q_dropout(dp, None, None, None, None, None, None, 0, thr, 1, None) == E_NULL
    assert L.bevr_attn_tap_bwd_k_dropout(dp, None, None, None, None, None, None, None, None, 0, thr, 1, None) == E_NULL
    assert L.bevr_attn_tap_fwd_dropout(None, one, one, one, one, one, one, one, 0, thr, 1, None) == E_NULL
