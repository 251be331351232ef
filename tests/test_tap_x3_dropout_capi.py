"""Attention dropout on the tap entry points in the split-bf16 mode (bevr_attn_tap_*_x3_dropout), the parts that need no
GPU: the exports and prototypes, the refusals (fake aligned pointers: the checks come before any launch), the host-side
operand builder's slot 15 against the header's words in float64, and the d(pos) kink census of the one key set that
tests/test_gpu_tap_x3_dropout.py judges with the kink rule and tests/test_tap_x3_host.py does not already cover."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from bevrender_amd import _lib, ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from test_tap_x3_host import CAP, _parts64, kink_shares  # noqa: E402
from test_gpu_tap import KERNEL_CASES  # noqa: E402  (nothing there touches the GPU on import)

X3 = _lib.PREC_BF16X3
P = C.c_void_p(0x10000)          # a 16-byte aligned, never dereferenced "device pointer"
NEW = ("bevr_attn_tap_fwd_x3_dropout", "bevr_attn_tap_bwd_q_x3_dropout", "bevr_attn_tap_bwd_k_x3_dropout")
E_NULL, E_SHAPE, E_PRECISION = -1, -2, -3

# the NB = 2 key set of the GPU test (S = 120: 8 row blocks, two per wave), drawn with host_rng=True there.  The cotangent
# lives on every tenth BEV column, as for X3_KERNEL_CASES["nb4"]: with all 120 compared columns nearly every key would be
# within 2e-3 of SOME column's kink
NB2_CASE = dict(KERNEL_CASES["two_blocks_per_wave"], h_cols=list(range(3, 120, 10)))


def _desc(**over):
    d = ops.AttnGeom(n_prob=2, q_div=1, heads=2, groups=1, S=12, N=100, Wt=71, precision=X3).desc()
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _calls(L, r, thr=100, lsum=P):
    """the three entry points on descriptor r, every pointer fake and aligned"""
    return (L.bevr_attn_tap_fwd_x3_dropout(r, P, P, P, P, P, lsum, P, 0, thr, 1, None),
            L.bevr_attn_tap_bwd_q_x3_dropout(r, P, P, P, P, P, P, 0, thr, 1, None),
            L.bevr_attn_tap_bwd_k_x3_dropout(r, P, P, P, P, P, P, P, P, 0, thr, 1, None))


def test_exports_and_prototypes():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.bevr_abi_version() == _lib.ABI_VERSION == 6
    # the binding's argument lists are the 16-bit dropout entry points' (the header declares the same parameters)
    for name in NEW:
        assert getattr(L, name).argtypes == getattr(L, name.replace("_x3", "")).argtypes, name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bevrender_hip.h")).read()

    def params(name):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        return re.sub(r"\s+", " ", m.group(1))
    for name in NEW:
        assert params(name) == params(name.replace("_x3", "")), name


@pytest.mark.parametrize("prec", [_lib.PREC_BF16, _lib.PREC_F16, _lib.PREC_F32])
def test_every_precision_but_the_split_mode_is_refused(prec):
    assert _calls(_lib.lib(), C.byref(_desc(precision=prec))) == (E_PRECISION,) * 3


def test_refusals_in_the_order_of_the_16_bit_dropout_entry_points():
    L = _lib.lib()
    r = C.byref(_desc())
    assert _calls(L, r, thr=65536) == (E_SHAPE,) * 3
    # (the threshold is looked at first: with a NULL lsum too it is still the shape error)
    assert L.bevr_attn_tap_fwd_x3_dropout(r, P, P, P, P, P, None, P, 0, 65536, 1, None) == E_SHAPE
    assert L.bevr_attn_tap_fwd_x3_dropout(r, P, P, P, P, P, None, P, 0, 100, 1, None) == E_NULL
    # lsum comes before the descriptor: a NULL lsum with a wrong-precision descriptor is the NULL error
    assert L.bevr_attn_tap_fwd_x3_dropout(C.byref(_desc(precision=_lib.PREC_BF16)), P, P, P, P, P, None, P, 0, 100, 1, None) == E_NULL
    assert _calls(L, C.byref(_desc(groups=2))) == (E_SHAPE,) * 3
    # NULL operands and a misaligned G, before the precision
    assert L.bevr_attn_tap_fwd_x3_dropout(r, None, P, P, P, P, P, P, 0, 100, 1, None) == E_NULL
    assert L.bevr_attn_tap_bwd_q_x3_dropout(r, P, None, P, P, P, P, 0, 100, 1, None) == E_NULL
    assert L.bevr_attn_tap_bwd_k_x3_dropout(r, P, P, P, P, P, P, P, None, 0, 100, 1, None) == E_NULL
    odd = C.c_void_p(0x10008)
    bf16 = C.byref(_desc(precision=_lib.PREC_BF16))
    assert L.bevr_attn_tap_fwd_x3_dropout(bf16, odd, P, P, P, P, P, P, 0, 100, 1, None) == -4
    assert L.bevr_attn_tap_bwd_q_x3_dropout(bf16, odd, P, P, P, P, P, 0, 100, 1, None) == -4
    assert L.bevr_attn_tap_bwd_k_x3_dropout(bf16, odd, P, P, P, P, P, P, P, 0, 100, 1, None) == -4


def test_the_16_bit_dropout_entry_points_keep_refusing_the_split_mode():
    L = _lib.lib()
    r = C.byref(_desc())
    assert L.bevr_attn_tap_fwd_dropout(r, P, P, P, P, P, P, P, 0, 100, 1, None) == E_PRECISION
    assert L.bevr_attn_tap_bwd_q_dropout(r, P, P, P, P, P, P, 0, 100, 1, None) == E_PRECISION
    assert L.bevr_attn_tap_bwd_k_dropout(r, P, P, P, P, P, P, P, P, 0, 100, 1, None) == E_PRECISION


def test_tap_supported_with_dropout_needs_both_switches(monkeypatch):
    for name in ("BEVR_TAP", "BEVR_TAP_X3", "BEVR_TAP_X3_DROP"):
        monkeypatch.delenv(name, raising=False)
    assert ops.TAP_X3_DROP_DEFAULT == "0"
    assert not ops.tap_supported(X3, 1, dropout=True)
    monkeypatch.setenv("BEVR_TAP_X3_DROP", "1")
    assert ops.tap_supported(X3, 1, dropout=True) == (ops.TAP_X3_DEFAULT != "0")      # the first switch still decides
    monkeypatch.setenv("BEVR_TAP_X3", "1")
    assert ops.tap_supported(X3, 1, dropout=True) and ops.tap_supported(X3, 1)
    assert not ops.tap_supported(X3, 2, dropout=True)
    monkeypatch.setenv("BEVR_TAP_X3_DROP", "0")
    assert not ops.tap_supported(X3, 1, dropout=True) and ops.tap_supported(X3, 1)
    monkeypatch.delenv("BEVR_TAP_X3_DROP")
    assert not ops.tap_supported(X3, 1, dropout=True)
    monkeypatch.setenv("BEVR_TAP_X3_DROP", "1")
    monkeypatch.setenv("BEVR_TAP_X3", "0")
    assert not ops.tap_supported(X3, 1, dropout=True)
    monkeypatch.setenv("BEVR_TAP_X3", "1")
    monkeypatch.setenv("BEVR_TAP", "0")
    assert not ops.tap_supported(X3, 1, dropout=True)
    monkeypatch.delenv("BEVR_TAP")
    # the 16-bit modes and f32 do not look at the new switch
    monkeypatch.setenv("BEVR_TAP_X3_DROP", "0")
    assert ops.tap_supported(_lib.PREC_BF16, 1, dropout=True) and ops.tap_supported(_lib.PREC_F16, 1, dropout=True)
    assert not ops.tap_supported(_lib.PREC_F32, 1, dropout=True)


@pytest.mark.parametrize("scale", [1e-6, 1.0, 37.5, 3.0e4])
def test_operand_builder_writes_slot_15_as_the_header_words_it(scale):
    """ops._tap_operand(x3=True, slot15=...) against include/bevrender_hip.h (bevr_attn_tap_*_x3_dropout), as
    tests/test_tap_x3_host.py::test_operand_builder_follows_the_header: slot 15's planes are the successive bf16 parts of
    the value, hi + lo is within 2^-16 relative; every other slot is what the builder wrote without slot15; and the
    tool's builder, written from the header alone, gives the same bits."""
    import tap_drop_check
    gen = torch.Generator().manual_seed(int(scale * 7) % 1000 + 3)
    rows = torch.randn(3, 2, 40, 12, generator=gen) * scale
    one = torch.randn(3, 2, 40, generator=gen) * scale
    c = torch.randn(3, 2, 40, generator=gen) * scale * 10 - 64.0
    planes, seen = ops._tap_operand(rows, True, slot15=one)
    assert planes.shape == (2, 3, 2, 40, 16) and planes.dtype == torch.bfloat16
    p = _parts64(one)
    assert torch.equal(planes[0][..., 15].double(), p[0]) and torch.equal(planes[1][..., 15].double(), p[1])
    got = planes[0][..., 15].double() + planes[1][..., 15].double()
    assert ((got - one.double()).abs() <= 2.0 ** -16 * one.double().abs()).all()
    plain, seen0 = ops._tap_operand(rows, True)
    assert torch.equal(planes[..., :15].view(torch.int16), plain[..., :15].view(torch.int16)) and torch.equal(seen, seen0)
    assert (plain[..., 15] == 0).all()
    ops._set_offset(planes, c, True)
    r16 = torch.zeros(3, 2, 40, 16)
    r16[..., :12] = rows
    hp, hc, hone = tap_drop_check.header_split_drop(r16, c, one)
    assert torch.equal(hp.view(torch.int16), planes.view(torch.int16))
    assert torch.equal(hone.double(), got)
    # the 16-bit pack keeps ONE value in slot 15
    op16, _ = ops._tap_operand(rows, False, torch.bfloat16, slot15=one)
    assert torch.equal(op16[..., 15], one.to(torch.bfloat16))


def test_kink_census_of_the_nb2_key_set():
    """tests/test_tap_x3_host.py::test_kink_census_of_the_gpu_tests_key_sets, with its two assertions, for the NB = 2 case
    the dropout GPU test adds to X3_KERNEL_CASES (the other key sets are covered there)."""
    import tap_check
    kw = NB2_CASE
    gen = torch.Generator().manual_seed(kw.get("seed", 0))
    a, b, ys, xs = tap_check.draw_keys(kw["P"], kw["S"], kw["N"], kw["Wt"], kw.get("spread", (5.0, 2.5)),
                                       kw.get("sort", True), gen)
    own, anyk, _ = kink_shares(a, b, ys, xs, kw["S"], kw["Wt"], kw.get("h_cols"))
    print(f"[census nb2] own-coordinate kinks {own:.4f}, any compared column {anyk:.4f}")
    assert own < CAP, own
    assert 1.0 - anyk >= 0.3, anyk


TWO_ROUTES_CFG = (1, 2, 64, 2, 34, 3, 12, 30, 1024)     # test_tap_pix_and_region_routes_evaluate_one_mask, seed 9


def test_kink_census_of_the_two_routes_key_set():
    """The same census for the keys the two-routes GPU test compares d(pos) on: ALL keys of the call, the scattered ones
    included (both routes differentiate them), over every BEV column."""
    from test_gpu_tap import _tap_problem
    B, V, Cc, h, S, D, Hi, Wi, n_pin = TWO_ROUTES_CFG
    pos = _tap_problem(*TWO_ROUTES_CFG, seed=9)[4].double()
    Wt = 2 * S * D - 1
    a = (1 - pos[..., 0]) * (S - 1) / 2
    b = (1 - pos[..., 1]) * (Wt - 1) / 4
    ys, xs = (pos[..., 0] + 1) * 0.5 * (Hi - 1), (pos[..., 1] + 1) * 0.5 * (Wi - 1)
    own, anyk, _ = kink_shares(a, b, ys, xs, S, Wt)
    print(f"[census two routes] own-coordinate kinks {own:.4f}, any compared column {anyk:.4f}")
    assert own < CAP, own
    assert 1.0 - anyk >= 0.3, anyk
