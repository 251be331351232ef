"""The split-bf16 gather forward without a GPU (include/bevrender_hip.h: bevr_attn_gather_fwd_x3): the symbol is declared,
bound and exported; every contract violation returns its code before anything is launched (fake non-NULL pointers are
never dereferenced); the switch BEVR_GATHER_X3 routes the region segment's forward and nothing else, and unset it leaves
every route what it was; ops.gather_split_table is the table operand the header words."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from bevrender_amd import _lib, ops

E_NULL, E_SHAPE, E_PRECISION, E_ALIGN = -1, -2, -3, -4
P = C.c_void_p(0x10000)          # a 16-byte aligned, never dereferenced "device pointer"
ODD = C.c_void_p(0x10004)        # misaligned
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16, X3 = _lib.PREC_F32, _lib.PREC_BF16, _lib.PREC_F16, _lib.PREC_BF16X3
NAME = "bevr_attn_gather_fwd_x3"
SWITCHES = ("BEVR_GATHER", "BEVR_GATHER_X3", "BEVR_SLAB", "BEVR_SLAB_ROWS", "BEVR_KNORM", "BEVR_MERGE_TAP", "BEVR_TAP",
            "BEVR_TAP_X3", "BEVR_FUSED_KV", "BEVR_CELL")


def desc(S=400, precision=X3, **over):
    d = ops.AttnGeom(n_prob=2, q_div=1, heads=2, groups=1, S=S, N=100, Wt=2 * S * 3 - 1, precision=precision).desc()
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


@pytest.fixture()
def clean_env(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    return monkeypatch


def x3(L, d, row0, n_rows, ptrs=None):
    a = [P] * 9 if ptrs is None else ptrs          # Q K V key_ws table_pk2 mref O LSE flags
    return L.bevr_attn_gather_fwd_x3(C.byref(d), *a, row0, n_rows, None)


def test_symbol_is_declared_bound_and_exported(L):
    assert NAME in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "bevrender_hip.h")).read()
    assert re.search(r"\bint\s+bevr_attn_gather_fwd_x3\s*\(", header)
    fn = L.bevr_attn_gather_fwd_x3
    assert fn.restype is C.c_int and len(fn.argtypes) == 13
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT bevr_attn_gather_fwd_x3$", out, re.M)
    assert L.bevr_abi_version() == 6 and _lib.ABI_VERSION == 6          # additive: no new version


def test_precision_contract(L):
    for prec in (BF16, F16, F32, 9):
        assert x3(L, desc(precision=prec), 0, 208) == E_PRECISION, prec
        assert x3(L, desc(S=12, precision=prec), 0, 12) == E_PRECISION, prec
    # the two 16-bit entry points keep refusing the split mode
    assert L.bevr_attn_gather_fwd(C.byref(desc(S=12)), *([P] * 9), None) == E_PRECISION
    assert L.bevr_attn_gather_fwd_rows(C.byref(desc()), *([P] * 9), 0, 208, None) == E_PRECISION


@pytest.mark.parametrize("S", [12, 200, 400, 448])
def test_row_range_contract(L, S):
    d = desc(S=S)
    bad = [(0, 225), (8, 4), (-16, 32), (0, 0), (0, -5), (0, S + 1), (16 * ((S - 1) // 16), 17), (S, 1),
           (16, S), (0, 1 << 30), (1 << 30, 16)]
    for row0, n in bad:
        assert x3(L, d, row0, n) == E_SHAPE, (S, row0, n)


def test_bad_descriptor_null_and_misaligned_pointers(L):
    for over in (dict(Sp=16), dict(Np=101), dict(Ht=20), dict(heads=3, groups=2), dict(Hp=7)):
        assert x3(L, desc(**over), 0, 208) == E_SHAPE, over
    d = desc()
    for i in range(9):
        a = [P] * 9
        a[i] = None
        assert x3(L, d, 0, 208, a) == E_NULL, i
    for i in (0, 1, 2, 3, 6):          # Q, K, V, key_ws, O
        a = [P] * 9
        a[i] = ODD
        assert x3(L, d, 0, 208, a) == E_ALIGN, i
    # the order: pointers, then precision, then the row range
    assert x3(L, desc(precision=F32), 0, 225, [None] + [P] * 8) == E_NULL
    assert x3(L, desc(precision=F32), 0, 225, [ODD] + [P] * 8) == E_ALIGN
    assert x3(L, desc(precision=F32), 0, 225) == E_PRECISION
    assert x3(L, desc(), 0, 225) == E_SHAPE
    # every band ops would launch passes the range check (and fails only at the null operand)
    for S in (21, 200, 232, 400, 448):
        for r0, n in ops.gather_bands(S):
            assert x3(L, desc(S=S), r0, n, [None] + [P] * 8) == E_NULL


def seg(r):
    return [(s.kind, s.n0, s.n1, s.fwd, s.bwd_q, s.bwd_k) for s in r.segments]


TILE = ("bevr_attn_fwd", "bevr_attn_bwd_q", "bevr_attn_bwd_k")
CELL = ("bevr_attn_cell_fwd", "bevr_attn_cell_bwd_q", "bevr_attn_cell_bwd_k")
TAP = ("bevr_attn_tap_fwd", "bevr_attn_tap_bwd_q", "bevr_attn_tap_bwd_k")
DROP = ("bevr_attn_fwd_dropout", "bevr_attn_bwd_q_dropout", "bevr_attn_bwd_k_dropout")


def test_unset_switch_keeps_every_route(clean_env):
    """BEVR_GATHER_X3 unset: what attention_route returned before the switch existed, spelled out."""
    assert ops.GATHER_X3_DEFAULT == "0"
    for S in (8, 21, 200, 400, 448, 449):
        assert not ops.gather_supported(X3, S)
    NK = 5000
    for S in (21, 200, 400):
        r = ops.attention_route(X3, 1, S, 2 * S * 5 - 1, NK)
        assert seg(r) == [("region", 0, NK) + TILE] and r.gather is None and not r.kn2 and r.merge == "merge_views"
    r = ops.attention_route(X3, 1, 200, 1999, NK, cell_split=1024)
    assert seg(r) == [("region", 0, 1024) + TILE, ("cell", 1024, NK) + CELL] and r.gather is None
    r = ops.attention_route(X3, 1, 200, 1999, NK, dropout=True)
    assert seg(r) == [("region", 0, NK) + DROP] and r.gather is None
    clean_env.setenv("BEVR_TAP_X3", "1")
    r = ops.attention_route(X3, 1, 200, 1999, NK, cell_split=1024, tap_source=True, source="tap_pix", C=64, heads=2)
    assert seg(r) == [("region", 0, 1024) + TILE, ("tap", 1024, NK) + TAP] and r.gather is None and r.merge == "merge_tap"
    # "0" is the unset behaviour too
    clean_env.setenv("BEVR_GATHER_X3", "0")
    assert not ops.gather_supported(X3, 200)
    assert seg(ops.attention_route(X3, 1, 200, 1999, NK)) == [("region", 0, NK) + TILE]


def test_switch_routes_the_region_forward_only(clean_env):
    clean_env.setenv("BEVR_GATHER_X3", "1")
    assert ops.K.GATHER_X3 == NAME and NAME in ops._RUN
    NK = 5000
    GX = (NAME, "bevr_attn_bwd_q", "bevr_attn_bwd_k")          # the backward entries are the parent's
    for S, how in ((21, "whole"), (200, "whole"), (400, "bands")):
        assert ops.gather_supported(X3, S)
        r = ops.attention_route(X3, 1, S, 2 * S * 5 - 1, NK)
        assert seg(r) == [("region", 0, NK) + GX] and r.gather == how and not r.kn2 and r.merge == "merge_views"
    assert ops.gather_supported(X3, 448) and not ops.gather_supported(X3, 449)
    assert seg(ops.attention_route(X3, 1, 449, 4489, NK)) == [("region", 0, NK) + TILE]
    # beside a cell segment and beside a tap segment: only the region segment's forward moves
    r = ops.attention_route(X3, 1, 200, 1999, NK, cell_split=1024)
    assert seg(r) == [("region", 0, 1024) + GX, ("cell", 1024, NK) + CELL]
    clean_env.setenv("BEVR_TAP_X3", "1")
    r = ops.attention_route(X3, 1, 200, 1999, NK, cell_split=1024, tap_source=True, source="tap_pix", C=64, heads=2)
    assert seg(r) == [("region", 0, 1024) + GX, ("tap", 1024, NK) + TAP] and r.merge == "merge_tap" and not r.kn2
    # dropout keeps the dropout kernels
    r = ops.attention_route(X3, 1, 200, 1999, NK, dropout=True)
    assert seg(r) == [("region", 0, NK) + DROP] and r.gather is None
    # F32 is never routed to it; the 16-bit modes keep their own gather entry points
    for S in (21, 200, 400):
        assert not ops.gather_supported(F32, S)
        assert seg(ops.attention_route(F32, 1, S, 2 * S * 5 - 1, NK)) == [("region", 0, NK) + TILE]
    assert ops.attention_route(BF16, 1, 21, 209, NK).segments[0].fwd == "bevr_attn_gather_fwd"
    assert ops.attention_route(F16, 1, 400, 3999, NK).segments[0].fwd == "bevr_attn_gather_fwd_rows"
    # BEVR_GATHER=0 turns the new route off too
    clean_env.setenv("BEVR_GATHER", "0")
    assert not ops.gather_supported(X3, 200)
    assert seg(ops.attention_route(X3, 1, 200, 1999, NK)) == [("region", 0, NK) + TILE]


def test_gather_split_table():
    gen = torch.Generator().manual_seed(4)
    T = torch.randn(2, 11, 37, generator=gen) * torch.logspace(-3, 2, 37)          # (h, Wp, Hp + 1): six decades of sizes
    pair = torch.stack((T[..., :-1], T[..., 1:]), dim=-1).contiguous()             # (h, Wp, Hp, 2)
    pk2 = ops.gather_split_table(pair)
    assert pk2.shape == (2, 2, 11, 36, 2) and pk2.dtype == torch.bfloat16 and pk2.is_contiguous()
    assert torch.equal(pk2[0], pair.to(torch.bfloat16))
    assert torch.equal(pk2[1], (pair - pk2[0].float()).to(torch.bfloat16))
    back = pk2[0].float() + pk2[1].float()
    assert ((back - pair).abs() <= 2.0 ** -16 * pair.abs()).all()
    # one dword per (column, row) entry and plane, as the kernel reads it
    assert pk2.view(torch.int32).shape == (2, 2, 11, 36, 1)
