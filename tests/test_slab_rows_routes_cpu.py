"""Which calls the row-band slab backward takes (ops.slab_rows_supported, ops.attention_route), without a GPU: behind
BEVR_SLAB_ROWS and nowhere else -- with the switch unset every route is the one tests/test_attention_routes_cpu.py pins."""
import pytest

from bevrender_amd import _lib, ops

F32, X3, BF16, F16 = _lib.PREC_F32, _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16
SWITCHES = ("BEVR_GATHER", "BEVR_SLAB", "BEVR_KNORM", "BEVR_MERGE_TAP", "BEVR_TAP", "BEVR_TAP_X3", "BEVR_FUSED_KV", "BEVR_CELL")
GATHER, ROWS = "bevr_attn_gather_fwd", "bevr_attn_gather_fwd_rows"
TILE_Q, SLAB, SLAB_ROWS = "bevr_attn_bwd_q", "bevr_attn_slab_bwd_q", "bevr_attn_slab_bwd_q_rows"
TAP = ("bevr_attn_tap_fwd", "bevr_attn_tap_bwd_q", "bevr_attn_tap_bwd_k")
NK = 4096


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in SWITCHES + ("BEVR_SLAB_ROWS",):
        monkeypatch.delenv(name, raising=False)


def tsa(S):
    return 2 * S - 1


def sca(S):     # depth 4
    return 2 * S * 4 - 1


def route(prec, S, Wt, **kw):
    kw.setdefault("C", 64)
    kw.setdefault("heads", 2)
    return ops.attention_route(prec, kw.pop("groups", 1), S, Wt, kw.pop("N", NK), **kw)


def names(r):
    return [(s.kind, s.n0, s.n1, s.fwd, s.bwd_q, s.bwd_k) for s in r.segments]


def region(n, fwd="bevr_attn_fwd", bwd_q=TILE_Q, bwd_k="bevr_attn_bwd_k"):
    return ("region", 0, n, fwd, bwd_q, bwd_k)


def test_entry_point_name_and_launcher():
    assert ops.K.SLAB_BWD_Q_ROWS == SLAB_ROWS and ops._RUN[SLAB_ROWS] is ops._bwd_q_slab_rows
    assert ops._RUN[SLAB] is ops._bwd_q_slab


def test_switch_unset_or_zero_changes_no_route(monkeypatch):
    for value in (None, "0", "", "yes"):
        if value is not None:
            monkeypatch.setenv("BEVR_SLAB_ROWS", value)
        for prec in (BF16, F16):
            assert not ops.slab_rows_supported(prec, 400, sca(400)) and not ops.slab_rows_supported(prec, 40)
            assert names(route(prec, 212, sca(212))) == [region(NK, GATHER, TILE_Q)]
            assert names(route(prec, 400, sca(400))) == [region(NK, ROWS, TILE_Q)]
            assert names(route(prec, 448, sca(448))) == [region(NK, ROWS, TILE_Q)]
            assert names(route(prec, 200, sca(200))) == [region(NK, GATHER, SLAB)]


def test_switch_one_takes_the_sides_above_the_one_band_kernel(monkeypatch):
    monkeypatch.setenv("BEVR_SLAB_ROWS", "1")
    for prec in (BF16, F16):
        for S, fwd in ((212, GATHER), (400, ROWS), (448, ROWS)):
            for source in ("kv", "kv_source"):
                r = route(prec, S, sca(S), source=source)
                assert names(r) == [region(NK, fwd, SLAB_ROWS)], (prec, S)
                assert r.merge == "merge_views" and not r.tap and r.split == NK
            assert ops.slab_rows_supported(prec, S, sca(S)) and ops.slab_rows_supported(prec, S)
        # everything else as it is today
        assert names(route(prec, 211, sca(211))) == [region(NK, GATHER, SLAB)]
        assert names(route(prec, 40, sca(40))) == [region(NK, GATHER, SLAB)]
        assert names(route(prec, 400, tsa(400))) == [region(NK, ROWS, TILE_Q)]
        assert names(route(prec, 212, tsa(212))) == [region(NK, GATHER, TILE_Q)]
        assert names(route(prec, 449, sca(449))) == [region(NK, "bevr_attn_fwd", TILE_Q)]
        r = route(prec, 400, sca(400), dropout=True)
        assert names(r) == [region(NK, "bevr_attn_fwd_dropout", "bevr_attn_bwd_q_dropout", "bevr_attn_bwd_k_dropout")]
    for prec in (F32, X3):
        for S in (200, 212, 400):
            assert names(route(prec, S, sca(S))) == [region(NK)]
            assert not ops.slab_rows_supported(prec, S, sca(S))
    # the widest TSA-like table that keeps the query-tile kernel, the narrowest that leaves it
    assert not ops.slab_rows_supported(BF16, 400, 4 * 399) and ops.slab_rows_supported(BF16, 400, 4 * 399 + 1)


def test_switch_one_follows_the_slab_switch(monkeypatch):
    monkeypatch.setenv("BEVR_SLAB_ROWS", "1")
    monkeypatch.setenv("BEVR_SLAB", "0")
    for prec in (BF16, F16):
        assert names(route(prec, 400, sca(400))) == [region(NK, ROWS, TILE_Q)]
        assert names(route(prec, 200, sca(200))) == [region(NK, GATHER, TILE_Q)]
    monkeypatch.setenv("BEVR_SLAB", "2")          # every table width, each kernel within its sides
    assert names(route(BF16, 400, tsa(400))) == [region(NK, ROWS, SLAB_ROWS)]
    assert names(route(BF16, 200, tsa(200))) == [region(NK, GATHER, SLAB)]
    assert names(route(BF16, 449, tsa(449))) == [region(NK, "bevr_attn_fwd", TILE_Q)]
    monkeypatch.setenv("BEVR_SLAB", "1")
    assert names(route(BF16, 400, sca(400))) == [region(NK, ROWS, SLAB_ROWS)]


@pytest.mark.parametrize("tap_source", [True, "pinned"])
def test_tap_and_cell_splits_keep_their_second_segment(tap_source, monkeypatch):
    monkeypatch.setenv("BEVR_SLAB_ROWS", "1")
    for prec in (BF16, F16):
        r = route(prec, 400, sca(400), cell_split=1024, tap_source=tap_source, source="kv_source")
        assert names(r) == [region(1024, ROWS, SLAB_ROWS), ("tap", 1024, NK) + TAP]
        assert r.tap and r.n_core == 1024 and r.split == 1024 and r.merge == "merge_tap" and r.kn2
        r = route(prec, 400, sca(400), cell_split=1024)
        assert names(r) == [region(1024, ROWS, SLAB_ROWS),
                            ("cell", 1024, NK, "bevr_attn_cell_fwd", "bevr_attn_cell_bwd_q", "bevr_attn_cell_bwd_k")]
        # with a keep mask the region half is the dropout kernels', as without the switch
        r = route(prec, 400, sca(400), cell_split=1024, tap_source="pinned", dropout=True, source="kv_source")
        assert r.segments[0].bwd_q == "bevr_attn_bwd_q_dropout"


def test_switch_two_forces_the_route_within_the_kernel_limits(monkeypatch):
    monkeypatch.setenv("BEVR_SLAB_ROWS", "2")
    for prec in (BF16, F16):
        assert names(route(prec, 40, sca(40))) == [region(NK, GATHER, SLAB_ROWS)]
        assert names(route(prec, 200, tsa(200))) == [region(NK, GATHER, SLAB_ROWS)]
        assert names(route(prec, 400, tsa(400))) == [region(NK, ROWS, SLAB_ROWS)]
        assert names(route(prec, 449, sca(449))) == [region(NK, "bevr_attn_fwd", TILE_Q)]
        assert route(prec, 40, sca(40), dropout=True).segments[0].bwd_q == "bevr_attn_bwd_q_dropout"
    monkeypatch.setenv("BEVR_SLAB", "0")          # forced: ahead of the one-band kernel's own switch
    assert names(route(BF16, 40, sca(40))) == [region(NK, GATHER, SLAB_ROWS)]
    for prec in (F32, X3):
        assert names(route(prec, 40, sca(40))) == [region(NK)]
