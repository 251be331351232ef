"""Which kernels an attention call runs, without a GPU: every refusal of ops.attention_core (CPU tensors: all of them fire
before a kernel), and the decision ops.attention_route makes -- the key segments and the entry points of their forward,
query-side and key-side backward -- as a table of literals over precision, grid side, table width, split, tap_source,
dropout, channel groups, source and every A/B switch."""
import pytest
import torch

from bevrender_amd import _lib, ops

F32, X3, BF16, F16 = _lib.PREC_F32, _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16
SWITCHES = ("BEVR_GATHER", "BEVR_SLAB", "BEVR_KNORM", "BEVR_MERGE_TAP", "BEVR_TAP", "BEVR_TAP_X3", "BEVR_FUSED_KV", "BEVR_CELL")


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


# --------------------------------------------------------------------------------------------------
# refusals, through attention_core itself
# --------------------------------------------------------------------------------------------------
B, V, C, H, S, N = 1, 1, 16, 2, 4, 8
WT = 2 * S * 2 - 1


def _args(**over):
    """A valid explicit K | V call of attention_core (CPU tensors) with `over` laid on top."""
    gen = torch.Generator().manual_seed(0)
    kw = dict(query=torch.randn(B, C, S, S, generator=gen), kproj=None, vproj=None, pos=torch.rand(B * V, N, 2, generator=gen) * 2 - 1,
              rpe_table=torch.zeros(H, 2 * S - 1, WT), heads=H, groups=1, views=V, precision=BF16,
              kv=torch.randn(B * V, N, 2 * C, generator=gen))
    kw.update(over)
    return kw


def _source(c=C, n=B * V):
    return (torch.zeros(n, 5, 6, c), torch.zeros(2 * c, c), torch.zeros(2 * c))


def _call(**over):
    kw = _args(**over)
    return ops.attention_core(kw.pop("query"), kw.pop("kproj"), kw.pop("vproj"), kw.pop("pos"), kw.pop("rpe_table"), **kw)


REFUSALS = {
    "drop_p_one": (dict(attn_drop=(1.0, 3)), "attention dropout probability must lie in (0, 1)"),
    "drop_p_rounds_to_zero": (dict(attn_drop=(1e-9, 3)), "attention dropout probability must lie in (0, 1)"),
    "tap_pix_dropout": (dict(kv=torch.zeros(B * V, 4, 2 * C), cell_split=4, tap_source="pinned", tap_pix=_source(),
                             attn_drop=(0.1, 3)),
                        "tap_pix has no attention dropout: pass every key's projected rows and no tap segment"),
    "kv_source_and_kv": (dict(kv_source=_source()), "pass kv_source alone"),
    "kv_source_and_kproj": (dict(kv=None, kproj=torch.zeros(B * V, N, C), kv_source=_source()), "pass kv_source alone"),
    "kv_source_f32": (dict(kv=None, kv_source=_source(), precision=F32),
                      "kv_source needs a 16-bit operand mode, C % 16 == 0 and (C / groups) % 4 == 0"),
    "kv_source_bf16x3": (dict(kv=None, kv_source=_source(), precision=X3),
                         "kv_source needs a 16-bit operand mode, C % 16 == 0 and (C / groups) % 4 == 0"),
    "kv_source_feat_batch": (dict(kv=None, kv_source=_source(n=2)),
                             "kv_source shapes: feat (B*views, Hi, Wi, C), pos (B*views*groups, N, 2), Wkv (2C, C)"),
    "kv_source_weight": (dict(kv=None, kv_source=(torch.zeros(1, 5, 6, C), torch.zeros(C, C), None)),
                         "kv_source shapes: feat (B*views, Hi, Wi, C), pos (B*views*groups, N, 2), Wkv (2C, C)"),
    "kv_and_kproj": (dict(kproj=torch.zeros(B * V, N, C)), "pass either kproj and vproj, or kv"),
    "kv_channels": (dict(kv=torch.zeros(B * V, N, C)), f"K | V rows must have 2 x {C} channels, got {C}"),
    "tap_pix_without_tap_source": (dict(kv=torch.zeros(B * V, 4, 2 * C), cell_split=4, tap_pix=_source()),
                                   "tap_pix needs tap_source, cell_split and the projected rows of the keys [0, cell_split) alone"),
    "tap_pix_without_split": (dict(kv=torch.zeros(B * V, 4, 2 * C), tap_source="pinned", tap_pix=_source()),
                              "tap_pix needs tap_source, cell_split and the projected rows of the keys [0, cell_split) alone"),
    "tap_pix_all_rows": (dict(cell_split=4, tap_source="pinned", tap_pix=_source()),
                         "tap_pix needs tap_source, cell_split and the projected rows of the keys [0, cell_split) alone"),
    "tap_pix_shapes": (dict(kv=torch.zeros(B * V, 4, 2 * C), cell_split=4, tap_source="pinned", tap_pix=_source(n=2)),
                       "tap_pix shapes: feat (B*views, Hi, Wi, C), Wkv (2C, C), bkv (2C,)"),
    "split_above_n": (dict(cell_split=N + 1), "cell_split must lie in [0, N]"),
    "split_negative": (dict(cell_split=-1), "cell_split must lie in [0, N]"),
    "table_height": (dict(rpe_table=torch.zeros(H, 2 * S, WT)), "rpe_table height must be 2S-1"),
    "tap_without_source": (dict(cell_split=4, tap_source=True),
                           "tap_source needs kv_source or tap_pix, groups == 1, a precision tap_supported accepts and S <= 448"),
    "tap_groups": (dict(kv=None, kv_source=_source(), pos=torch.zeros(2 * B * V, N, 2), groups=2, cell_split=4, tap_source="pinned"),
                   "tap_source needs kv_source or tap_pix, groups == 1, a precision tap_supported accepts and S <= 448"),
    "tap_pix_f32": (dict(kv=torch.zeros(B * V, 4, 2 * C), cell_split=4, tap_source="pinned", tap_pix=_source(), precision=F32),
                    "tap_source needs kv_source or tap_pix, groups == 1, a precision tap_supported accepts and S <= 448"),
    "tap_pix_no_segment": (dict(cell_split=N, tap_source="pinned", tap_pix=_source()),
                           "tap_pix needs a tap segment: 0 <= cell_split < N"),
    "head_dim": (dict(query=torch.zeros(B, 66, S, S), kv=torch.zeros(B * V, N, 132), heads=2),
                 "head_dim 33 > 32 is not supported by the gfx950 kernels"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_attention_core_refuses(case):
    over, message = REFUSALS[case]
    with pytest.raises(ValueError) as err:
        _call(**over)
    assert str(err.value) == message


def test_tap_switch_off_refuses_a_tap_call(monkeypatch):
    """BEVR_TAP=0: tap_supported is False, so a call that asks for the tap kernels outright is refused (the module asks
    tap_supported first and keeps the keys on the cell kernels)."""
    monkeypatch.setenv("BEVR_TAP", "0")
    with pytest.raises(ValueError) as err:
        _call(kv=None, kv_source=_source(), cell_split=4, tap_source="pinned")
    assert str(err.value) == "tap_source needs kv_source or tap_pix, groups == 1, a precision tap_supported accepts and S <= 448"


# --------------------------------------------------------------------------------------------------
# the decision, as literals
# --------------------------------------------------------------------------------------------------
TILE = ("bevr_attn_fwd", "bevr_attn_bwd_q", "bevr_attn_bwd_k")
TILE_DROP = ("bevr_attn_fwd_dropout", "bevr_attn_bwd_q_dropout", "bevr_attn_bwd_k_dropout")
CELL = ("bevr_attn_cell_fwd", "bevr_attn_cell_bwd_q", "bevr_attn_cell_bwd_k")
TAP = ("bevr_attn_tap_fwd", "bevr_attn_tap_bwd_q", "bevr_attn_tap_bwd_k")
TAP_DROP = ("bevr_attn_tap_fwd_dropout", "bevr_attn_tap_bwd_q_dropout", "bevr_attn_tap_bwd_k_dropout")
GATHER, ROWS, SLAB = "bevr_attn_gather_fwd", "bevr_attn_gather_fwd_rows", "bevr_attn_slab_bwd_q"
FAMILY = {"region": set(TILE + TILE_DROP) | {GATHER, ROWS, SLAB}, "cell": set(CELL), "tap": set(TAP + TAP_DROP)}
NK = 4096       # keys


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


def region(n, fwd="bevr_attn_fwd", bwd_q="bevr_attn_bwd_q", bwd_k="bevr_attn_bwd_k"):
    return ("region", 0, n, fwd, bwd_q, bwd_k)


def check_consistency(r, N=NK):
    """every segment's three entry points are of its kernel family, all with the keep mask or none; the segments tile [0, N)"""
    assert r.segments[0].n0 == 0 and r.segments[-1].n1 == N
    for s, t in zip(r.segments, r.segments[1:]):
        assert s.n1 == t.n0
    for s in r.segments:
        assert {s.fwd, s.bwd_q, s.bwd_k} <= FAMILY[s.kind], s
        assert len({"dropout" in n for n in (s.fwd, s.bwd_q, s.bwd_k)}) == 1, s
        assert "_fwd" in s.fwd and "bwd_q" in s.bwd_q and "bwd_k" in s.bwd_k, s
    assert r.merge in ("merge_tap", "merge_views")


# no split, scattered keys: the forward and the query-side backward by precision, BEV side and table width
#   gather forward: 16-bit modes, whole up to S = 224, in bands up to 448; slab backward: 16-bit, S <= 211, SCA-wide tables
REGION_TABLE = [
    # S,   table, {precision: (forward, bwd_q)}
    (40, tsa, {BF16: (GATHER, "bevr_attn_bwd_q"), F16: (GATHER, "bevr_attn_bwd_q")}),
    (40, sca, {BF16: (GATHER, SLAB), F16: (GATHER, SLAB)}),
    (200, tsa, {BF16: (GATHER, "bevr_attn_bwd_q"), F16: (GATHER, "bevr_attn_bwd_q")}),
    (200, sca, {BF16: (GATHER, SLAB), F16: (GATHER, SLAB)}),
    (211, sca, {BF16: (GATHER, SLAB), F16: (GATHER, SLAB)}),
    (212, sca, {BF16: (GATHER, "bevr_attn_bwd_q"), F16: (GATHER, "bevr_attn_bwd_q")}),
    (400, tsa, {BF16: (ROWS, "bevr_attn_bwd_q"), F16: (ROWS, "bevr_attn_bwd_q")}),
    (400, sca, {BF16: (ROWS, "bevr_attn_bwd_q"), F16: (ROWS, "bevr_attn_bwd_q")}),
    (448, sca, {BF16: (ROWS, "bevr_attn_bwd_q"), F16: (ROWS, "bevr_attn_bwd_q")}),
    (449, sca, {BF16: ("bevr_attn_fwd", "bevr_attn_bwd_q"), F16: ("bevr_attn_fwd", "bevr_attn_bwd_q")}),
]


@pytest.mark.parametrize("S,table,want", REGION_TABLE, ids=[f"S{S}-{t.__name__}" for S, t, _ in REGION_TABLE])
@pytest.mark.parametrize("source", ["kv", "kv_source"])
def test_region_route_by_precision_side_and_table(S, table, want, source):
    for prec in (BF16, F16):
        r = route(prec, S, table(S), source=source)
        fwd, bwd_q = want[prec]
        assert names(r) == [region(NK, fwd, bwd_q)], (prec, names(r))
        assert r.gather == {GATHER: "whole", ROWS: "bands", "bevr_attn_fwd": None}[fwd]
        assert r.kn2 == (source == "kv_source" and fwd != "bevr_attn_fwd")       # the gather forward's reference
        assert r.merge == "merge_views" and not r.tap and r.n_core == NK and r.split == NK
        check_consistency(r)
    for prec in (F32, X3):          # the float layouts: the query-tile kernels everywhere (no fused source)
        r = route(prec, S, table(S))
        assert names(r) == [region(NK)] and r.gather is None and not r.kn2
        check_consistency(r)


def test_one_row_band_up_to_224():
    assert route(BF16, 224, sca(224)).gather == "whole" and route(BF16, 225, sca(225)).gather == "bands"


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("source", ["kv", "kv_source"])
def test_cell_split(groups, source):
    """a cell split is kept for any groups and source; the region half keeps its own route"""
    for prec in (BF16, F16):
        r = route(prec, 200, sca(200), cell_split=1024, source=source, groups=groups)
        assert names(r) == [region(1024, GATHER, SLAB), ("cell", 1024, NK) + CELL]
        assert r.split == 1024 and r.n_core == NK and not r.tap and r.merge == "merge_views"
        assert r.kn2 == (source == "kv_source")
        check_consistency(r)
    if source == "kv":
        for prec in (F32, X3):
            assert names(route(prec, 200, sca(200), cell_split=1024, groups=groups)) == [region(1024), ("cell", 1024, NK) + CELL]
    # the ends of the range: one segment
    assert names(route(BF16, 200, sca(200), cell_split=0, source=source, groups=groups)) == [("cell", 0, NK) + CELL]
    assert names(route(BF16, 200, sca(200), cell_split=NK, source=source, groups=groups)) == [region(NK, GATHER, SLAB)]
    assert not route(BF16, 200, sca(200), cell_split=0, source="kv_source", groups=groups).kn2         # no region segment


def test_cell_kernels_size_limits():
    """Sp > 480, Sp > 224 with f32-sized operands, more than 8 x 100 x 1024 keys: every key on the region kernels; the
    caller's split stays on record (its keys are still ordered as it promised)"""
    r = route(BF16, 449, sca(449), cell_split=1024)                        # Sp = 480: still the cell kernels
    assert names(r) == [region(1024), ("cell", 1024, NK) + CELL]
    r = route(BF16, 481, sca(481), cell_split=1024)
    assert names(r) == [region(NK)] and r.split == 1024
    for prec in (F32, X3):
        assert names(route(prec, 224, sca(224), cell_split=1024)) == [region(1024), ("cell", 1024, NK) + CELL]
        r = route(prec, 225, sca(225), cell_split=1024)
        assert names(r) == [region(NK)] and r.split == 1024
    big = 8 * 100 * 1024
    assert names(route(BF16, 200, sca(200), N=big + 64, cell_split=64)) == [region(64, GATHER, SLAB), ("cell", 64, big + 64) + CELL]
    assert names(route(BF16, 200, sca(200), N=big + 65, cell_split=64)) == [region(big + 65, GATHER, SLAB)]


@pytest.mark.parametrize("tap_source", [True, "pinned"])
def test_tap_split(tap_source, monkeypatch):
    for prec in (BF16, F16):
        for S, fwd, bwd_q in ((40, GATHER, SLAB), (200, GATHER, SLAB), (211, GATHER, SLAB), (212, GATHER, "bevr_attn_bwd_q"),
                              (400, ROWS, "bevr_attn_bwd_q"), (448, ROWS, "bevr_attn_bwd_q")):
            r = route(prec, S, sca(S), cell_split=1024, tap_source=tap_source, source="kv_source")
            assert names(r) == [region(1024, fwd, bwd_q), ("tap", 1024, NK) + TAP], (prec, S)
            assert r.tap and r.n_core == 1024 and r.split == 1024 and r.merge == "merge_tap" and r.kn2
            check_consistency(r)
        r = route(prec, 200, sca(200), cell_split=0, tap_source=tap_source, source="kv_source")
        assert names(r) == [("tap", 0, NK) + TAP] and r.n_core == 0 and r.merge == "merge_views" and not r.kn2
        # head widths the fused merge does not take
        assert route(prec, 200, sca(200), cell_split=1024, tap_source=tap_source, source="kv_source", C=48).merge == "merge_tap"
        assert route(prec, 200, sca(200), cell_split=1024, tap_source=tap_source, source="kv_source", C=48, heads=8).merge \
            == "merge_views"
        # no tap segment asked for after all
        assert names(route(prec, 200, sca(200), cell_split=NK, tap_source=tap_source, source="kv_source")) \
            == [region(NK, GATHER, SLAB)]
    # split-bf16: beside projected rows (tap_pix), behind its switch
    monkeypatch.setenv("BEVR_TAP_X3", "1")
    r = route(X3, 200, sca(200), cell_split=1024, tap_source=tap_source, source="tap_pix")
    assert names(r) == [region(1024), ("tap", 1024, NK) + TAP] and r.merge == "merge_tap" and not r.kn2
    check_consistency(r)
    r = route(BF16, 200, sca(200), cell_split=1024, tap_source=tap_source, source="tap_pix")        # 16-bit rows beside it
    assert names(r) == [region(1024, GATHER, SLAB), ("tap", 1024, NK) + TAP] and not r.kn2
    for bad in (dict(source="kv"), dict(source="kv_source", groups=2), dict(source="tap_pix", prec=F32),
                dict(source="kv_source", S=449)):
        S = bad.pop("S", 200)
        with pytest.raises(ValueError, match="tap_source needs kv_source or tap_pix"):
            route(bad.pop("prec", BF16), S, sca(S), cell_split=1024, tap_source=tap_source, **bad)
    monkeypatch.setenv("BEVR_TAP_X3", "0")
    with pytest.raises(ValueError, match="tap_source needs kv_source or tap_pix"):
        route(X3, 200, sca(200), cell_split=1024, tap_source=tap_source, source="tap_pix")
    with pytest.raises(ValueError, match="tap_pix needs a tap segment"):
        route(BF16, 200, sca(200), cell_split=NK, tap_source=tap_source, source="tap_pix")


def _never(split):
    raise AssertionError("this call must not look at the keys")


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("source", ["kv", "kv_source"])
@pytest.mark.parametrize("cell_split", [None, 0, 1024, NK])
def test_dropout_without_tap_source_runs_every_key_on_the_region_dropout_kernels(groups, source, cell_split):
    for prec in (BF16, F16) + ((F32, X3) if source == "kv" else ()):
        for S, table in ((40, tsa), (200, sca), (400, sca), (449, sca)):
            r = route(prec, S, table(S), cell_split=cell_split, dropout=True, source=source, groups=groups, keys_in_tap_grid=_never)
            assert names(r) == [("region", 0, NK) + TILE_DROP] and r.split == NK and r.gather is None and not r.kn2
            assert r.merge == "merge_views"
            check_consistency(r)
    # (cell_split is ignored, out of range included)
    assert names(route(BF16, 200, sca(200), cell_split=NK + 7, dropout=True)) == [("region", 0, NK) + TILE_DROP]


def test_dropout_with_pinned_keys_keeps_the_split_on_the_tap_kernels():
    for prec in (BF16, F16):
        for S in (40, 200, 400, 448):
            r = route(prec, S, sca(S), cell_split=1024, tap_source="pinned", dropout=True, source="kv_source", keys_in_tap_grid=_never)
            assert names(r) == [("region", 0, 1024) + TILE_DROP, ("tap", 1024, NK) + TAP_DROP]
            assert r.merge == "merge_views" and not r.kn2 and r.gather is None and r.split == 1024 and r.n_core == 1024
            check_consistency(r)
        assert names(route(prec, 200, sca(200), cell_split=0, tap_source="pinned", dropout=True, source="kv_source")) \
            == [("tap", 0, NK) + TAP_DROP]
        # what the tap dropout kernels do not take falls back to the region kernels, silently (any split is a valid result)
        for kw in (dict(S=449), dict(groups=2), dict(source="kv")):
            S = kw.pop("S", 200)
            kw.setdefault("source", "kv_source")
            r = route(prec, S, sca(S), cell_split=1024, tap_source="pinned", dropout=True, keys_in_tap_grid=_never, **kw)
            assert names(r) == [("region", 0, NK) + TILE_DROP] and r.split == NK
    with pytest.raises(ValueError, match="tap_pix has no attention dropout"):
        route(X3, 200, sca(200), cell_split=1024, tap_source="pinned", dropout=True, source="tap_pix")


def test_the_checked_tap_contract_is_evaluated_once_and_only_where_it_syncs_today():
    calls = []

    def inside(split):
        calls.append(split)
        return True

    def outside(split):
        calls.append(split)
        return False
    r = route(BF16, 200, sca(200), cell_split=1024, tap_source=True, dropout=True, source="kv_source", keys_in_tap_grid=inside)
    assert calls == [1024] and names(r) == [("region", 0, 1024) + TILE_DROP, ("tap", 1024, NK) + TAP_DROP]
    del calls[:]
    r = route(BF16, 200, sca(200), cell_split=1024, tap_source=True, dropout=True, source="kv_source", keys_in_tap_grid=outside)
    assert calls == [1024] and names(r) == [("region", 0, NK) + TILE_DROP] and r.split == NK
    # never otherwise: the promise, no mask, no tap_source, no segment beside or behind the split, a call the tap dropout
    # kernels do not take
    for kw in (dict(tap_source="pinned", dropout=True), dict(tap_source=True), dict(tap_source=False, dropout=True),
               dict(tap_source=True, dropout=True, cell_split=0), dict(tap_source=True, dropout=True, cell_split=NK),
               dict(tap_source=True, dropout=True, cell_split=None), dict(tap_source=True, dropout=True, S=449),
               dict(tap_source=True, dropout=True, groups=2), dict(tap_source=True, dropout=True, source="kv")):
        S = kw.pop("S", 200)
        kw.setdefault("cell_split", 1024)
        kw.setdefault("source", "kv_source")
        route(BF16, S, sca(S), keys_in_tap_grid=_never, **kw)
    # split 0 with the checked contract: the route dropout always took for such a call
    assert names(route(BF16, 200, sca(200), cell_split=0, tap_source=True, dropout=True, source="kv_source",
                       keys_in_tap_grid=_never)) == [("region", 0, NK) + TILE_DROP]


def test_switches(monkeypatch):
    """each A/B switch at its other value (the default values are every table above)"""
    def tapped(**kw):
        return route(BF16, 200, sca(200), cell_split=1024, tap_source="pinned", source="kv_source", **kw)
    monkeypatch.setenv("BEVR_GATHER", "0")
    r = route(BF16, 200, sca(200), source="kv_source")
    assert names(r) == [region(NK, "bevr_attn_fwd", SLAB)] and r.gather is None and not r.kn2
    assert names(route(F16, 400, sca(400))) == [region(NK)]
    monkeypatch.setenv("BEVR_GATHER", "1")
    assert names(route(BF16, 200, sca(200))) == [region(NK, GATHER, SLAB)]
    monkeypatch.delenv("BEVR_GATHER")

    monkeypatch.setenv("BEVR_SLAB", "0")
    assert names(route(BF16, 200, sca(200))) == [region(NK, GATHER, "bevr_attn_bwd_q")]
    monkeypatch.setenv("BEVR_SLAB", "2")        # forced for every table -- within the kernel's limits
    assert names(route(BF16, 200, tsa(200))) == [region(NK, GATHER, SLAB)]
    assert names(route(BF16, 212, tsa(212))) == [region(NK, GATHER, "bevr_attn_bwd_q")]
    assert names(route(F32, 200, tsa(200))) == [region(NK)]
    monkeypatch.setenv("BEVR_SLAB", "1")
    assert names(route(BF16, 200, tsa(200))) == [region(NK, GATHER, "bevr_attn_bwd_q")]
    monkeypatch.delenv("BEVR_SLAB")

    monkeypatch.setenv("BEVR_KNORM", "0")
    r = route(BF16, 200, sca(200), source="kv_source")
    assert not r.kn2 and names(r) == [region(NK, GATHER, SLAB)]
    monkeypatch.setenv("BEVR_KNORM", "1")
    assert route(BF16, 200, sca(200), source="kv_source").kn2
    monkeypatch.delenv("BEVR_KNORM")

    monkeypatch.setenv("BEVR_MERGE_TAP", "0")
    r = tapped()
    assert r.merge == "merge_views" and names(r) == [region(1024, GATHER, SLAB), ("tap", 1024, NK) + TAP]
    monkeypatch.setenv("BEVR_MERGE_TAP", "1")
    assert tapped().merge == "merge_tap"
    monkeypatch.delenv("BEVR_MERGE_TAP")

    monkeypatch.setenv("BEVR_TAP", "0")
    assert not ops.tap_supported(BF16, 1)
    with pytest.raises(ValueError, match="tap_source needs kv_source or tap_pix"):
        tapped()
    # with dropout the unsupported tap segment is not an error: every key on the region kernels
    assert names(tapped(dropout=True, keys_in_tap_grid=_never)) == [("region", 0, NK) + TILE_DROP]
    monkeypatch.setenv("BEVR_TAP", "1")
    assert names(tapped()) == [region(1024, GATHER, SLAB), ("tap", 1024, NK) + TAP]
    monkeypatch.delenv("BEVR_TAP")

    # BEVR_TAP_X3: unset is TAP_X3_DEFAULT
    x3 = dict(cell_split=1024, tap_source="pinned", source="tap_pix")
    if ops.TAP_X3_DEFAULT == "0":
        with pytest.raises(ValueError, match="tap_source needs kv_source or tap_pix"):
            route(X3, 200, sca(200), **x3)
    else:
        assert route(X3, 200, sca(200), **x3).tap
    monkeypatch.setenv("BEVR_TAP_X3", "1")
    assert names(route(X3, 200, sca(200), **x3)) == [region(1024), ("tap", 1024, NK) + TAP]
    assert names(route(BF16, 200, sca(200), cell_split=1024, tap_source="pinned", source="kv_source")) \
        == [region(1024, GATHER, SLAB), ("tap", 1024, NK) + TAP]                   # the 16-bit route does not read it
    monkeypatch.setenv("BEVR_TAP_X3", "0")
    with pytest.raises(ValueError, match="tap_source needs kv_source or tap_pix"):
        route(X3, 200, sca(200), **x3)
    monkeypatch.delenv("BEVR_TAP_X3")

    monkeypatch.setenv("BEVR_FUSED_KV", "0")
    assert not ops.kv_source_supported(64, 2, 1, BF16)
    with pytest.raises(ValueError, match="kv_source needs a 16-bit operand mode"):
        route(BF16, 200, sca(200), source="kv_source")
    assert names(route(BF16, 200, sca(200), source="kv")) == [region(NK, GATHER, SLAB)]
    monkeypatch.setenv("BEVR_FUSED_KV", "1")
    assert route(BF16, 200, sca(200), source="kv_source").kn2
    monkeypatch.delenv("BEVR_FUSED_KV")

    # BEVR_CELL decides the static split (split_key_order), not a call's kernels
    import numpy as np
    ref = np.full((2, 4096, 2), -1.0)
    ref[:, :1024] = np.random.RandomState(0).rand(2, 1024, 2)
    assert ops.split_key_order(ref, 16, 127)[1] == 1024
    monkeypatch.setenv("BEVR_CELL", "0")
    assert ops.split_key_order(ref, 16, 127)[1] == 4096
    assert names(route(BF16, 200, sca(200), cell_split=1024)) == [region(1024, GATHER, SLAB), ("cell", 1024, NK) + CELL]
    monkeypatch.setenv("BEVR_CELL", "1")
    assert ops.split_key_order(ref, 16, 127)[1] == 1024


def test_route_refusals():
    with pytest.raises(ValueError, match=r"cell_split must lie in \[0, N\]"):
        route(BF16, 200, sca(200), cell_split=NK + 1)
    for prec in (F32, X3):
        with pytest.raises(ValueError, match="kv_source needs a 16-bit operand mode"):
            route(prec, 200, sca(200), source="kv_source")
    with pytest.raises(ValueError, match="kv_source needs a 16-bit operand mode"):
        route(BF16, 200, sca(200), source="kv_source", C=72)            # C % 16


def test_fused_source_adjoint_makes_no_copy_without_groups(monkeypatch):
    """ops._kv_source_adjoint is the grouped form for every G: at G == 1, on a contiguous map, the tensors handed to the
    sampler and to its scatter share their sources' storage (plain CPU tensors; the two launches replaced by stand-ins)."""
    seen = {}
    nb, Hi, Wi, Cc, Nk = 3, 5, 6, 16, 7
    feat, spos = torch.randn(nb, Hi, Wi, Cc), torch.rand(nb, Nk, 2)
    dkv, Wkv = torch.randn(nb, Nk, 2 * Cc), torch.randn(2 * Cc, Cc)
    samples, dmap = torch.randn(nb, Nk, Cc), torch.randn(nb, Hi, Wi, Cc)

    def sample(fg, pos):
        seen["fg"] = fg
        return samples

    def scatter(fg, pos, dxs, need_dfeat=True):
        seen["dxs"] = dxs
        return dmap, torch.zeros_like(pos)
    monkeypatch.setattr(ops._Sample, "sample", staticmethod(sample))
    monkeypatch.setattr(ops._Sample, "scatter", staticmethod(scatter))
    dfeat, dspos, dW, dbias = ops._kv_source_adjoint(dkv, feat, spos, Wkv, 1, True, True, True)
    assert seen["fg"].data_ptr() == feat.data_ptr() and seen["fg"].shape == feat.shape and seen["fg"].stride() == feat.stride()
    want_dxs = dkv.reshape(-1, 2 * Cc) @ Wkv
    assert torch.equal(seen["dxs"].reshape(want_dxs.shape), want_dxs) and seen["dxs"].is_contiguous()
    assert seen["dxs"].shape == (nb, Nk, Cc) and seen["dxs"]._base is not None          # a view of the product, no copy
    assert dfeat.data_ptr() == dmap.data_ptr() and dfeat.shape == feat.shape
    assert torch.equal(dW, torch.bmm(dkv.transpose(1, 2), samples).sum(0)) and torch.equal(dbias, dkv.reshape(-1, 2 * Cc).sum(0))
