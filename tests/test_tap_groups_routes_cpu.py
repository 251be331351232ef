"""The route of a pinned key segment with TWO channel groups (ops.attention_route, ops.tap_supported), without a GPU:
behind BEVR_TAP_GROUPS the segment names the two-group tap entry points; every other call, and every call with the
switch unset, keeps the route it had."""
import importlib.util
import os

import pytest

from bevrender_amd import _lib, ops

F32, X3, BF16, F16 = _lib.PREC_F32, _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16
TAP_G2 = ("bevr_attn_tap_g2_fwd", "bevr_attn_tap_g2_bwd_q", "bevr_attn_tap_g2_bwd_k")
NK, SPLIT = 4096, 1024

_spec = importlib.util.spec_from_file_location(
    "_routes_table", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_attention_routes_cpu.py"))
table = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(table)


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in table.SWITCHES + ("BEVR_TAP_GROUPS", "BEVR_TAP_X3_DROP", "BEVR_SCATTER_DROP", "BEVR_KV_WSPLIT"):
        monkeypatch.delenv(name, raising=False)


def record(prec, groups, S=200, **kw):
    """the route of a pinned-split SCA call as a comparable record: the AttnRoute, or the refusal's text"""
    kw = dict(dict(cell_split=SPLIT, tap_source="pinned", source="kv_source", C=64, heads=4), **kw)
    try:
        return ops.attention_route(prec, groups, S, 2 * S * 4 - 1, NK, **kw)
    except ValueError as e:
        return "ValueError: " + str(e)


def test_the_switch_is_off_by_default_and_read_by_tap_supported():
    assert ops.TAP_GROUPS_DEFAULT == "0"
    assert not ops.tap_supported(BF16, 2) and ops.tap_supported(BF16, 1)


def test_tap_supported_with_the_switch(monkeypatch):
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    assert ops.tap_supported(BF16, 2) and ops.tap_supported(F16, 2)
    assert not ops.tap_supported(BF16, 2, dropout=True)
    assert not ops.tap_supported(X3, 2) and not ops.tap_supported(F32, 2)
    assert not ops.tap_supported(BF16, 4) and not ops.tap_supported(BF16, 3)
    assert ops.tap_supported(BF16, 1) and ops.tap_supported(BF16, 1, dropout=True)      # one group: as it was
    monkeypatch.setenv("BEVR_TAP", "0")
    assert not ops.tap_supported(BF16, 2)
    monkeypatch.delenv("BEVR_TAP")
    monkeypatch.setenv("BEVR_TAP_GROUPS", "0")
    assert not ops.tap_supported(BF16, 2)


@pytest.mark.parametrize("prec", [BF16, F16])
@pytest.mark.parametrize("tap_source", [True, "pinned"])
def test_two_groups_with_the_switch_name_the_new_entry_points(prec, tap_source, monkeypatch):
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    for S, fwd, bwd_q in ((40, table.GATHER, table.SLAB), (200, table.GATHER, table.SLAB), (400, table.ROWS, "bevr_attn_bwd_q")):
        r = record(prec, 2, S, tap_source=tap_source)
        assert table.names(r) == [table.region(SPLIT, fwd, bwd_q), ("tap", SPLIT, NK) + TAP_G2], (S, r)
        # the fused merge_tap forms O = Rn Vpix for 12 taps only
        assert r.tap and r.n_core == SPLIT and r.split == SPLIT and r.merge == "merge_views" and r.kn2
    r = record(prec, 2, cell_split=0, tap_source=tap_source)
    assert table.names(r) == [("tap", 0, NK) + TAP_G2] and r.n_core == 0 and r.merge == "merge_views"
    # one group beside it: its own entry points and the fused merge, as before
    r = record(prec, 1, tap_source=tap_source)
    assert table.names(r)[-1] == ("tap", SPLIT, NK) + table.TAP and r.merge == "merge_tap"
    # the tap kernels' limit on the grid side holds for two groups too
    assert record(prec, 2, 449, tap_source=tap_source).startswith("ValueError: tap_source needs kv_source or tap_pix")


OTHER_CALLS = {
    "dropout": dict(prec=BF16, groups=2, dropout=True),
    "dropout_fp16": dict(prec=F16, groups=2, dropout=True),
    "split_bf16": dict(prec=X3, groups=2),
    "split_bf16_tap_pix": dict(prec=X3, groups=2, source="tap_pix"),
    "f32": dict(prec=F32, groups=2, source="kv"),
    "f32_fused": dict(prec=F32, groups=2),
    "four_groups": dict(prec=BF16, groups=4),
    "four_groups_fp16": dict(prec=F16, groups=4),
    "projected_rows": dict(prec=BF16, groups=2, source="kv"),
    "cell_split": dict(prec=BF16, groups=2, tap_source=False),
    "one_group": dict(prec=BF16, groups=1),
    "one_group_dropout": dict(prec=BF16, groups=1, dropout=True),
    "no_split": dict(prec=BF16, groups=2, cell_split=None, tap_source=False),
}


@pytest.mark.parametrize("case", list(OTHER_CALLS))
def test_every_other_call_keeps_its_route_with_the_switch_on(case, monkeypatch):
    kw = dict(OTHER_CALLS[case])
    prec, groups = kw.pop("prec"), kw.pop("groups")
    before = record(prec, groups, **kw)
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    assert record(prec, groups, **kw) == before, case
    assert "bevr_attn_tap_g2" not in repr(before)


def test_unset_or_zero_two_groups_are_refused_as_before(monkeypatch):
    unset = record(BF16, 2)
    assert unset.startswith("ValueError: tap_source needs kv_source or tap_pix")
    monkeypatch.setenv("BEVR_TAP_GROUPS", "0")
    assert record(BF16, 2) == unset
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    monkeypatch.setenv("BEVR_TAP", "0")
    assert record(BF16, 2) == unset


def test_every_row_of_the_route_table_is_unchanged_with_the_switch_on(monkeypatch):
    """tests/test_attention_routes_cpu.py's literals, run again under BEVR_TAP_GROUPS=1 (its one statement about two
    groups on the tap kernels -- a refusal inside test_tap_split -- is what the switch changes, and is not a table row)"""
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    for S, tbl, want in table.REGION_TABLE:
        for source in ("kv", "kv_source"):
            table.test_region_route_by_precision_side_and_table(S, tbl, want, source)
    table.test_one_row_band_up_to_224()
    for groups in (1, 2):
        for source in ("kv", "kv_source"):
            table.test_cell_split(groups, source)
            for cell_split in (None, 0, 1024, table.NK):
                table.test_dropout_without_tap_source_runs_every_key_on_the_region_dropout_kernels(groups, source, cell_split)
    table.test_cell_kernels_size_limits()
    table.test_dropout_with_pinned_keys_keeps_the_split_on_the_tap_kernels()
    table.test_the_checked_tap_contract_is_evaluated_once_and_only_where_it_syncs_today()
    table.test_route_refusals()
