"""Every opt-in switch on together, without a GPU: the route ops.attention_route decides for the calls
SCADeformableAttention.forward makes, as a table of literals over precision, channel groups, BEV side, table width and
keep mask; which fields of that route each switch owns (the route with one switch taken away differs from the all-on
route in exactly those); and a census of the package's BEVR_* environment reads, so that a switch added later fails here
until it is classified -- and, if it is an opt-in switch, joins ALL_ON and with it the combined tests
(tests/test_gpu_all_switches.py)."""
import os
import re

import pytest

from bevrender_amd import _lib, ops

F32, X3, BF16, F16 = _lib.PREC_F32, _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16
NAME = {F32: "f32", X3: "bf16x3", BF16: "bf16", F16: "f16"}

# ---- the three classes of switches ------------------------------------------------------------------------------------
# opt-in: new kernel families, off until the pinned route table changes with them
OPT_IN = ("BEVR_TAP_X3", "BEVR_TAP_X3_DROP", "BEVR_GATHER_X3", "BEVR_SLAB_X3", "BEVR_SCATTER_DROP", "BEVR_SLAB_ROWS",
          "BEVR_TAP_GROUPS", "BEVR_KV_WSPLIT")
# default-on A/B switches: "0" is the plain route the A/B timings compare against
DEFAULT_ON = ("BEVR_GATHER", "BEVR_SLAB", "BEVR_KNORM", "BEVR_MERGE_TAP", "BEVR_TAP", "BEVR_FUSED_KV", "BEVR_CELL",
              "BEVR_BWDK_LIST", "BEVR_FUSED_MLP")
# tuning constants: numbers, not routes (BEVR_GRAM_WAVES: the correlation kernel's waves per workgroup, csrc/corr.hip)
TUNING = ("BEVR_KD_LEAF", "BEVR_CELL_MIN", "BEVR_CELL_TAIL", "BEVR_GRAM_WAVES")
ALL_ON = {name: "1" for name in OPT_IN}
FLOOR = {name: "0" for name in DEFAULT_ON}


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in OPT_IN + DEFAULT_ON:
        monkeypatch.delenv(name, raising=False)


def set_switches(monkeypatch, env, without=None):
    for name in OPT_IN + DEFAULT_ON:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        if name != without:
            monkeypatch.setenv(name, value)


# ---- the table ----------------------------------------------------------------------------------------------------------
NK, CS = 4096, 1024         # keys; the projector's split: keys [CS, NK) are pinned to pixel (0, 0)
C, HEADS = 64, 2
A = "bevr_attn_"
TILE = (A + "fwd", A + "bwd_q", A + "bwd_k")
TILE_DROP = (A + "fwd_dropout", A + "bwd_q_dropout", A + "bwd_k_dropout")
CELL = ("cell", CS, NK, A + "cell_fwd", A + "cell_bwd_q", A + "cell_bwd_k")
TAP = ("tap", CS, NK, A + "tap_fwd", A + "tap_bwd_q", A + "tap_bwd_k")
TAP_DROP = ("tap", CS, NK, A + "tap_fwd_dropout", A + "tap_bwd_q_dropout", A + "tap_bwd_k_dropout")
TAP_X3_DROP = ("tap", CS, NK, A + "tap_fwd_x3_dropout", A + "tap_bwd_q_x3_dropout", A + "tap_bwd_k_x3_dropout")
TAP_G2 = ("tap", CS, NK, A + "tap_g2_fwd", A + "tap_g2_bwd_q", A + "tap_g2_bwd_k")
GATHER, ROWS, GATHER_X3, GATHER_DROP = A + "gather_fwd", A + "gather_fwd_rows", A + "gather_fwd_x3", A + "gather_fwd_dropout"
SLAB, SLAB_ROWS, SLAB_X3 = A + "slab_bwd_q", A + "slab_bwd_q_rows", A + "slab_bwd_q_x3"
SLAB_DROP, SLAB_X3_DROP = A + "slab_bwd_q_dropout", A + "slab_bwd_q_x3_dropout"
BWD_Q, BWD_K, BWD_Q_DROP, BWD_K_DROP = A + "bwd_q", A + "bwd_k", A + "bwd_q_dropout", A + "bwd_k_dropout"
WIDE, NARROW, ANY = ("wide",), ("narrow",), ("wide", "narrow")
H16 = (BF16, F16)

# the call as SCADeformableAttention.forward makes it with every opt-in switch on: (source, cell_split, tap_source)
#   16-bit modes: the fused K | V source; the pinned split on the tap kernels -- with two groups only without a mask
#   bf16x3: one group keeps the split beside projected rows (tap_pix), mask or not; two groups have no split
#   f32: projected rows; one group keeps the split for the cell kernels
SRC_TAP, SRC_NOSPLIT = ("kv_source", CS, "pinned"), ("kv_source", None, False)
PIX, KV_SPLIT, KV = ("tap_pix", CS, "pinned"), ("kv", CS, False), ("kv", None, False)

# precisions, groups, sides, widths, mask | call | region (n1, fwd, bwd_q, bwd_k), second segment | split, gather, merge, wsplit, kn2
TABLE = [
    # f32: no switch reaches it
    ((F32,), 1, (40,), ANY, False, KV_SPLIT, (CS,) + TILE, CELL, CS, None, "merge_views", False, False),
    ((F32,), 1, (240,), ANY, False, KV_SPLIT, (NK,) + TILE, None, CS, None, "merge_views", False, False),   # Sp > 224: no cell kernels
    ((F32,), 1, (40, 240), ANY, True, KV_SPLIT, (NK,) + TILE_DROP, None, NK, None, "merge_views", False, False),
    ((F32,), 2, (40, 240), ANY, False, KV, (NK,) + TILE, None, NK, None, "merge_views", False, False),
    ((F32,), 2, (40, 240), ANY, True, KV, (NK,) + TILE_DROP, None, NK, None, "merge_views", False, False),
    # bf16x3, one group: split gather forward, split slab bwd_q (S <= 211, wide), tap kernels on split operands
    ((X3,), 1, (40,), WIDE, False, PIX, (CS, GATHER_X3, SLAB_X3, BWD_K), TAP, CS, "whole", "merge_tap", False, False),
    ((X3,), 1, (40,), NARROW, False, PIX, (CS, GATHER_X3, BWD_Q, BWD_K), TAP, CS, "whole", "merge_tap", False, False),
    ((X3,), 1, (240,), ANY, False, PIX, (CS, GATHER_X3, BWD_Q, BWD_K), TAP, CS, "bands", "merge_tap", False, False),
    ((X3,), 1, (40,), WIDE, True, PIX, (CS, TILE_DROP[0], SLAB_X3_DROP, BWD_K_DROP), TAP_X3_DROP, CS, None, "merge_views", False, False),
    ((X3,), 1, (40,), NARROW, True, PIX, (CS,) + TILE_DROP, TAP_X3_DROP, CS, None, "merge_views", False, False),
    ((X3,), 1, (240,), ANY, True, PIX, (CS,) + TILE_DROP, TAP_X3_DROP, CS, None, "merge_views", False, False),
    # bf16x3, two groups: no tap kernels, no split
    ((X3,), 2, (40,), WIDE, False, KV, (NK, GATHER_X3, SLAB_X3, BWD_K), None, NK, "whole", "merge_views", False, False),
    ((X3,), 2, (40,), NARROW, False, KV, (NK, GATHER_X3, BWD_Q, BWD_K), None, NK, "whole", "merge_views", False, False),
    ((X3,), 2, (240,), ANY, False, KV, (NK, GATHER_X3, BWD_Q, BWD_K), None, NK, "bands", "merge_views", False, False),
    ((X3,), 2, (40,), WIDE, True, KV, (NK, TILE_DROP[0], SLAB_X3_DROP, BWD_K_DROP), None, NK, None, "merge_views", False, False),
    ((X3,), 2, (40,), NARROW, True, KV, (NK,) + TILE_DROP, None, NK, None, "merge_views", False, False),
    ((X3,), 2, (240,), ANY, True, KV, (NK,) + TILE_DROP, None, NK, None, "merge_views", False, False),
    # 16-bit modes, one group
    (H16, 1, (40,), WIDE, False, SRC_TAP, (CS, GATHER, SLAB, BWD_K), TAP, CS, "whole", "merge_tap", True, True),
    (H16, 1, (40,), NARROW, False, SRC_TAP, (CS, GATHER, BWD_Q, BWD_K), TAP, CS, "whole", "merge_tap", True, True),
    (H16, 1, (240, 448), WIDE, False, SRC_TAP, (CS, ROWS, SLAB_ROWS, BWD_K), TAP, CS, "bands", "merge_tap", True, True),
    (H16, 1, (240, 448), NARROW, False, SRC_TAP, (CS, ROWS, BWD_Q, BWD_K), TAP, CS, "bands", "merge_tap", True, True),
    (H16, 1, (40,), WIDE, True, SRC_TAP, (CS, GATHER_DROP, SLAB_DROP, BWD_K_DROP), TAP_DROP, CS, "whole", "merge_views", True, True),
    (H16, 1, (40,), NARROW, True, SRC_TAP, (CS, GATHER_DROP, BWD_Q_DROP, BWD_K_DROP), TAP_DROP, CS, "whole", "merge_views", True, True),
    (H16, 1, (240, 448), ANY, True, SRC_TAP, (CS, GATHER_DROP, BWD_Q_DROP, BWD_K_DROP), TAP_DROP, CS, "bands", "merge_views", True, True),
    # 16-bit modes, two groups: the two-group tap kernels without a mask; with one the split is dropped
    (H16, 2, (40,), WIDE, False, SRC_TAP, (CS, GATHER, SLAB, BWD_K), TAP_G2, CS, "whole", "merge_views", True, True),
    (H16, 2, (40,), NARROW, False, SRC_TAP, (CS, GATHER, BWD_Q, BWD_K), TAP_G2, CS, "whole", "merge_views", True, True),
    (H16, 2, (240, 448), WIDE, False, SRC_TAP, (CS, ROWS, SLAB_ROWS, BWD_K), TAP_G2, CS, "bands", "merge_views", True, True),
    (H16, 2, (240, 448), NARROW, False, SRC_TAP, (CS, ROWS, BWD_Q, BWD_K), TAP_G2, CS, "bands", "merge_views", True, True),
    (H16, 2, (40,), WIDE, True, SRC_NOSPLIT, (NK, GATHER_DROP, SLAB_DROP, BWD_K_DROP), None, NK, "whole", "merge_views", True, True),
    (H16, 2, (40,), NARROW, True, SRC_NOSPLIT, (NK, GATHER_DROP, BWD_Q_DROP, BWD_K_DROP), None, NK, "whole", "merge_views", True, True),
    (H16, 2, (240, 448), ANY, True, SRC_NOSPLIT, (NK, GATHER_DROP, BWD_Q_DROP, BWD_K_DROP), None, NK, "bands", "merge_views", True, True),
]

# the call with ONE switch taken away, where it is not the all-on call: what SCADeformableAttention.forward does without
# the tap kernels of the mode (ops.tap_supported is False there: projected rows of every key; one group keeps the split
# for the cell kernels, two groups drop it)
CALL_WITHOUT = {
    "BEVR_TAP_X3": lambda p: KV_SPLIT if p["prec"] == X3 and p["groups"] == 1 else None,
    "BEVR_TAP_X3_DROP": lambda p: KV_SPLIT if p["prec"] == X3 and p["groups"] == 1 and p["mask"] else None,
    "BEVR_TAP_GROUPS": lambda p: SRC_NOSPLIT if p["prec"] in H16 and p["groups"] == 2 else None,
}


def grid():
    points = []
    for precs, groups, sides, widths, mask, call, region, second, split, gather, merge, wsplit, kn2 in TABLE:
        for prec in precs:
            for S in sides:
                for width in widths:
                    point = dict(prec=prec, groups=groups, S=S, width=width, mask=mask)
                    want = dict(source=call[0], cell_split=call[1], tap_source=call[2], second=second, split=split,
                                gather=gather, merge=merge, wsplit=wsplit, kn2=kn2)
                    want.update(zip(("region.n1", "region.fwd", "region.bwd_q", "region.bwd_k"), region))
                    points.append((point, want))
    return points


GRID = grid()


def point_id(p):
    return f"{NAME[p['prec']]}-g{p['groups']}-S{p['S']}-{p['width']}-{'mask' if p['mask'] else 'nomask'}"


def table_width(S, width):      # SCA's table at depth 4, or one of TSA's width: Wt - 1 >= 4 (S - 1) or not
    return 2 * S * 4 - 1 if width == "wide" else 2 * S - 1


def _never(split):
    raise AssertionError("a pinned split is a promise: the route must not look at the keys")


def decided(p, call):
    """the fields of ops.attention_route's answer for grid point p and the call (source, cell_split, tap_source)"""
    source, cell_split, tap_source = call
    r = ops.attention_route(p["prec"], p["groups"], p["S"], table_width(p["S"], p["width"]), NK, cell_split, tap_source,
                            p["mask"], source, C, HEADS, _never)
    segs = [(s.kind, s.n0, s.n1, s.fwd, s.bwd_q, s.bwd_k) for s in r.segments]
    assert 1 <= len(segs) <= 2 and segs[0][:2] == ("region", 0) and segs[-1][2] == NK, segs
    got = dict(source=source, cell_split=cell_split, tap_source=tap_source, second=segs[1] if len(segs) == 2 else None,
               split=r.split, gather=r.gather, merge=r.merge, wsplit=r.wsplit, kn2=r.kn2)
    got.update(zip(("region.n1", "region.fwd", "region.bwd_q", "region.bwd_k"), segs[0][2:]))
    if len(segs) == 2:
        assert segs[1][1] == segs[0][2], segs
    assert r.tap == (got["second"] is not None and got["second"][0] == "tap")
    assert r.n_core == (CS if r.tap else NK)
    return got


def test_the_grid_is_the_one_the_table_was_written_for():
    """precision in all four modes x groups {1, 2} x S {40, 240} (+ 448 in the 16-bit modes) x {wide, narrow} x {mask,
    none}, each point once"""
    want = {(prec, g, S, w, m) for prec in (F32, X3, BF16, F16) for g in (1, 2)
            for S in ((40, 240, 448) if prec in H16 else (40, 240)) for w in ANY for m in (False, True)}
    have = [(p["prec"], p["groups"], p["S"], p["width"], p["mask"]) for p, _ in GRID]
    assert len(have) == len(set(have)) == 80 and set(have) == want


@pytest.mark.parametrize("p,want", GRID, ids=[point_id(p) for p, _ in GRID])
def test_all_on_route(p, want, monkeypatch):
    set_switches(monkeypatch, ALL_ON)
    wide = table_width(p["S"], p["width"]) - 1 >= 4 * (p["S"] - 1)
    assert wide == (p["width"] == "wide")
    got = decided(p, (want["source"], want["cell_split"], want["tap_source"]))
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}


def test_f32_is_the_default_route(monkeypatch):
    """no opt-in switch reaches the exact mode: its rows with every switch unset"""
    for p, want in GRID:
        if p["prec"] == F32:
            assert decided(p, (want["source"], want["cell_split"], want["tap_source"])) == want, point_id(p)


# ---- ownership ----------------------------------------------------------------------------------------------------------
# switch -> [(condition on the grid point, the fields that differ without the switch)]: the route under ALL_ON - {switch}
# differs from the route under ALL_ON in exactly the union of the fields whose condition holds (nothing where none does)
def _x3(p):
    return p["prec"] == X3


def _h16(p):
    return p["prec"] in H16


def _one_band_slab(p):      # slab_supported's limits
    return p["S"] <= 211 and p["width"] == "wide"


OWNS = {
    # the tap segment's existence and the source; the keys it gives back go to the cell kernels (S = 40), or join the
    # region segment (f32-sized operands past Sp = 224; any call with a mask, which also forgets the split)
    "BEVR_TAP_X3": [(lambda p: _x3(p) and p["groups"] == 1, {"source", "tap_source", "second"}),
                    (lambda p: _x3(p) and p["groups"] == 1 and not p["mask"], {"merge"}),
                    (lambda p: _x3(p) and p["groups"] == 1 and not p["mask"] and p["S"] == 240, {"region.n1"}),
                    (lambda p: _x3(p) and p["groups"] == 1 and p["mask"], {"region.n1", "split"})],
    "BEVR_TAP_X3_DROP": [(lambda p: _x3(p) and p["groups"] == 1 and p["mask"],
                          {"source", "tap_source", "second", "region.n1", "split"})],
    "BEVR_GATHER_X3": [(lambda p: _x3(p) and not p["mask"], {"region.fwd", "gather"})],
    "BEVR_SLAB_X3": [(lambda p: _x3(p) and _one_band_slab(p), {"region.bwd_q"})],
    # with a mask: the gather forward (and with it the K norm the projection emits for it) in the 16-bit modes, the slab
    # bwd_q in those and in bf16x3
    "BEVR_SCATTER_DROP": [(lambda p: _h16(p) and p["mask"], {"region.fwd", "gather", "kn2"}),
                          (lambda p: (_h16(p) or _x3(p)) and p["mask"] and _one_band_slab(p), {"region.bwd_q"})],
    "BEVR_SLAB_ROWS": [(lambda p: _h16(p) and p["S"] > 211 and p["width"] == "wide" and not p["mask"], {"region.bwd_q"})],
    "BEVR_TAP_GROUPS": [(lambda p: _h16(p) and p["groups"] == 2 and not p["mask"],
                         {"cell_split", "tap_source", "second", "region.n1", "split"})],
    "BEVR_KV_WSPLIT": [(_h16, {"wsplit"})],
}


def test_every_opt_in_switch_has_an_ownership_rule():
    assert set(OWNS) == set(OPT_IN) == set(ALL_ON)


@pytest.mark.parametrize("switch", OPT_IN)
def test_a_switch_moves_the_fields_it_owns_and_no_others(switch, monkeypatch):
    moved_somewhere = False
    for p, want in GRID:
        set_switches(monkeypatch, ALL_ON, without=switch)
        call = CALL_WITHOUT.get(switch, lambda p: None)(p) or (want["source"], want["cell_split"], want["tap_source"])
        got = decided(p, call)
        differs = {k for k in want if got[k] != want[k]}
        owned = set().union(*[fields for cond, fields in OWNS[switch] if cond(p)])
        assert differs == owned, (switch, point_id(p), sorted(differs), sorted(owned))
        moved_somewhere |= bool(differs)
    assert moved_somewhere, f"{switch} decides nothing on this grid"


def test_the_call_without_a_tap_switch_is_the_modules(monkeypatch):
    """CALL_WITHOUT against what SCADeformableAttention.forward asks ops for: tap_supported decides `pinned`, and with two
    groups whether the split is kept at all"""
    for switch, fn in CALL_WITHOUT.items():
        for p, want in GRID:
            for env_without in (None, switch):
                set_switches(monkeypatch, ALL_ON, without=env_without)
                call = (env_without and fn(p)) or (want["source"], want["cell_split"], want["tap_source"])
                pinned = ops.tap_supported(p["prec"], p["groups"])
                keeps = p["groups"] == 1 or (pinned and ops.tap_supported(p["prec"], p["groups"], dropout=p["mask"]))
                assert (call[1] is not None) == keeps, (switch, point_id(p))
                tap = pinned and keeps and call[0] != "kv"
                assert (call[2] == "pinned") == tap, (switch, point_id(p))
                if p["prec"] == X3 and p["groups"] == 1:
                    assert (call[0] == "tap_pix") == ops.tap_supported(X3, 1, dropout=p["mask"]), (switch, point_id(p))


# ---- the floor ------------------------------------------------------------------------------------------------------------
def test_floor_is_the_query_tile_kernels_alone(monkeypatch):
    """every default-on A/B switch at "0", the opt-in ones unset: projected rows, no split, the query-tile kernels"""
    set_switches(monkeypatch, FLOOR)
    for p, _ in GRID:
        assert not ops.kv_source_supported(C, HEADS, p["groups"], p["prec"]) and not ops.tap_supported(p["prec"], p["groups"])
        assert not ops.gather_supported(p["prec"], p["S"]) and not ops.slab_supported(p["prec"], p["S"], table_width(p["S"], p["width"]))
        got = decided(p, KV)
        tile = TILE_DROP if p["mask"] else TILE
        assert (got["region.n1"], got["region.fwd"], got["region.bwd_q"], got["region.bwd_k"]) == (NK,) + tile, point_id(p)
        assert got["second"] is None and got["gather"] is None and not got["kn2"] and not got["wsplit"]
        assert got["merge"] == "merge_views"
    assert not ops.bwd_k_list()


# ---- census ---------------------------------------------------------------------------------------------------------------
PKG = os.path.dirname(os.path.abspath(ops.__file__))
PY_READ = re.compile(r"""os\.(?:environ\.get\(|environ\[|getenv\()\s*["'](BEVR_[A-Z0-9_]+)["']""")
C_READ = re.compile(r"""getenv\s*\(\s*"(BEVR_[A-Z0-9_]+)"\s*\)""")


def _scan(ext, pattern):
    found = {}
    for top, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(ext):
                with open(os.path.join(top, f), encoding="utf-8", errors="replace") as fh:
                    for name in pattern.findall(fh.read()):
                        found.setdefault(name, set()).add(os.path.relpath(os.path.join(top, f), PKG))
    return found


def test_census_of_environment_switches():
    """every BEVR_* name the package reads (Python: os.environ / os.getenv; csrc: getenv) is in exactly one class"""
    found = _scan(".py", PY_READ)
    for ext in (".hip", ".h", ".cpp", ".c"):
        for name, where in _scan(ext, C_READ).items():
            found.setdefault(name, set()).update(where)
    classes = OPT_IN + DEFAULT_ON + TUNING
    assert len(classes) == len(set(classes)), "a name in two classes"
    unlisted = {n: sorted(w) for n, w in found.items() if n not in classes}
    assert not unlisted, f"classify these and, if opt-in, add them to the combined tests: {unlisted}"
    stale = sorted(set(classes) - set(found))
    assert not stale, f"listed but read nowhere: {stale}"
    assert len(OPT_IN) == 8 and len(DEFAULT_ON) == 9
    # the scan sees the reads it is meant to see
    assert "ops.py" in found["BEVR_KV_WSPLIT"] and os.path.join("model", "SCA.py") in found["BEVR_CELL_MIN"]
    assert os.path.join("csrc", "corr.hip") in found["BEVR_GRAM_WAVES"]


def test_opt_in_defaults_are_off():
    """no default changes with these tests: unset, every opt-in switch reads as off"""
    assert (ops.TAP_X3_DEFAULT, ops.TAP_X3_DROP_DEFAULT, ops.GATHER_X3_DEFAULT, ops.SLAB_X3_DEFAULT, ops.SCATTER_DROP_DEFAULT,
            ops.TAP_GROUPS_DEFAULT, ops.KV_WSPLIT_DEFAULT) == ("0",) * 7
    assert not ops.slab_rows_supported(BF16, 240, 2 * 240 * 4 - 1)
    assert not ops.tap_supported(X3, 1) and not ops.tap_supported(BF16, 2) and not ops.kv_wsplit() and not ops.scatter_drop()
    assert not ops.gather_supported(X3, 40) and not ops.slab_supported(X3, 40, 2 * 40 * 4 - 1)
