"""The route of the split-bf16 slab backward in row bands, without a GPU: BEVR_SLAB_X3=2 (no new environment name -- the
census of tests/test_all_switches_routes_cpu.py stays what it is) moves the scattered keys' bwd_q of the split-bf16 mode
onto K.SLAB_BWD_Q_X3_ROWS where the one-band kernel does not reach, and nothing else: every other value of the switch,
every call with a keep mask and every other precision keep the route they had, field by field.

"The route they had" is ops.attention_route with ops.slab_x3_rows_supported answering False -- the one question the
function adds to it -- and, for every switch at "1", the literal table of tests/test_all_switches_routes_cpu.py."""
import pytest

from bevrender_amd import _lib, ops
from test_all_switches_routes_cpu import ALL_ON, DEFAULT_ON, GRID, OPT_IN, decided, point_id, table_width

F32, X3, BF16, F16 = _lib.PREC_F32, _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16
K = ops.K
NK, CS = 4096, 1024
KV, KV_SPLIT, PIX, SRC_TAP = ("kv", None, False), ("kv", CS, False), ("tap_pix", CS, "pinned"), ("kv_source", CS, "pinned")
SIDES = (40, 211, 212, 240, 400, 448)
VALUES = (None, "0", "1", "2")
# the switches around the one under test: defaults, every opt-in switch on, and the two that widen a slab route
AMBIENT = ({}, dict(ALL_ON), {"BEVR_SLAB": "2"}, {"BEVR_SLAB": "0"}, {"BEVR_SLAB_ROWS": "2"}, {"BEVR_SLAB_ROWS": "1"},
           {"BEVR_SLAB_ROWS": "2", "BEVR_SLAB": "2", "BEVR_GATHER_X3": "1"}, {"BEVR_SCATTER_DROP": "1"})


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in OPT_IN + DEFAULT_ON:
        monkeypatch.delenv(name, raising=False)


def set_env(monkeypatch, env, value):
    for name in OPT_IN + DEFAULT_ON:
        monkeypatch.delenv(name, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if value is None:
        monkeypatch.delenv("BEVR_SLAB_X3", raising=False)
    else:
        monkeypatch.setenv("BEVR_SLAB_X3", value)


def points():
    """precision x groups x S x width x mask, as tests/test_all_switches_routes_cpu.py enumerates them, on more sides"""
    return [dict(prec=prec, groups=g, S=S, width=w, mask=m) for prec in (F32, X3, BF16, F16) for g in (1, 2) for S in SIDES
            for w in ("wide", "narrow") for m in (False, True)]


def calls(p, env):
    """the calls the module makes for the point: projected rows without a split always; with one group also the split, and
    where the tap kernels take the mode the pinned split on them"""
    out = [KV]
    if p["groups"] == 1:
        out.append(KV_SPLIT)
    if ops.tap_supported(p["prec"], p["groups"], dropout=p["mask"]) and ops.tap_supported(p["prec"], p["groups"]):
        if p["prec"] == X3:
            out.append(PIX)
        elif ops.kv_source_supported(64, 2, p["groups"], p["prec"]):
            out.append(SRC_TAP)
    return out


def bwd_q(prec, S, Wt, mask=False, groups=1):
    r = ops.attention_route(prec, groups, S, Wt, NK, None, False, mask, "kv", 64, 2, None)
    return r.segments[0].bwd_q


WIDE = lambda S: 2 * S * 4 - 1          # noqa: E731  (SCA's table at depth 4)
NARROW = lambda S: 2 * S - 1            # noqa: E731  (TSA's)


def test_value_2_routes_the_tall_sides_onto_the_band_kernel(monkeypatch):
    assert K.SLAB_BWD_Q_X3_ROWS == "bevr_attn_slab_bwd_q_x3_rows" and K.SLAB_BWD_Q_X3_ROWS in ops._RUN
    assert ops._RUN[K.SLAB_BWD_Q_X3_ROWS] is ops._RUN[K.SLAB_BWD_Q_ROWS]
    set_env(monkeypatch, {}, "2")
    for g in (1, 2):
        for S in (212, 240, 400, 448):
            assert ops.slab_x3_rows_supported(X3, S, WIDE(S)) and ops.slab_x3_rows_supported(X3, S)
            assert bwd_q(X3, S, WIDE(S), groups=g) == K.SLAB_BWD_Q_X3_ROWS, S
            assert bwd_q(X3, S, NARROW(S), groups=g) == K.BWD_Q, S          # TSA's table: the query-tile kernel
            assert bwd_q(X3, S, WIDE(S), mask=True, groups=g) == K.BWD_Q_DROP, S
        for S in (2, 40, 211):          # the one-band kernel keeps what it reaches
            assert not ops.slab_x3_rows_supported(X3, S, WIDE(S))
            assert bwd_q(X3, S, WIDE(S), groups=g) == K.SLAB_BWD_Q_X3, S
            assert bwd_q(X3, S, NARROW(S), groups=g) == K.BWD_Q, S
    assert not ops.slab_x3_rows_supported(X3, 449, WIDE(449)) and bwd_q(X3, 480, WIDE(480)) == K.BWD_Q
    for prec in (F32, BF16, F16):
        assert not ops.slab_x3_rows_supported(prec, 240, WIDE(240))
    # BEVR_SLAB=2: every table width; BEVR_SLAB=0: no slab route at all
    set_env(monkeypatch, {"BEVR_SLAB": "2"}, "2")
    for S in (212, 400):
        assert bwd_q(X3, S, NARROW(S)) == K.SLAB_BWD_Q_X3_ROWS
    assert bwd_q(X3, 40, NARROW(40)) == K.SLAB_BWD_Q_X3
    set_env(monkeypatch, {"BEVR_SLAB": "0"}, "2")
    for S in (40, 240, 400):
        assert not ops.slab_x3_rows_supported(X3, S, WIDE(S)) and bwd_q(X3, S, WIDE(S)) == K.BWD_Q
    set_env(monkeypatch, {"BEVR_SLAB": "0", "BEVR_SLAB_ROWS": "2"}, "2")
    assert bwd_q(X3, 40, WIDE(40)) == K.BWD_Q
    # BEVR_SLAB_ROWS=2 on top: every S and every width on the band kernel, ahead of the one-band kernel
    set_env(monkeypatch, {"BEVR_SLAB_ROWS": "2"}, "2")
    for S in (2, 40, 211, 240, 448):
        for Wt in (WIDE(S), NARROW(S)):
            assert bwd_q(X3, S, Wt) == K.SLAB_BWD_Q_X3_ROWS, (S, Wt)
    assert bwd_q(X3, 449, WIDE(449)) == K.BWD_Q
    assert bwd_q(BF16, 40, WIDE(40)) == K.SLAB_BWD_Q_ROWS          # the 16-bit unit's own band kernel, as before
    # ... and without the value 2 that switch does nothing for the split mode
    set_env(monkeypatch, {"BEVR_SLAB_ROWS": "2"}, "1")
    assert bwd_q(X3, 40, WIDE(40)) == K.SLAB_BWD_Q_X3 and bwd_q(X3, 240, WIDE(240)) == K.BWD_Q
    set_env(monkeypatch, {"BEVR_SLAB_ROWS": "1"}, "2")          # BEVR_SLAB_ROWS=1 is the 16-bit modes' business
    assert bwd_q(X3, 40, WIDE(40)) == K.SLAB_BWD_Q_X3 and bwd_q(X3, 240, WIDE(240)) == K.SLAB_BWD_Q_X3_ROWS


def records(monkeypatch, env, value, stub):
    """{(point, call): route fields}; stub: ops.slab_x3_rows_supported answers False (the route before it existed)"""
    set_env(monkeypatch, env, value)
    out = {}
    with monkeypatch.context() as m:
        if stub:
            m.setattr(ops, "slab_x3_rows_supported", lambda *a, **k: False)
        for p in points():
            for call in calls(p, env):
                try:
                    out[point_id(p), call] = decided(p, call)
                except ValueError as e:          # a call the route refuses: refused alike
                    out[point_id(p), call] = str(e)
    return out


@pytest.mark.parametrize("env", AMBIENT, ids=["+".join(sorted(e)) or "defaults" if len(e) < 5 else "all_on" for e in AMBIENT])
def test_other_values_masks_and_precisions_keep_their_routes(env, monkeypatch):
    """BEVR_SLAB_X3 unset, 0 or 1: the whole table is the one before (the new function never says yes).  At 2: every
    record with a keep mask, in a 16-bit mode or in f32 is the one before, and a record that moves is a split-bf16
    record without a mask, moves in region.bwd_q alone, onto the new name, exactly where slab_x3_rows_supported says."""
    moved = 0
    for value in VALUES:
        before, now = records(monkeypatch, env, value, True), records(monkeypatch, env, value, False)
        assert before.keys() == now.keys() and len(now) >= 4 * 2 * len(SIDES) * 2 * 2
        set_env(monkeypatch, env, value)
        for key in now:
            pid, call = key
            x3_nomask = pid.startswith("bf16x3-") and pid.endswith("-nomask")
            if value != "2" or not x3_nomask:
                assert now[key] == before[key], (value, key)
                assert isinstance(now[key], str) or now[key]["region.bwd_q"] != K.SLAB_BWD_Q_X3_ROWS, (value, key)
                continue
            if isinstance(now[key], str):
                assert now[key] == before[key]
                continue
            S = int(pid.split("-S")[1].split("-")[0])
            yes = ops.slab_x3_rows_supported(X3, S, table_width(S, pid.split("-")[3]))
            differs = {k for k in now[key] if now[key][k] != before[key][k]}
            assert differs == ({"region.bwd_q"} if yes else set()), (key, differs)
            if yes:
                assert now[key]["region.bwd_q"] == K.SLAB_BWD_Q_X3_ROWS
                assert before[key]["region.bwd_q"] in (K.BWD_Q, K.SLAB_BWD_Q_X3), key
                moved += 1
    assert (moved > 0) == (env.get("BEVR_SLAB") != "0")


def test_every_switch_at_1_is_the_pinned_table(monkeypatch):
    """BEVR_SLAB_X3=1 with every other opt-in switch on: the literal table, where split-bf16 S = 240 keeps
    bevr_attn_bwd_q; at 2 the table's split-bf16 wide no-mask rows above 211 move, and only they"""
    for value in ("1", "2"):
        set_env(monkeypatch, ALL_ON, value)
        for p, want in GRID:
            got = decided(p, (want["source"], want["cell_split"], want["tap_source"]))
            moves = value == "2" and p["prec"] == X3 and not p["mask"] and p["S"] > 211 and p["width"] == "wide"
            if moves:
                assert want["region.bwd_q"] == K.BWD_Q
                want = dict(want, **{"region.bwd_q": K.SLAB_BWD_Q_X3_ROWS})
            assert got == want, (value, point_id(p))


def test_the_older_questions_keep_their_answers(monkeypatch):
    for value in VALUES:
        for env in AMBIENT:
            set_env(monkeypatch, env, value)
            for S in SIDES + (449,):
                for Wt in (WIDE(S), NARROW(S), None):
                    # the split mode's one-band answer: any value but 0, S <= 211, under BEVR_SLAB's rules
                    slab = env.get("BEVR_SLAB", "1")
                    on = value not in (None, "0") and S <= 211 and slab != "0"
                    wide = slab == "2" or Wt is None or Wt - 1 >= 4 * (S - 1)
                    assert ops.slab_supported(X3, S, Wt) == (on and wide), (value, env, S, Wt)
                    assert not ops.slab_rows_supported(X3, S, Wt) and not ops.slab_rows_supported(F32, S, Wt)
                    assert not ops.slab_x3_rows_supported(BF16, S, Wt) and not ops.slab_x3_rows_supported(F16, S, Wt)
    assert ops.SLAB_X3_DEFAULT == "0"
