"""BEVR_KV_WSPLIT (split hi + lo weights for the fused K | V source, bevr_kv_project_w2), without a GPU: the switch changes
one field of ops.attention_route's decision, `wsplit`, and only for kv_source calls -- over the argument grid of
tests/test_attention_routes_cpu.py --, and ops.kv_split_weights builds planes that reproduce the float weights."""
import dataclasses
import itertools

import pytest
import torch

from bevrender_amd import _lib, ops

F32, X3, BF16, F16 = _lib.PREC_F32, _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16
SWITCHES = ("BEVR_GATHER", "BEVR_SLAB", "BEVR_KNORM", "BEVR_MERGE_TAP", "BEVR_TAP", "BEVR_TAP_X3", "BEVR_FUSED_KV", "BEVR_CELL",
            "BEVR_KV_WSPLIT", "BEVR_SCATTER_DROP", "BEVR_GATHER_X3", "BEVR_SLAB_X3", "BEVR_SLAB_ROWS", "BEVR_TAP_X3_DROP")
NK = 4096


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def tsa(S):
    return 2 * S - 1


def sca(S):     # depth 4
    return 2 * S * 4 - 1


def grid():
    """(precision, S, Wt, keyword arguments) of every call shape tests/test_attention_routes_cpu.py routes: precision, BEV
    side, table width, split, tap_source, dropout, channel groups, source."""
    for prec, S, table, source, groups, split, tap, drop in itertools.product(
            (F32, X3, BF16, F16), (40, 200, 211, 212, 400, 448, 449), (tsa, sca), ("kv", "kv_source", "tap_pix"), (1, 2),
            (None, 0, 1024, NK), (False, True, "pinned"), (False, True)):
        kw = dict(source=source, groups=groups, cell_split=split, tap_source=tap, dropout=drop, C=64, heads=2,
                  keys_in_tap_grid=lambda s: True)
        yield prec, S, table(S), kw


def routes():
    """every call of the grid that attention_route accepts, as (key, route)"""
    out = {}
    for prec, S, Wt, kw in grid():
        try:
            r = ops.attention_route(prec, kw["groups"], S, Wt, NK, **{k: v for k, v in kw.items() if k != "groups"})
        except ValueError:
            continue
        key = (prec, S, Wt) + tuple((k, v) for k, v in sorted(kw.items()) if k != "keys_in_tap_grid")
        out[key] = (kw["source"], r)
    return out


def test_default_is_off_and_written_like_the_neighbouring_switches():
    assert ops.KV_WSPLIT_DEFAULT == "0" and not ops.kv_wsplit()
    assert "wsplit" in {f.name for f in dataclasses.fields(ops.AttnRoute)}
    assert ops.AttnRoute((), 0, None, False, "merge_views").wsplit is False        # a defaulted field


def test_switch_unset_no_route_splits_the_weights():
    got = routes()
    assert len(got) > 500 and any(src == "kv_source" for src, _ in got.values())
    assert all(r.wsplit is False for _, r in got.values())


@pytest.mark.parametrize("value", ["1", "0"])
def test_switch_changes_wsplit_of_kv_source_calls_and_nothing_else(value, monkeypatch):
    off = routes()
    monkeypatch.setenv("BEVR_KV_WSPLIT", value)
    assert ops.kv_wsplit() == (value == "1")
    on = routes()
    assert set(on) == set(off)                                       # the same calls are accepted and refused
    n_split = 0
    for key, (source, r) in on.items():
        assert r.wsplit == (value == "1" and source == "kv_source"), key
        assert dataclasses.replace(r, wsplit=False) == off[key][1], key
        n_split += r.wsplit
    assert (n_split > 100) == (value == "1")


def test_refused_modes_stay_refused(monkeypatch):
    monkeypatch.setenv("BEVR_KV_WSPLIT", "1")
    for prec in (F32, X3):
        with pytest.raises(ValueError, match="kv_source needs a 16-bit operand mode"):
            ops.attention_route(prec, 1, 200, sca(200), NK, source="kv_source", C=64, heads=2)
    monkeypatch.setenv("BEVR_FUSED_KV", "0")
    with pytest.raises(ValueError, match="kv_source needs a 16-bit operand mode"):
        ops.attention_route(BF16, 1, 200, sca(200), NK, source="kv_source", C=64, heads=2)


# hi + lo 2^-lo_exp against the float weights: hi carries p bits, the scaled residual p more (bf16 p = 8, fp16 p = 11,
# round to nearest: half an ulp each) -- 2^-16 / 2^-22 relative; the issue's bounds are 2^-16 and 2^-21
@pytest.mark.parametrize("prec,lo_exp,bound", [(BF16, 0, 2.0 ** -16), (F16, 11, 2.0 ** -21)])
@pytest.mark.parametrize("wscale", [1.0, 2.0 ** -7])
def test_kv_split_weights_reproduces_the_float_weights(prec, lo_exp, bound, wscale):
    C = 64
    W = torch.randn(2 * C, C, generator=torch.Generator().manual_seed(5)) / C ** 0.5 * wscale
    if wscale < 1:
        assert 5e-4 < W.abs().median().item() < 2e-3                 # |w| about 1e-3
    planes, e = ops.kv_split_weights(W, prec)
    ed = torch.bfloat16 if prec == BF16 else torch.float16
    assert e == lo_exp and planes.shape == (2, 2 * C, C) and planes.dtype == ed and planes.is_contiguous()
    assert torch.equal(planes[0], W.to(ed))
    assert torch.equal(planes[1], ((W - W.to(ed).float()) * 2.0 ** lo_exp).to(ed))
    back = planes[0].double() + planes[1].double() * 2.0 ** -lo_exp
    err, mag = (back - W.double()).abs(), W.double().abs()
    # per element -- down to where fp16's own grid ends: a scaled residual below 2^-14 is subnormal, spaced 2^-24, so
    # its rounding is up to 2^-25 2^-11 = 2^-36 absolute, which is 2^-21 relative for |w| >= 2^-15 (3e-5); the few
    # elements of a random matrix below that keep the absolute bound.  bf16 has float's exponents: every element.
    floor = 2.0 ** -15 if prec == F16 else 0.0
    big = mag >= floor
    rel = (err[big] / mag[big]).max().item()
    print(f"prec {prec} wscale {wscale}: max relative error {rel:.3e} (bound {bound:.3e}), {int((~big).sum())} tiny elements, "
          f"whole matrix {(err.norm() / mag.norm()).item():.3e}")
    assert big.float().mean().item() > 0.9 and rel <= bound
    assert (~big).sum() == 0 or err[~big].max().item() <= 2.0 ** -36
    assert (err.norm() / mag.norm()).item() <= bound
    # the rounded weights alone are 2^8 (bf16) / 2^10 (fp16) times further away: the error the split removes
    assert ((planes[0].double() - W.double()).abs() / W.double().abs()).max().item() > 64 * bound


def test_kv_split_weights_refuses_the_float_layouts_and_keeps_its_input():
    W = torch.randn(32, 16, requires_grad=True)
    for prec in (F32, X3):
        with pytest.raises(ValueError):
            ops.kv_split_weights(W, prec)
    planes, _ = ops.kv_split_weights(W, BF16)
    assert not planes.requires_grad
