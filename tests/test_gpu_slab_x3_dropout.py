"""Attention dropout on the split-bf16 slab bwd_q (csrc/attn_slab_bwd_q_x3_drop.hip, bevr_attn_slab_bwd_q_x3_dropout, behind
BEVR_SLAB_X3=1 together with BEVR_SCATTER_DROP=1): the scattered keys of a bf16x3 call with a keep mask on the kernel they
take without one.

Every reference is float64 with the host twin of the mask (ops.dropout_keep_mask through drop_mult), p = 0.3 and a fixed
seed unless a test says otherwise.  The limits are the mode's masked route's own (tests/test_gpu_dropout.py):
GRAD_LIM[PREC_BF16X3] = 5e-4 of tests/test_gpu_ops.py for dQ and d(table), TOL[PREC_BF16X3] for the output.

In every test the PARENT's route (BEVR_SCATTER_DROP unset, same seed: bevr_attn_bwd_q_dropout) runs too and is asserted
first, with a message of its own -- if it misses a limit the inputs are at fault -- and the new route's dQ and d(table)
are held to the parent's at the same limit.  Both routes' errors are printed before anything is asserted (-s).  Which
entry points ran is read off a recorder around ops._launch: the new name exactly once on the new route and never on the
parent's, bevr_attn_bwd_q_dropout the other way round.  The recorded run is profiles/r21_slab_x3_dropout.txt, section 3."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bevrender_amd import _lib, ops
from oracle import bevrender_oracle as O
from test_gpu_dropout import STRESS_P, _oracle_core_drop, drop_mult
from test_gpu_fullsize import check_dpos, kink_distance
from test_gpu_gather import _problem as gather_problem
from test_gpu_ops import CORE_CFGS, GRAD_LIM, TOL, _core_problem, rel_err
from test_gpu_random_sweep_routes import OUT_LIM, POS_LIM, UNIT, gradient_terms
from test_gpu_scatter_dropout import SLAB_CFGS, _capture_bwd_q, _far_rows
from test_gpu_slab import CASES as SLAB_CASES, _problem as slab_problem
from test_gpu_tap import _tap_problem
from test_gpu_tap_dropout import _oracle_chain_drop
from test_gpu_tap_x3 import check_keys, pos_kink_distance

pytestmark = pytest.mark.gpu
DEV = "cuda"
X3 = _lib.PREC_BF16X3
LIM = GRAD_LIM[X3]
P_DROP = 0.3
NEW = "bevr_attn_slab_bwd_q_x3_dropout"
NEW_PREP = "bevr_attn_slab_x3_drop_prep"
FWD_DROP, BWD_Q_DROP, BWD_K_DROP = "bevr_attn_fwd_dropout", "bevr_attn_bwd_q_dropout", "bevr_attn_bwd_k_dropout"
TAP_X3_DROP = ("bevr_attn_tap_fwd_x3_dropout", "bevr_attn_tap_bwd_q_x3_dropout", "bevr_attn_tap_bwd_k_x3_dropout")
SWITCHES = ("BEVR_GATHER", "BEVR_SLAB", "BEVR_SLAB_ROWS", "BEVR_GATHER_X3", "BEVR_SLAB_X3", "BEVR_SCATTER_DROP", "BEVR_TAP_X3",
            "BEVR_TAP_X3_DROP")
NAMES5 = ["query", "k", "v", "pos", "table"]


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


class Recorder:
    """Around ops._launch: the entry points in the order they ran."""

    def __init__(self):
        self.names, self.orig = [], ops._launch

    def __call__(self, entry, *a, **kw):
        self.names.append(entry)
        return self.orig(entry, *a, **kw)


def on_route(monkeypatch, new, fn, slab2=False, taps=False, n_bwd_q=1):
    """fn() with BEVR_SLAB_X3=1 on both routes and BEVR_SCATTER_DROP=1 on the new one alone (slab2: BEVR_SLAB=2, the slab
    kernel for every table width; taps: the split-mode tap kernels and their mask), the launches recorded and counted."""
    rec = Recorder()
    with monkeypatch.context() as m:
        m.setenv("BEVR_SLAB_X3", "1")
        if new:
            m.setenv("BEVR_SCATTER_DROP", "1")
        if slab2:
            m.setenv("BEVR_SLAB", "2")
        if taps:
            m.setenv("BEVR_TAP_X3", "1")
            m.setenv("BEVR_TAP_X3_DROP", "1")
        m.setattr(ops, "_launch", rec)
        res = fn()
        torch.cuda.synchronize()
    assert rec.names.count(NEW) == (n_bwd_q if new else 0), rec.names
    assert rec.names.count(NEW_PREP) == (n_bwd_q if new else 0), rec.names
    assert rec.names.count(BWD_Q_DROP) == (0 if new else n_bwd_q), rec.names
    assert not any(n.startswith(("bevr_attn_slab", "bevr_attn_gather")) and n not in (NEW, NEW_PREP) for n in rec.names), rec.names
    assert FWD_DROP in rec.names and BWD_K_DROP in rec.names and "bevr_attn_bwd_q" not in rec.names, rec.names
    return res, rec.names


def core5(ins, h, g, V, drop, cot):
    """ops.attention_core on (query, k, v, pos, table), forward and backward: (out, [five gradients]) in float64 on the host"""
    dev = [t.clone().to(DEV).requires_grad_(True) for t in ins]
    out = ops.attention_core(*dev, heads=h, groups=g, views=V, precision=X3, attn_drop=drop)
    out.backward(cot.float().to(DEV))
    return out.detach().cpu().double(), [t.grad.cpu().double() for t in dev]


def oracle5(ins, h, g, V, keep, cot):
    cpu = [t.clone().double().requires_grad_(True) for t in ins]
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    want = _oracle_core_drop(*cpu, h, g, V, keep)
    want.backward(cot.double())
    return want.detach(), [t.grad for t in cpu]


def hold_both(tag, new, parent, want, kinds=("query", "table")):
    """new, parent, want: {name: gradient}.  Prints both routes' errors, asserts the parent's route first, then the new one
    against float64 and against the parent, all at GRAD_LIM[PREC_BF16X3]."""
    e1 = {k: rel_err(new[k], want[k]) for k in kinds}
    e0 = {k: rel_err(parent[k], want[k]) for k in kinds}
    ab = {k: rel_err(new[k], parent[k]) for k in kinds}
    print(f"\n[slab x3 dropout {tag}] new route " + "  ".join(f"{k} {v:.3e}" for k, v in e1.items()) + " | parent route " +
          "  ".join(f"{k} {v:.3e}" for k, v in e0.items()) + " | new against parent " +
          "  ".join(f"{k} {v:.3e}" for k, v in ab.items()) + f" | limit {LIM:.1e}")
    for k in kinds:
        assert e0[k] < LIM, f"{tag}: the PARENT route misses the limit on these inputs: {k} {e0[k]:.3e}"
    for k in kinds:
        assert torch.isfinite(new[k]).all(), f"{tag}: {k} not finite"
        assert e1[k] < LIM, f"{tag}: {k} {e1[k]:.3e}"
        assert ab[k] < LIM, f"{tag}: {k} against the parent route {ab[k]:.3e}"
    return e1, e0


# ---- 1. the entry point on the operands of a call's backward ------------------------------------------------------------
@pytest.mark.parametrize("name", list(SLAB_CFGS))
def test_entry_point_on_a_calls_backward_operands(name, monkeypatch):
    """bevr_attn_slab_bwd_q_x3_dropout beside bevr_attn_bwd_q_dropout on the same Q, dO, LSE, delta and scales: two problems of
    two heads, 700 keys with random b over an SCA-wide table (runs longer than one emission, the sorted order far from the
    identity, more than three 15-column slabs), keys whose rows leave the slab window (the clamped body).  What each
    launch adds into the zeroed dQ, and the call's gradients against float64."""
    B, V, Cc, h, S, D, N = SLAB_CFGS[name]
    Wt = 2 * S * D - 1
    seed = 0x51ab + S
    ins = gather_problem(B, V, Cc, h, S, D, N, 300 + S, _far_rows)
    a, b = ops.key_coords(ins[3], S, Wt, N)
    far = (a.floor() + 10 < 0) | (a.floor() > S - 1 + 8)
    assert far.any() and not far.all(), "keys whose rows leave the slab window, beside keys inside it"
    assert (b.argsort(1) != torch.arange(N)).float().mean() > 0.9, "the sorted order is far from the identity"
    assert (b.amax() - b.amin()).item() > 3 * 15, "more than three slabs of 15 columns"
    monkeypatch.setenv("BEVR_SLAB_X3", "1")
    assert ops.slab_supported(X3, S, Wt), "an SCA-wide table: no BEVR_SLAB=2"
    monkeypatch.delenv("BEVR_SLAB_X3")
    cot = torch.randn(B * V, S * S, Cc, generator=torch.Generator().manual_seed(4))
    store, res = {}, {}
    for new in (True, False):
        with monkeypatch.context() as m:
            _capture_bwd_q(m, NEW if new else BWD_Q_DROP, store)
            res[new], _ = on_route(m, new, lambda: core5(ins, h, 1, V, (P_DROP, seed), cot))
    keep = drop_mult(seed, P_DROP, B * V * h, S, N)
    want_out, want = oracle5(ins, h, 1, V, keep, cot)
    (out1, g1), (out0, g0) = res[True], res[False]
    dq_s, dq_t = store[NEW][0].double(), store[BWD_Q_DROP][0].double()
    e_launch = rel_err(dq_s, dq_t)
    print(f"\n[slab x3 dropout {name}] the launch's dQ against bevr_attn_bwd_q_dropout's {e_launch:.3e}; out "
          f"{rel_err(out1, want_out):.3e}")
    hold_both(name, dict(query=g1[0], table=g1[4]), dict(query=g0[0], table=g0[4]), dict(query=want[0], table=want[4]))
    assert e_launch < LIM, e_launch
    assert torch.equal(out1, out0), "the two routes share one forward"
    np.testing.assert_allclose(out1.numpy(), want_out.numpy(), **TOL[X3])
    # the key side: the same bwd_k launches (float atomics in the position gradient: equal up to their order)
    assert rel_err(g1[1], g0[1]) < 1e-5 and rel_err(g1[2], g0[2]) < 1e-5 and rel_err(g1[3], g0[3]) < 1e-4
    assert dq_s.abs().max() > 0 and store[NEW][1].abs().max() > 0


# ---- 2. the shapes of tests/test_gpu_slab.py with a mask ------------------------------------------------------------------
MASK_CASES = {k: SLAB_CASES[k] for k in ("tsa_small", "ragged", "groups", "wide_table", "far_keys")}
# (the single-key case of that file has zero gradients under ANY mask -- a kept pair has D dP - delta = 0, a dropped one
# delta = 0 --: three keys instead of its special normalisation)
MASK_CASES["three_keys"] = (1, 1, 64, 2, 1, 9, 3, 2 * 9 * 5 - 1, {})


@functools.lru_cache(maxsize=None)
def mask_case(name):
    """inputs, seed, cotangent and the oracle's output and gradients of a case: computed once, left unchanged"""
    B, V, C, h, g, S, N, Wt, extra = MASK_CASES[name]
    query, kv, pos, table = slab_problem(B, V, C, h, g, S, N, Wt, seed=3 + S, **extra)
    ins = (query, kv[..., :C].contiguous(), kv[..., C:].contiguous(), pos, table)
    seed = 0x3d0 + S + N
    cot = torch.randn(B * V, S * S, C, generator=torch.Generator().manual_seed(77))
    keep = drop_mult(seed, P_DROP, B * V * h, S, N)
    return ins, seed, cot, oracle5(ins, h, g, V, keep, cot)


@pytest.mark.parametrize("name", list(MASK_CASES))
def test_slab_shapes_with_a_mask(name, monkeypatch):
    """S = 12 on a TSA-wide table, ragged S = 21 / N = 333 (partial emissions, padding keys), channel groups (h = 4, g = 2:
    the hash's problem-head against the key arrays' problem-group), a table two orders wider than a slab, keys far outside
    the table, three keys.  BEVR_SLAB=2: the narrow tables take the slab route too."""
    B, V, C, h, g, S, N, Wt, extra = MASK_CASES[name]
    ins, seed, cot, (want_out, want) = mask_case(name)
    (out1, g1), _ = on_route(monkeypatch, True, lambda: core5(ins, h, g, V, (P_DROP, seed), cot), slab2=True)
    (out0, g0), _ = on_route(monkeypatch, False, lambda: core5(ins, h, g, V, (P_DROP, seed), cot), slab2=True)
    hold_both(name, dict(query=g1[0], table=g1[4]), dict(query=g0[0], table=g0[4]), dict(query=want[0], table=want[4]))
    assert torch.equal(out1, out0), "the two routes share one forward"
    np.testing.assert_allclose(out1.numpy(), want_out.numpy(), **TOL[X3])
    assert rel_err(g1[1], g0[1]) < 1e-5 and rel_err(g1[2], g0[2]) < 1e-5 and rel_err(g1[3], g0[3]) < 1e-4
    assert g1[4].abs().sum() > 0 and g1[0].abs().sum() > 0


# ---- 3. ops.attention_core over CORE_CFGS -----------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CORE_CFGS, ids=[f"cfg{i}" for i in range(len(CORE_CFGS))])
def test_attention_core_matches_the_oracle_and_the_parent_route(cfg, monkeypatch):
    """CORE_CFGS at p = 0.3, both switches on, BEVR_SLAB=2: output (TOL) and every gradient (GRAD_LIM) against the oracle with
    the same mask; d(pos) by check_dpos's rule against the parent route's (the same bwd_k kernel on both); and the result
    without a mask lies more than 0.05 away from the masked oracle."""
    B, V, Cc, h, g, S, D, N = cfg
    seed = 0x5eed1234
    ins = _core_problem(B, V, Cc, h, g, S, D, N, seed=sum(cfg))
    keep = drop_mult(seed, P_DROP, B * V * h, S, N)
    cot = torch.randn(B * V, S * S, Cc, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    want_out, want = oracle5(ins, h, g, V, keep, cot)
    (out1, g1), _ = on_route(monkeypatch, True, lambda: core5(ins, h, g, V, (P_DROP, seed), cot), slab2=True)
    (out0, g0), _ = on_route(monkeypatch, False, lambda: core5(ins, h, g, V, (P_DROP, seed), cot), slab2=True)
    tag = f"core cfg {cfg}"
    print(f"\n[slab x3 dropout {tag}] out new {rel_err(out1, want_out):.3e} parent {rel_err(out0, want_out):.3e}")
    kinds = ("query", "k", "v", "table")
    pick = lambda gs: {n: gs[NAMES5.index(n)] for n in kinds}
    hold_both(tag, pick(g1), pick(g0), pick(want), kinds)
    np.testing.assert_allclose(out0.numpy(), want_out.numpy(), **TOL[X3])
    np.testing.assert_allclose(out1.numpy(), want_out.numpy(), **TOL[X3])
    check_dpos(g1[3], g0[3], ins[3], S, 2 * S * D - 1, LIM, tag + " d(pos) against the parent route")
    with torch.no_grad():
        plain = ops.attention_core(*[t.to(DEV) for t in ins], heads=h, groups=g, views=V, precision=X3)
    assert rel_err(plain.cpu().double(), want_out) > 0.05, "the mask changed nothing"


# ---- 4. one mask across the region and the tap halves ------------------------------------------------------------------
NAMES6 = ["query", "feat", "Wkv", "bkv", "pos", "table"]


def tap_route(ins, split, h, V, drop, cot):
    """the SCA module's split-mode branch: the scattered keys sampled and projected, the pinned ones attention_core's tap
    segment (tap_source=True: checked), one mask over all N keys"""
    gpu = [t.clone().to(DEV).requires_grad_(True) for t in ins]
    query, feat, Wkv, bkv, pos, table = gpu
    kv = F.linear(ops.sample_features(feat.permute(0, 3, 1, 2), pos[:, :split].contiguous(), 1), Wkv, bkv)
    out = ops.attention_core(query, None, None, pos, table, heads=h, groups=1, views=V, precision=X3, kv=kv,
                             cell_split=split, tap_source=True, tap_pix=(feat, Wkv, bkv), attn_drop=drop)
    out.backward(cot.float().to(DEV))
    return out.detach().cpu().double(), [t.grad.cpu().double() for t in gpu]


def test_region_and_tap_halves_share_one_mask(monkeypatch):
    """tests/test_gpu_tap.py's problem with all four switches on (BEVR_SLAB=2: its table is narrower than SCA's): the new
    kernel on the scattered keys, the split-mode tap dropout kernels on the pinned ones from key index split on, merged
    through merge_views, against the oracle's materialised attention with ONE mask over all N keys and against the same
    call with BEVR_SCATTER_DROP unset.  Output TOL, gradients GRAD_LIM, d(pos) by the kink rule at 1e-3 as
    tests/test_gpu_tap_x3_dropout.py holds this call."""
    B, V, Cc, h, S, D, Hi, Wi, n_pin = 1, 2, 64, 2, 12, 3, 6, 20, 128
    seed = 0x5eed4321
    ins = _tap_problem(B, V, Cc, h, S, D, Hi, Wi, n_pin, seed=91)
    split, N = ins[-1], ins[4].shape[1]
    assert 0 < split < N
    keep = drop_mult(seed, P_DROP, B * V * h, S, N)
    cpu = [t.clone().double().requires_grad_(True) for t in ins[:-1]]
    want = _oracle_chain_drop(*cpu, h, V, keep)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    want.backward(cot)
    want_g = dict(zip(NAMES6, (t.grad for t in cpu)))
    runs = {}
    for new in (True, False):
        (out, gs), names = on_route(monkeypatch, new, lambda: tap_route(ins[:-1], split, h, V, (P_DROP, seed), cot),
                                    slab2=True, taps=True)
        assert set(TAP_X3_DROP) <= set(names) and "bevr_merge_views_fwd" in names, names
        runs[new] = (out, dict(zip(NAMES6, gs)))
    print(f"\n[slab x3 dropout region + tap] out new {rel_err(runs[True][0], want.detach()):.3e} parent "
          f"{rel_err(runs[False][0], want.detach()):.3e}")
    kinds = ("query", "feat", "Wkv", "bkv", "table")
    hold_both("region + tap", runs[True][1], runs[False][1], want_g, kinds)
    np.testing.assert_allclose(runs[False][0].numpy(), want.detach().numpy(), **TOL[X3])
    np.testing.assert_allclose(runs[True][0].numpy(), want.detach().numpy(), **TOL[X3])
    dist = pos_kink_distance(ins[4], S, 2 * S * D - 1, Hi, Wi)
    check_keys("region + tap d(pos), parent route", runs[False][1]["pos"], want_g["pos"], dist, 1e-3)
    check_keys("region + tap d(pos)", runs[True][1]["pos"], want_g["pos"], dist, 1e-3)


# ---- 5. high rates ------------------------------------------------------------------------------------------------------
def dominant_key_check(tag, out, grads, want_out, want, terms, pos, S, Wt):
    """the bounds of tests/test_gpu_dropout.py::test_dropout_high_rates_one_dominant_key_per_row; figures printed first"""
    figs, fails = [f"out {rel_err(out, want_out):.3e}"], []
    if not rel_err(out, want_out) < OUT_LIM[X3]:
        fails.append(figs[-1])
    for n, a, b in zip(NAMES5, grads, want):
        if not torch.isfinite(a).all():
            fails.append(f"grad {n} not finite")
            continue
        if n == "pos":
            clean = kink_distance(pos, S, Wt) >= 1e-4
            ep = (a[clean] - b[clean]).norm().item() / max(b[clean].norm().item(), 1e-30)
            figs.append(f"pos 2-norm {ep:.3e}")
            ok = ep < POS_LIM[X3]
        elif n in ("table", "query", "k"):
            # one key per row near P = 1: D dP - delta cancels there, the roundings apply to the terms
            bound = 2.0 * UNIT[X3] * terms[("table", "query", "k").index(n)] + LIM * b.abs().max().item()
            worst = ((a - b).abs() / bound).max().item()
            figs.append(f"{n} {worst:.2f} x its term bound")
            ok = worst < 1.0
        else:
            ev = (a - b).abs().max().item() / b.abs().max().item()
            figs.append(f"{n} {ev:.3e}")
            ok = ev < LIM
        if not ok:
            fails.append(figs[-1])
    print(f"[slab x3 dropout {tag}] " + "  ".join(figs))
    return fails


@pytest.mark.parametrize("p", STRESS_P)
def test_high_rates_one_dominant_key_per_row(p, monkeypatch):
    """tests/test_gpu_dropout.py::test_dropout_high_rates_one_dominant_key_per_row on the new route: D up to 100 and one key
    per row near P = 1, so D Pmax sits at the top of the slab's fixed-point cells and D dP - delta cancels where it must.
    That test's set-up and bounds."""
    B, V, Cc, h, g, S, D, N = 1, 1, 64, 2, 1, 12, 3, 96
    query, k, v, pos, table = _core_problem(B, V, Cc, h, g, S, D, N, seed=77)
    ins = (query * 12.0, k, v, pos, table)
    seed = 0x51ce + int(p * 1000)
    keep = drop_mult(seed, p, B * V * h, S, N)
    cpu = [t.clone().double().requires_grad_(True) for t in ins]
    want = _oracle_core_drop(*cpu, h, g, V, keep)
    with torch.no_grad():      # the premise: rows are dominated by one key
        pl = torch.softmax(torch.einsum("bcm,bcn->bmn", cpu[0][0].reshape(h, Cc // h, S * S),
                                        cpu[1][0].reshape(N, h, Cc // h).permute(1, 2, 0)) * (Cc // h) ** -0.5, -1)
        assert pl.amax(-1).median().item() > 0.9
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    want.backward(cot)
    terms = gradient_terms(cpu, cot, h, g, V, keep=keep, keys=True)
    want_g = [t.grad for t in cpu]
    (out1, g1), _ = on_route(monkeypatch, True, lambda: core5(ins, h, g, V, (p, seed), cot))
    (out0, g0), _ = on_route(monkeypatch, False, lambda: core5(ins, h, g, V, (p, seed), cot))
    Wt = 2 * S * D - 1
    print()
    f0 = dominant_key_check(f"dominant key p={p}, parent route", out0, g0, want.detach(), want_g, terms, pos, S, Wt)
    f1 = dominant_key_check(f"dominant key p={p}", out1, g1, want.detach(), want_g, terms, pos, S, Wt)
    assert not f0, f"p={p}: the PARENT route misses its bounds on these inputs: {f0}"
    assert not f1, f"p={p}: {f1}"


# ---- 6. the SCA module in training mode ---------------------------------------------------------------------------------
def _sampled_keys(rec, nb, Hi, Wi, C):
    """keys per problem of the ONE bevr_sample_fwd launch in a kernel-timer record, out of its byte count
    (ops.sample_features: 4 nb (Hi Wi C + N C + 2 N))"""
    assert rec["n"] == 1, rec
    return round((rec["bytes"] / (4.0 * nb) - Hi * Wi * C) / (C + 2))


def test_sca_module_in_training_takes_the_new_route(monkeypatch):
    """SpatialCrossAttn (its SCADeformableAttention) in bf16x3, training mode, attn_drop_rate = 0.3, S = 72 (24 x 64
    features, six views, 256 sampled BEV rows), the four switches on, at the module limits
    tests/test_gpu_tap_x3_dropout.py holds its module case to (out 3e-4, _check_module_grads in the f32 class).  The
    (p, seed) draw and the per-call cell_order permutation are captured and the kernels' mask is put into the oracle's key
    order; the parent's route (BEVR_SCATTER_DROP unset) repeats the step with the SAME draw and is asserted first."""
    from bevrender_amd.model import SCA_deform_attn as SCAmod
    from bevrender_amd.model.SCA import SpatialCrossAttn
    from bevrender_amd.model.bev_cmr_proj import BEV2CameraProjector
    from test_gpu_fullsize import _check_module_grads, _randomize, pick_rows, ring_rig
    from test_gpu_fullsize import rel_err as rel_err_rows
    S, img_w, img_h, n_rows = 72, 256, 96, 256
    D, V, C, h, B, Hi, Wi = 5, 6, 64, 2, 1, img_h // 4, img_w // 4
    N = (S // 2) * S * D
    T, K = ring_rig(V, img_w, img_h)
    proj = BEV2CameraProjector(imu_to_rgb={0: T}, K={0: K}, vehicle_type_code=0, img_width=img_w, img_height=img_h,
                               ori_img_width=img_w, ori_img_height=img_h, device=DEV)
    bound = {"X": 50, "Y": 50, "Z": 2}
    sca = SpatialCrossAttn(bound, proj, S, D, -1.0, C, h, 1, 1, 3, B, True, n_views=V, attn_drop_rate=0.3, precision=X3)
    _randomize(sca, 11)
    gen = torch.Generator().manual_seed(12)
    query, x = torch.randn(B, C, S, S, generator=gen), torch.randn(B, V, C, Hi, Wi, generator=gen)
    rows = pick_rows(S, n_rows, 5)
    cot = torch.randn(B, C, len(rows), generator=gen)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    att = sca.spatial_deform_attn
    used = [n for n, _ in att.named_parameters() if not n.startswith(("proj_q", "proj_views"))]
    pw = {k_: v_.detach().clone().double().requires_grad_(k_ in used) for k_, v_ in att.state_dict().items()}
    draws, orders, replay = [], [], []
    orig_drop, orig_order = SCAmod.attention_dropout, ops.cell_order

    def spy_drop(m):
        r = replay[0] if replay else orig_drop(m)
        draws.append(r)
        return r

    def spy_order(a, b, n_tail=0):
        r = orig_order(a, b, n_tail)
        orders.append((r.cpu(), n_tail))
        return r
    monkeypatch.setattr(SCAmod, "attention_dropout", spy_drop)
    monkeypatch.setattr(ops, "cell_order", spy_order)
    sca = sca.to(DEV).train()
    qg, xg = query.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    cot_full = torch.zeros(B, C, S * S, device=DEV)
    cot_full[:, :, rows.to(DEV)] = cot.to(DEV)

    def step():
        for t in list(sca.parameters()) + [qg, xg]:
            t.grad = None
        ops.KERNEL_TIMER.start()
        try:
            out, _ = sca(qg, xg.reshape(B * V, C, Hi, Wi), torch.tensor(0), None, False)
            out.backward(cot_full.reshape(B, C, S, S))
        finally:
            ran = ops.KERNEL_TIMER.stop()
        got = {n: prm.grad.clone() for n, prm in att.named_parameters() if prm.grad is not None}
        got.update({"in.query": qg.grad.clone(), "in.x": xg.grad.clone()})
        return out.detach().reshape(B, C, S * S)[:, :, rows.to(DEV)].cpu(), got, ran

    (out1, got1, ran1), names1 = on_route(monkeypatch, True, step, taps=True)
    replay.append(draws[0])
    (out0, got0, ran0), names0 = on_route(monkeypatch, False, step, taps=True)
    _, order, cs = sca.reference_points(0, qg.device)
    assert 0 < cs < 10000 and len(draws) == 2 and draws[0] is not None and draws[1] == draws[0] and len(orders) == 2
    assert torch.equal(orders[0][0], orders[1][0]) and orders[0][1] == orders[1][1]
    # the launches of the step: the three split-mode tap kernels with the mask, the region forward and bwd_k with the mask,
    # the new kernel under its own timer name, and no query-tile bwd_q
    for k in TAP_X3_DROP + (FWD_DROP, NEW, BWD_K_DROP):
        assert k in ran1 and ran1[k]["n"] >= 1, sorted(ran1)
    assert BWD_Q_DROP not in ran1 and "bevr_attn_bwd_q" not in ran1, sorted(ran1)
    assert BWD_Q_DROP in ran0 and NEW not in ran0, sorted(ran0)
    (pd, sd), (dyn, n_tail) = draws[0], orders[0]
    # ONE sampling launch, covering the region segment's keys alone: the pinned keys are neither sampled nor projected
    for ran in (ran1, ran0):
        assert _sampled_keys(ran["bevr_sample_fwd"], B * V, Hi, Wi, C) == cs + n_tail < N, (ran["bevr_sample_fwd"], cs, n_tail)
    # kernel key nk of view v is the oracle's key order[v][nk] for nk < cs and order[v][cs + dyn[problem][nk - cs]] behind
    m_k = drop_mult(sd, pd, B * V * h, S, N, rows=rows)
    keep = torch.empty_like(m_k)
    order = order.cpu()
    for pv in range(B * V):
        perm = order[pv % V][torch.cat((torch.arange(cs), cs + dyn[pv]))]
        keep[pv * h:(pv + 1) * h][:, :, perm] = m_k[pv * h:(pv + 1) * h]
    del m_k
    qc, xc = query.clone().double().requires_grad_(True), x.clone().double().requires_grad_(True)
    pts = O.sample_3d_points(bound, S, D, -1.0)
    ref = O.sca_reference_points(O.bev_grid_to_camera(pts, T, K, img_w, img_h, img_w, img_h), B).double()
    want = O.sca_forward(pw, xc, qc, ref, n_heads=h, depth_dim=D, rows=rows, keep=keep)
    (want * cot.double()).sum().backward()
    wnt = {n: pw[n].grad for n in used}
    wnt.update({"in.query": qc.grad, "in.x": xc.grad})
    e1, e0 = rel_err_rows(out1, want.detach()), rel_err_rows(out0, want.detach())
    eq = rel_err(got1["in.query"].cpu().double(), got0["in.query"].cpu().double())
    et = rel_err(got1["rpe_table"].cpu().double(), got0["rpe_table"].cpu().double())
    print(f"\n[sca module x3 slab dropout S={S}] out rel err new {e1:.3e} parent {e0:.3e}; new against parent: d(query) "
          f"{eq:.3e} d(table) {et:.3e}")
    assert e0 < 3e-4, f"the PARENT route misses the limit on these inputs: out {e0:.3e}"
    _check_module_grads(f"sca module x3 dropout S={S}, PARENT route", got0, wnt, 0)
    assert e1 < 3e-4, f"out: {e1:.3e}"
    _check_module_grads(f"sca module x3 slab dropout S={S}", got1, wnt, 0)
    assert torch.equal(out1, out0), "the two routes share one forward"
    assert eq < LIM and et < LIM, (eq, et)
