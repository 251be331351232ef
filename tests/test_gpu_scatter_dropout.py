"""Attention dropout on the gather forward and the slab bwd_q (csrc/attn_gather_fwd_drop.hip, csrc/attn_slab_bwd_q_drop.hip,
behind BEVR_SCATTER_DROP=1): the scattered keys of a call with a keep mask on the kernels they take without one.

Four levels.  bevr_attn_gather_fwd_dropout through the C ABI, on the operands ops.attention_core packs (picked up at its
own gather launch), against float64 with the host twin of the mask (ops.dropout_keep_mask) and against the no-mask entry
point on the same operands.  bevr_attn_slab_bwd_q_dropout on the operands of a call's backward, against float64 and against
bevr_attn_bwd_q_dropout on the same operands.  ops.attention_core(attn_drop=...) with the switch set, forward and every
gradient, against the oracle with the same mask and against the switch-unset route.  SCADeformableAttention in training
mode.  Limits: LIMITS of tests/test_gpu_fullsize.py, TOL and GRAD_LIM of tests/test_gpu_ops.py, check_dpos's rule.

Every test prints its figures before it asserts (-s); the recorded run is profiles/r19_scatter_dropout_errors.txt."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from bevrender_amd import _lib, ops
from oracle import bevrender_oracle as O
from test_gpu_dropout import STRESS_P, _oracle_core_drop, drop_mult
from test_gpu_fullsize import LIMITS, check_dpos, kink_distance, oracle_rows, pick_rows
from test_gpu_fullsize import rel_err as rel_err_rows
from test_gpu_gather import CASES as GATHER_CASES, _problem
from test_gpu_gather_rows import SENT, Outputs, band_rows, regime_inputs, run_core
from test_gpu_ops import CORE_CFGS, GRAD_LIM, TOL, _core_problem, rel_err
from test_gpu_random_sweep_routes import POS_LIM, UNIT, gradient_terms
from test_gpu_tap import _tap_problem
from test_gpu_tap_dropout import TAP_DROP, _oracle_chain_drop

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = _lib.PREC_BF16, _lib.PREC_F16
TAG = {BF16: "bf16", F16: "f16"}
P_DROP = 0.3
THR = int(round(P_DROP * 65536))
GATHER_DROP, SLAB_DROP = "bevr_attn_gather_fwd_dropout", "bevr_attn_slab_bwd_q_dropout"
FWD_DROP, BWD_Q_DROP, BWD_K_DROP = "bevr_attn_fwd_dropout", "bevr_attn_bwd_q_dropout", "bevr_attn_bwd_k_dropout"
NAMES5 = ["query", "k", "v", "pos", "table"]


def _ptr(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in ("BEVR_GATHER", "BEVR_SLAB", "BEVR_SLAB_ROWS", "BEVR_SCATTER_DROP"):
        monkeypatch.delenv(name, raising=False)


# ---- the gather forward through the C ABI ------------------------------------------------------------------------------
class DropOutputs(Outputs):
    def drop(self, dref, opnds, stream, row0, n_rows, seed, thr=THR):
        self.flags.zero_()
        _lib.check(_lib.lib().bevr_attn_gather_fwd_dropout(dref, *opnds, _ptr(self.O), _ptr(self.LSE), _ptr(self.flags),
                                                           row0, n_rows, thr, seed, stream), GATHER_DROP)
        self.flagged |= self.flags
        return self


def oracle_with_lse(ins, h, V, rows, keep):
    """float64: the output with the dropout multiplier `keep` on `rows` (query indices m = i S + j), and both LSE planes of
    those rows in the kernels' units (log2): plane 0 the log-sum-exp of the logits, plane 1 log2 of the largest softmax
    weight.  The logits are the oracle's own: picked up where oracle.attention_core hands them to its softmax."""
    seen = []
    real = O.F.softmax

    def spy(x, dim):
        seen.append(x.detach())
        return real(x, dim=dim)
    p = dict(zip(NAMES5, ins))
    O.F.softmax = spy
    try:
        want, _ = oracle_rows(p, h, rows, None, want_grads=False, keep=keep)
    finally:
        O.F.softmax = real
    logits = torch.cat(seen, 0)                                     # (V h, R, N), natural units
    lse = torch.logsumexp(logits, -1)
    return want, lse * ops.LOG2E, (logits.amax(-1) - lse) * ops.LOG2E


def lse_rows(out, rows, S):
    """both LSE planes of an Outputs at the query indices `rows`: (2, P h, R)"""
    _, L = out.by_row()                                             # (2, P, h, j, i)
    i, j = rows // S, rows % S
    return L[:, :, :, j.to(DEV), i.to(DEV)].reshape(2, -1, len(rows)).cpu().double()


def strip_tiles(pos, S, Wt, win_cols=28):
    """32-key tiles whose taps span more table columns than the gather window holds (at BEV column 0): emitted in strips"""
    _, b = ops.key_coords(pos, S, Wt, pos.shape[1])
    n = 0
    for t in range(0, pos.shape[1], 32):
        bt = b[:, t:t + 32]
        n += int(((bt.amax(1).floor() + 1 - bt.amin(1).floor() + 1) > win_cols).sum())
    return n


def _spread(u):
    return (u * 2 - 1) * 0.9


def _kd(S, D):
    """scattered keys in the modules' static k-d order: the 32-key tiles are leaves that fit the gather window"""
    def fn(u):
        pos = _spread(u)
        order = torch.from_numpy(ops.kd_key_order(pos[0].double().numpy(), S, 2 * S * D - 1))
        return pos[:, order].contiguous()
    return fn


GATHER_CFGS = {
    # B, V, C, h, S, D, N, key positions, calls (row0, n_rows) of the dropout entry point (None: the range (0, S))
    "S40 N100: one block per wave, ragged last block, padding keys": ((1, 1, 64, 2, 40, 3, 100), _spread, None),
    "S136: two blocks per wave, the last wave's second block past the column": ((1, 1, 64, 2, 136, 2, 1500), _kd(136, 2), None),
    "S240: the two bands of gather_bands": ((1, 1, 64, 2, 240, 2, 1500), _kd(240, 2), "bands"),
    "S240: the second band alone": ((1, 1, 64, 2, 240, 2, 1500), _kd(240, 2), "second"),
    "one key": ((1, 1, 64, 2, 8, 1, 1), lambda u: u * 2 - 1, None),
    "three views of one query, two heads": ((1, 3, 64, 2, 21, 3, 77), lambda u: (u * 2 - 1) * 0.5, None),
    "strips: two clusters far apart in every tile": (GATHER_CASES[1][1], GATHER_CASES[1][2], None),
}


@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(GATHER_CFGS))
def test_gather_dropout_entry_point(name, prec, monkeypatch):
    """bevr_attn_gather_fwd_dropout, p = 0.3: O and both LSE planes against float64 with the host twin of the mask at the
    mode's forward limit (LIMITS[...]["out"], relative to the largest entry); LSE equal to the no-mask entry point's to
    that limit; O more than 0.05 of its largest entry away from the no-mask O.  A band called alone with row0 > 0 hashes
    the absolute BEV row: it reproduces its rows of the same float64 result and leaves the others alone."""
    (B, V, Cc, h, S, D, N), pos_fn, calls = GATHER_CFGS[name]
    seed = 0x6a7 + S + N
    ins = _problem(B, V, Cc, h, S, D, N, 700 + N + S, pos_fn)
    Wt = 2 * S * D - 1
    n_tiles = B * V * ((N + 31) // 32)
    if name.startswith("strips"):       # tiles wider than the window: emitted in strips of 14 keys, the others masked
        assert strip_tiles(ins[3], S, Wt) == n_tiles, "a tile fits the window"
    elif S > 100:                       # k-d leaves: tiles that fit the window as they are, beside wider ones
        assert 0 < strip_tiles(ins[3], S, Wt) < n_tiles
    nblk = (min(S, 128) + 15) // 16 if calls else (S + 15) // 16
    assert (nblk > 7) == (S in (136, 240)), "NB = 2 instantiation"
    bands = ops.gather_bands(S)
    if calls == "bands":
        assert len(bands) == 2 and bands[1][0] > 0
        ranges = bands
    elif calls == "second":
        ranges = bands[1:]
    else:
        assert len(bands) == 1
        ranges = [(0, S)]
    got = {}

    def probe(dref, opnds, stream):
        d = dref._obj
        plain = Outputs(d)
        for r0, n in ranges:
            plain.rows(dref, opnds, stream, r0, n)
        masked = DropOutputs(d)
        for r0, n in ranges:
            masked.drop(dref, opnds, stream, r0, n, seed)
        got.update(plain=plain, masked=masked)

    run_core(ins, h, V, prec, monkeypatch, probe)
    assert set(got) == {"plain", "masked"}, "the gather launch was not reached"
    plain, masked = got["plain"], got["masked"]
    # columns are flagged on ALL the weights (fp16: also where the largest one lies too deep in the subnormals for N
    # keys): the mask flags the columns the no-mask entry point flags, and recomputes them under the same mask
    assert torch.equal(masked.flagged, plain.flagged)
    lo, hi = ranges[0][0], ranges[-1][0] + ranges[-1][1]
    if S <= 40:
        rows = torch.arange(S * S)
    else:
        rows = torch.unique(torch.cat((pick_rows(S, 48, 3), band_rows(S, bands, 9))))
    inside = (rows // S >= lo) & (rows // S < hi)
    rows_in = rows[inside]
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    keep = drop_mult(seed, P_DROP, B * V * h, S, N, rows=rows_in)
    want, lse0, lse1 = oracle_with_lse(ins, h, V, rows_in, keep)
    lim = LIMITS[prec]["out"]
    c = Cc // h
    o_m, o_p = masked.out(c)[:, rows_in], plain.out(c)[:, rows_in]
    L_m, L_p = lse_rows(masked, rows_in, S), lse_rows(plain, rows_in, S)
    e_o = rel_err_rows(o_m, want)
    e_l0, e_l1 = rel_err_rows(L_m[0], lse0), rel_err_rows(L_m[1], lse1)
    d_l0, d_l1 = rel_err_rows(L_m[0], L_p[0]), rel_err_rows(L_m[1], L_p[1]) if N > 1 else 0.0
    moved = (o_m - o_p).abs().max().item() / o_p.abs().max().item()
    print(f"\n[gather dropout {TAG[prec]} {name}] O {e_o:.3e}  LSE0 {e_l0:.3e}  LSE1 {e_l1:.3e}  "
          f"LSE against no mask {d_l0:.3e} {d_l1:.3e}  O against no mask {moved:.3e}  ({len(rows_in)} rows)")
    assert torch.isfinite(masked.LSE[masked.LSE != SENT]).all()
    assert e_o < lim, f"O {e_o:.3e}"
    assert e_l0 < lim, f"LSE plane 0 {e_l0:.3e}"
    if N > 1:      # (one key: plane 1 is log2(1) = 0 on both sides)
        assert e_l1 < lim, f"LSE plane 1 {e_l1:.3e}"
    else:
        assert L_m[1].abs().max().item() < lim
    assert d_l0 < lim and d_l1 < lim, (d_l0, d_l1)
    assert moved > 0.05, f"the mask changed O by {moved:.3e} only"
    if calls == "second":      # rows outside the band: untouched
        Om, Lm = masked.by_row()
        assert (Om[..., :lo, :] == SENT).all() and (Lm[..., :lo] == SENT).all()


@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "f16"])
def test_gather_dropout_recomputes_flagged_columns_under_the_mask(prec, monkeypatch):
    """tests/test_gpu_gather_rows.py's `useless` regime (huge orthogonal Q and K: the static bound lies thousands of
    binades over the logits, every weight of the first pass is zero): every column is flagged and recomputed by the EXACT
    instantiation, which must evaluate the same mask."""
    ins, (B, V, Cc, h, S, D, N) = regime_inputs("useless")
    seed = 0xe4ac7
    got = {}

    def probe(dref, opnds, stream):
        got["plain"] = Outputs(dref._obj).rows(dref, opnds, stream, 0, S)
        got["masked"] = DropOutputs(dref._obj).drop(dref, opnds, stream, 0, S, seed)

    run_core(ins, h, V, prec, monkeypatch, probe)
    masked, plain = got["masked"], got["plain"]
    assert int(masked.flagged.sum()) == masked.flagged.numel(), "not every column went to the exact pass"
    rows = torch.arange(S * S)
    keep = drop_mult(seed, P_DROP, B * V * h, S, N)
    want, lse0, lse1 = oracle_with_lse(ins, h, V, rows, keep)
    lim = LIMITS[prec]["out"]
    c = Cc // h
    e_o = rel_err_rows(masked.out(c), want)
    L_m, L_p = lse_rows(masked, rows, S), lse_rows(plain, rows, S)
    e_l0, e_l1 = rel_err_rows(L_m[0], lse0), rel_err_rows(L_m[1], lse1)
    moved = (masked.out(c) - plain.out(c)).abs().max().item() / plain.out(c).abs().max().item()
    print(f"\n[gather dropout {TAG[prec]} flagged columns] O {e_o:.3e}  LSE0 {e_l0:.3e}  LSE1 {e_l1:.3e}  "
          f"LSE against no mask {rel_err_rows(L_m[0], L_p[0]):.3e}  O against no mask {moved:.3e}")
    assert e_o < lim and e_l0 < lim and e_l1 < lim, (e_o, e_l0, e_l1)
    assert rel_err_rows(L_m[0], L_p[0]) < lim and rel_err_rows(L_m[1], L_p[1]) < lim
    assert moved > 0.05


# ---- the slab bwd_q on the operands of a call's backward -------------------------------------------------------------
def _far_rows(u):
    """keys over and past the table: some whose table rows leave the slab window for some row block (the clamped body)"""
    return (u * 2 - 1) * 1.6


SLAB_CFGS = {
    # B, V, C, h, S, D, N
    "S40: two row blocks": (1, 2, 64, 2, 40, 4, 700),
    "S70: three row blocks": (1, 2, 64, 2, 70, 4, 700),
}


def _capture_bwd_q(monkeypatch, name, store):
    """ops runs `name` through ops._RUN: keep what that launch adds into the (zeroed) dQ and d(table) of its call"""
    orig = ops._RUN[name]

    def wrapped(nm, o):
        assert not o.dQ.any() and not o.dT.any()
        orig(nm, o)
        torch.cuda.synchronize()
        store[name] = (o.dQ.clone(), o.dT.clone())
    monkeypatch.setitem(ops._RUN, name, wrapped)


@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(SLAB_CFGS))
def test_slab_dropout_entry_point(name, prec, monkeypatch):
    """bevr_attn_slab_bwd_q_dropout, p = 0.3, two problems of two heads, 700 keys with random b (runs longer than one
    emission, the sorted order far from the identity), an SCA-wide table over more than three slabs, keys whose rows leave
    the slab window.  The forward is the region dropout kernel in both runs (BEVR_GATHER=0), so both bwd_q launches see
    the same Q, dO, LSE, delta and scales: the slab launch's dQ and the call's d(table) against bevr_attn_bwd_q_dropout's, and
    the call's query and table gradients against float64 with the same mask, all at GRAD_LIM."""
    B, V, Cc, h, S, D, N = SLAB_CFGS[name]
    Wt = 2 * S * D - 1
    seed = 0x51ab + S
    ins = _problem(B, V, Cc, h, S, D, N, 300 + S, _far_rows)
    a, b = ops.key_coords(ins[3], S, Wt, N)
    far = (a.floor() + 10 < 0) | (a.floor() > S - 1 + 8)
    assert far.any() and not far.all(), "keys whose rows leave the slab window, beside keys inside it"
    order = b.argsort(1)
    assert (order != torch.arange(N)).float().mean() > 0.9, "the sorted order is far from the identity"
    assert (b.amax() - b.amin()).item() > 3 * 24, "at least three slabs"
    monkeypatch.setenv("BEVR_GATHER", "0")
    assert ops.slab_supported(prec, S, Wt)
    cot = torch.randn(B * V, S * S, Cc, generator=torch.Generator().manual_seed(4))
    store, res = {}, {}
    for sw in ("1", "0"):
        monkeypatch.setenv("BEVR_SCATTER_DROP", sw)
        kname = SLAB_DROP if sw == "1" else BWD_Q_DROP
        _capture_bwd_q(monkeypatch, kname, store)
        dev = [t.clone().to(DEV).requires_grad_(True) for t in ins]
        ops.KERNEL_TIMER.start()
        out = ops.attention_core(*dev, heads=h, groups=1, views=V, precision=prec, attn_drop=(P_DROP, seed))
        out.backward(cot.to(DEV))
        used = set(ops.KERNEL_TIMER.stop())
        assert kname in used and FWD_DROP in used and BWD_K_DROP in used, sorted(used)
        assert (SLAB_DROP in used) == (sw == "1") and (BWD_Q_DROP in used) == (sw == "0"), sorted(used)
        res[sw] = (out.detach().cpu().double(), [t.grad.cpu().double() for t in dev])
    assert torch.equal(res["1"][0], res["0"][0]), "the two runs share one forward"
    lim = GRAD_LIM[prec]
    (dq_s, dt_s), (dq_t, dt_t) = store[SLAB_DROP], store[BWD_Q_DROP]
    # (d(table): the call's table gradient, whose other terms are the same launches in both runs -- the raw buffers also
    # hold the zero padding around the table, where a clamped key's taps land in one kernel and are discarded in the other)
    e_dq, e_dt = rel_err(dq_s.double(), dq_t.double()), rel_err(res["1"][1][4], res["0"][1][4])
    print(f"\n[slab dropout {TAG[prec]} {name}] against bevr_attn_bwd_q_dropout: dQ {e_dq:.3e}  d(table) {e_dt:.3e}")
    keep = drop_mult(seed, P_DROP, B * V * h, S, N)
    cpu = [t.clone().double().requires_grad_(True) for t in ins]
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    want = _oracle_core_drop(*cpu, h, 1, V, keep)
    want.backward(cot.double())
    errs = {n: rel_err(g, c_.grad) for n, g, c_ in zip(NAMES5, res["1"][1], cpu)}
    print(f"[slab dropout {TAG[prec]} {name}] against float64: " + "  ".join(f"{n} {v:.3e}" for n, v in errs.items()))
    assert e_dq < lim and e_dt < lim, (e_dq, e_dt)
    assert errs["query"] < lim and errs["table"] < lim, errs
    assert dq_s.abs().max() > 0 and dt_s.abs().max() > 0


# ---- ops.attention_core with the switch set ----------------------------------------------------------------------------
def _core_run(ins, h, g, V, prec, drop, cot, **kw):
    dev = [t.clone().to(DEV).requires_grad_(True) for t in ins]
    ops.KERNEL_TIMER.start()
    out = ops.attention_core(*dev, heads=h, groups=g, views=V, precision=prec, attn_drop=drop, **kw)
    out.backward(cot.float().to(DEV))
    used = ops.KERNEL_TIMER.stop()
    return out.detach().cpu().double(), [t.grad.cpu().double() for t in dev], used


@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("cfg", CORE_CFGS, ids=[f"cfg{i}" for i in range(len(CORE_CFGS))])
def test_attention_core_with_the_switch_matches_the_oracle_and_the_region_route(cfg, prec, monkeypatch):
    """CORE_CFGS at p = 0.3 with BEVR_SCATTER_DROP=1 (BEVR_SLAB=2: the narrow tables among them take the slab route too):
    output (TOL) and every gradient (GRAD_LIM; positions by check_dpos's rule) against the oracle with the same mask; the
    same call on the switch-unset route with the same seed at the same limits; the launches."""
    B, V, Cc, h, g, S, D, N = cfg
    seed = 0x5eed1234
    ins = _core_problem(B, V, Cc, h, g, S, D, N, seed=sum(cfg))
    keep = drop_mult(seed, P_DROP, B * V * h, S, N)
    cpu = [t.clone().double().requires_grad_(True) for t in ins]
    want = _oracle_core_drop(*cpu, h, g, V, keep)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    want.backward(cot)
    monkeypatch.setenv("BEVR_SLAB", "2")
    monkeypatch.setenv("BEVR_SCATTER_DROP", "1")
    out, grads, used = _core_run(ins, h, g, V, prec, (P_DROP, seed), cot)
    monkeypatch.delenv("BEVR_SCATTER_DROP")
    out0, grads0, used0 = _core_run(ins, h, g, V, prec, (P_DROP, seed), cot)
    tag = f"core dropout {TAG[prec]} cfg {cfg}"
    errs = {n: rel_err(a, b.grad) for n, a, b in zip(NAMES5, grads, cpu)}
    errs0 = {n: rel_err(a, b) for n, a, b in zip(NAMES5, grads, grads0)}
    print(f"\n[{tag}] out {rel_err(out, want.detach()):.3e}  " + "  ".join(f"{n} {v:.3e}" for n, v in errs.items()))
    print(f"[{tag}] against the switch-unset route: out {rel_err(out, out0):.3e}  " +
          "  ".join(f"{n} {v:.3e}" for n, v in errs0.items()))
    assert {GATHER_DROP, SLAB_DROP, BWD_K_DROP} <= set(used), sorted(used)
    assert not {FWD_DROP, BWD_Q_DROP, "bevr_attn_gather_fwd", "bevr_attn_slab_bwd_q"} & set(used), sorted(used)
    assert {FWD_DROP, BWD_Q_DROP, BWD_K_DROP} <= set(used0) and not {GATHER_DROP, SLAB_DROP} & set(used0), sorted(used0)
    np.testing.assert_allclose(out.numpy(), want.detach().numpy(), **TOL[prec])
    np.testing.assert_allclose(out.numpy(), out0.numpy(), **TOL[prec])
    Wt = 2 * S * D - 1
    for n in ("query", "k", "v", "table"):
        assert errs[n] < GRAD_LIM[prec], f"{tag}: grad {n} {errs[n]:.3e}"
        assert errs0[n] < GRAD_LIM[prec], f"{tag}: grad {n} against the region route {errs0[n]:.3e}"
    check_dpos(grads[3], cpu[3].grad, ins[3], S, Wt, GRAD_LIM[prec], tag)
    check_dpos(grads[3], grads0[3], ins[3], S, Wt, GRAD_LIM[prec], tag + " (region route)")
    with torch.no_grad():
        plain = ops.attention_core(*[t.to(DEV) for t in ins], heads=h, groups=g, views=V, precision=prec)
    assert rel_err(plain.cpu().double(), want.detach()) > 0.05, "the mask changed nothing"


@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "f16"])
def test_region_and_tap_halves_share_one_mask(prec, monkeypatch):
    """A tap segment beside the region segment (kv_source, tap_source="pinned"): gather forward and slab bwd_q with the
    mask on the scattered keys, the tap dropout kernels on the pinned ones from key index split on, merged through
    merge_views -- ONE mask over all N keys, against the oracle's materialised attention with it.  The limits of
    tests/test_gpu_tap_dropout.py's host-path tests (TOL / GRAD_LIM of the mode)."""
    B, V, Cc, h, S, D, Hi, Wi, n_pin = 1, 2, 64, 2, 12, 3, 6, 20, 128
    seed = 0x5eed4321
    ins = _tap_problem(B, V, Cc, h, S, D, Hi, Wi, n_pin, seed=91)
    split, N = ins[-1], ins[4].shape[1]
    keep = drop_mult(seed, P_DROP, B * V * h, S, N)
    cpu = [t.clone().double().requires_grad_(True) for t in ins[:-1]]
    want = _oracle_chain_drop(*cpu, h, V, keep)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * (1e-5 if prec == F16 else 1.0)
    want.backward(cot)
    monkeypatch.setenv("BEVR_SCATTER_DROP", "1")
    gpu = [t.clone().to(DEV).requires_grad_(True) for t in ins[:-1]]
    query, feat, Wkv, bkv, pos, table = gpu
    ops.KERNEL_TIMER.start()
    got = ops.attention_core(query, None, None, pos, table, heads=h, groups=1, views=V, precision=prec,
                             kv_source=(feat, Wkv, bkv), cell_split=split, tap_source="pinned", attn_drop=(P_DROP, seed))
    got.backward(cot.float().to(DEV))
    used = set(ops.KERNEL_TIMER.stop())
    assert {GATHER_DROP, SLAB_DROP, BWD_K_DROP} | set(TAP_DROP) <= used, sorted(used)
    assert not {FWD_DROP, BWD_Q_DROP} & used, sorted(used)
    names = ["query", "feat", "Wkv", "bkv", "pos", "table"]
    errs = {n: rel_err(a.grad.double().cpu(), b.grad) for n, a, b in zip(names, gpu, cpu)}
    e = rel_err(got.detach().double().cpu(), want.detach())
    print(f"\n[region + tap dropout {TAG[prec]}] out {e:.3e}  " + "  ".join(f"{n} {v:.3e}" for n, v in errs.items()))
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().float().numpy(), **TOL[prec])
    for n, v in errs.items():
        assert v < GRAD_LIM[prec], f"grad {n}: {v:.3e}"


@pytest.mark.parametrize("p", STRESS_P)
@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "f16"])
def test_high_rates_one_dominant_key_per_row(prec, p, monkeypatch):
    """tests/test_gpu_dropout.py::test_dropout_high_rates_one_dominant_key_per_row on the new route: D up to 100, one key
    per row near P = 1 -- the forward's weights and the backward's operands at the top of their range, O / l and
    D dP - delta cancelling where they must.  That test's limits."""
    from test_gpu_random_sweep_routes import OUT_LIM
    B, V, Cc, h, g, S, D, N = 1, 1, 64, 2, 1, 12, 3, 96
    query, k, v, pos, table = _core_problem(B, V, Cc, h, g, S, D, N, seed=77)
    query = query * 12.0
    seed = 0x51ce + int(p * 1000)
    keep = drop_mult(seed, p, B * V * h, S, N)
    cpu = [t.clone().double().requires_grad_(True) for t in (query, k, v, pos, table)]
    want = _oracle_core_drop(*cpu, h, g, V, keep)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    want.backward(cot)
    monkeypatch.setenv("BEVR_SCATTER_DROP", "1")
    out, grads, used = _core_run((query, k, v, pos, table), h, g, V, prec, (p, seed), cot)
    assert {GATHER_DROP, SLAB_DROP} <= set(used) and not {FWD_DROP, BWD_Q_DROP} & set(used), sorted(used)
    tag = f"dominant key p={p} {TAG[prec]}"
    e = rel_err(out, want.detach())
    terms = gradient_terms(cpu, cot, h, g, V, keep=keep, keys=True)
    print(f"\n[{tag}] out {e:.3e}")
    assert e < OUT_LIM[prec], f"{tag}: out {e:.3e}"
    for n, a, b in zip(NAMES5, grads, cpu):
        b = b.grad
        assert torch.isfinite(a).all(), f"{tag}: grad {n} not finite"
        if n == "pos":
            clean = kink_distance(pos, S, 2 * S * D - 1) >= 1e-4
            ep = (a[clean] - b[clean]).norm().item() / max(b[clean].norm().item(), 1e-30)
            print(f"[{tag}] grad pos 2-norm {ep:.3e}")
            assert ep < POS_LIM[prec], f"{tag}: grad pos 2-norm {ep:.3e}"
            continue
        scale = b.abs().max().item()
        if n in ("table", "query", "k"):
            bound = 2.0 * UNIT[prec] * terms[("table", "query", "k").index(n)] + GRAD_LIM[prec] * scale
            worst = ((a - b).abs() / bound).max().item()
            print(f"[{tag}] grad {n} {worst:.2f} x its term bound")
            assert worst < 1.0, f"{tag}: grad {n} {worst:.2f} x its term bound"
            continue
        ev = (a - b).abs().max().item() / scale
        print(f"[{tag}] grad {n} {ev:.3e}")
        assert ev < GRAD_LIM[prec], f"{tag}: grad {n} {ev:.3e}"


# ---- the SCA module in training mode ---------------------------------------------------------------------------------
def test_sca_module_in_training_takes_the_scatter_dropout_route(monkeypatch):
    """SpatialCrossAttn (its SCADeformableAttention) in bf16, training mode, attn_drop_rate = 0.3, at S = 72 (24 x 64
    features, six views: the smallest side the tap route accepts with enough pinned keys), 256 sampled BEV rows.  The
    (p, seed) draw and the per-call cell_order permutation are captured, the kernels' mask is put into the oracle's key
    order, and the output and every parameter and input gradient are held to O.sca_forward(keep=...) at the module limits
    of tests/test_gpu_fullsize.py (out 2e-2, _check_module_grads).  The launches: the gather forward and the slab bwd_q
    with the mask beside the tap dropout kernels; no region forward or bwd_q."""
    from bevrender_amd.model import SCA_deform_attn as SCAmod
    from bevrender_amd.model.SCA import SpatialCrossAttn
    from bevrender_amd.model.bev_cmr_proj import BEV2CameraProjector
    from test_gpu_fullsize import _check_module_grads, _randomize, ring_rig
    monkeypatch.setenv("BEVR_SCATTER_DROP", "1")
    S, img_w, img_h, n_rows = 72, 256, 96, 256
    D, V, Cc, h, B, Hi, Wi = 5, 6, 64, 2, 1, img_h // 4, img_w // 4
    N = (S // 2) * S * D
    T, K = ring_rig(V, img_w, img_h)
    proj = BEV2CameraProjector(imu_to_rgb={0: T}, K={0: K}, vehicle_type_code=0, img_width=img_w, img_height=img_h,
                               ori_img_width=img_w, ori_img_height=img_h, device=DEV)
    bound = {"X": 50, "Y": 50, "Z": 2}
    sca = SpatialCrossAttn(bound, proj, S, D, -1.0, Cc, h, 1, 1, 3, B, True, n_views=V, attn_drop_rate=0.3, precision=BF16)
    _randomize(sca, 11)
    gen = torch.Generator().manual_seed(12)
    query, x = torch.randn(B, Cc, S, S, generator=gen), torch.randn(B, V, Cc, Hi, Wi, generator=gen)
    rows = pick_rows(S, n_rows, 5)
    cot = torch.randn(B, Cc, len(rows), generator=gen)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    att = sca.spatial_deform_attn
    used_p = [n for n, _ in att.named_parameters() if not n.startswith(("proj_q", "proj_views"))]
    pw = {k_: v_.detach().clone().double().requires_grad_(k_ in used_p) for k_, v_ in att.state_dict().items()}
    draws, orders = [], []
    orig_drop, orig_order = SCAmod.attention_dropout, ops.cell_order

    def spy_drop(m):
        r = orig_drop(m)
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
    cot_full = torch.zeros(B, Cc, S * S, device=DEV)
    cot_full[:, :, rows.to(DEV)] = cot.to(DEV)
    ops.KERNEL_TIMER.start()
    try:
        out, _ = sca(qg, xg.reshape(B * V, Cc, Hi, Wi), torch.tensor(0), None, False)
        out.backward(cot_full.reshape(B, Cc, S, S))
    finally:
        ran = ops.KERNEL_TIMER.stop()
    _, order, cs = sca.reference_points(0, qg.device)
    assert 0 < cs < 10000 and len(draws) == 1 and draws[0] is not None and len(orders) == 1
    assert {GATHER_DROP, SLAB_DROP, BWD_K_DROP} | set(TAP_DROP) <= set(ran), sorted(ran)
    assert not {FWD_DROP, BWD_Q_DROP, "bevr_attn_fwd", "bevr_attn_bwd_q"} & set(ran), sorted(ran)
    (pd, sd), (dyn, n_tail) = draws[0], orders[0]
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
    e = rel_err_rows(out.detach().reshape(B, Cc, S * S)[:, :, rows.to(DEV)].cpu(), want.detach())
    print(f"\n[sca module bf16 scatter dropout S={S}] out rel err {e:.3e}")
    got = {n: prm.grad for n, prm in att.named_parameters()}
    got.update({"in.query": qg.grad, "in.x": xg.grad})
    wnt = {n: pw[n].grad for n in used_p}
    wnt.update({"in.query": qc.grad, "in.x": xc.grad})
    assert e < 2e-2, f"out: {e:.3e}"
    _check_module_grads(f"sca module bf16 scatter dropout S={S}", got, wnt, BF16)
