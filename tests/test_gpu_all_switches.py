"""Every opt-in switch on together (ALL_ON of tests/test_all_switches_routes_cpu.py), against float64:

1. ops.attention_core on every distinct route of the all-on table, called the way the route takes its operands (the fused
   K | V source in the 16-bit modes, projected rows + tap_pix in bf16x3), forward and one backward for every input, with
   the launches it must make and the ones it must not;
2. the SCA module in training mode under ALL_ON, and under FLOOR (every default-on A/B switch at "0": the plain route the
   README's "same results" and every A/B timing compare against);
3. the whole model under ALL_ON on the conditioned fixtures.

No tolerance here is new: every limit is the one the existing test of the same route and mode applies (named at each
check).  Every case also runs with every switch unset on the same inputs, seed and mask -- a control, printed beside the
all-on figures and not asserted (it is held to the oracle by its own tests).  teardown_module prints the table that
profiles/all_switches.txt records."""
import functools
import logging
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bevrender_amd import _lib, ops
from oracle import bevrender_oracle as O
from test_all_switches_routes_cpu import ALL_ON, DEFAULT_ON, FLOOR, GRID, OPT_IN
from test_gpu_dropout import _oracle_core_drop, drop_mult
from test_gpu_fullsize import check_dpos, kink_distance, pick_rows
from test_gpu_ops import GRAD_LIM, TOL, _oracle_core, rel_err
from test_gpu_random_sweep_routes import (POS_LIM, TAP_GRAD_LIM, TAP_OUT_LIM, UNIT, chain_kv, gradient_terms,
                                          pixel_kink_distance)
from test_gpu_tap_x3 import check_keys, pos_kink_distance

DEV = "cuda"
F32, X3, BF16, F16 = _lib.PREC_F32, _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16
MODE = {X3: "bf16x3", BF16: "bf16", F16: "f16"}
P_DROP, SEED = 0.3, 0x5eed1234
NAMES = ["query", "feat", "Wkv", "bkv", "pos", "table"]
RECORD = []         # (case, quantity, all-on error / limit, control error / limit, launched): teardown_module's table

A = "bevr_attn_"
TAPS = {A + "tap_fwd", A + "tap_bwd_q", A + "tap_bwd_k"}
TAPS_DROP = {A + "tap_fwd_dropout", A + "tap_bwd_q_dropout", A + "tap_bwd_k_dropout"}
TAPS_X3_DROP = {A + "tap_fwd_x3_dropout", A + "tap_bwd_q_x3_dropout", A + "tap_bwd_k_x3_dropout"}
TAPS_G2 = {A + "tap_g2_fwd", A + "tap_g2_bwd_q", A + "tap_g2_bwd_k"}
CELL = {A + "cell_fwd", A + "cell_bwd_q", A + "cell_bwd_k"}
TILE = {A + "fwd", A + "bwd_q", A + "bwd_k"}
TILE_DROP = {A + "fwd_dropout", A + "bwd_q_dropout", A + "bwd_k_dropout"}
# every entry point a route chooses among (ops.K): what "no other attention kernel ran" is judged over
FAMILY = {v for v in vars(ops.K).values() if isinstance(v, str) and v.startswith(A)}


def set_switches(monkeypatch, env):
    for name in OPT_IN + DEFAULT_ON:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


class Launches:
    """What ran: ops.KERNEL_TIMER's timer names and the library symbols behind them (as tests/test_gpu_kv_wsplit.py
    takes them), and every entry point ops._launch was asked for, timed or not (bevr_pack_kv, the merges)."""

    def __init__(self, monkeypatch):
        self.names, self.symbols, self.entries = set(), set(), set()
        run, launch = ops.KERNEL_TIMER.run, ops._launch

        def timed(name, flops, fn, *args, **kw):
            self.names.add(name)
            self.symbols.add(getattr(fn, "__name__", repr(fn)))
            return run(name, flops, fn, *args, **kw)

        def launched(entry, *args, **kw):
            self.entries.add(entry)
            return launch(entry, *args, **kw)
        monkeypatch.setattr(ops.KERNEL_TIMER, "run", timed)
        monkeypatch.setattr(ops, "_launch", launched)

    def take(self):
        got = (set(self.names), set(self.symbols), set(self.entries))
        self.names.clear(), self.symbols.clear(), self.entries.clear()
        return got


# ---------------------------------------------------------------------------------------------------------------------
# 1. attention_core on every distinct all-on route
# ---------------------------------------------------------------------------------------------------------------------
# (S, D): feature map sides inside the tap contract as tests/test_gpu_random_sweep_routes.py::draw bounds them
# (2.5 (Hi - 1) / (Hk - 1) < 3, 2.5 (Wi - 1) / (Wk - 1) < 2, at most 48), keys, scattered keys (the split)
#   S = 40: two row blocks of the slab kernel, three 16-row blocks of the gather forward, a ragged split (437 = 13 x 32 + 21)
#   and a ragged pinned segment; S = 240 > 211, > 224: two gather bands, two slab bands, the tile bwd_q with a mask
SHAPES = {(40, 3): (16, 44, 700, 437), (40, 1): (16, 30, 700, 437), (240, 2): (24, 44, 2000, 1333)}
N_ROWS = 256        # S = 240: sampled query rows, the cotangent zero elsewhere

# row of the all-on table -> (groups, S, D, keep mask)
SHAPE_OF = {"g1-S40": (1, 40, 3, False), "g1-S40-mask": (1, 40, 3, True), "g2-S40": (2, 40, 3, False),
            "g2-S40-mask": (2, 40, 3, True), "g1-S240": (1, 240, 2, False), "g1-S240-mask": (1, 240, 2, True),
            "g2-S240": (2, 240, 2, False), "g1-S40-narrow": (1, 40, 1, False)}
# the attention entry points each row must launch -- these and no other of FAMILY -- and its merge, written out
REGION = lambda fwd, bwd_q, drop=False: {A + fwd, A + bwd_q, A + ("bwd_k_dropout" if drop else "bwd_k")}     # noqa: E731
WANT_16 = {
    "g1-S40": (REGION("gather_fwd", "slab_bwd_q") | TAPS, "merge_tap"),
    "g1-S40-mask": (REGION("gather_fwd_dropout", "slab_bwd_q_dropout", True) | TAPS_DROP, "merge_views"),
    "g2-S40": (REGION("gather_fwd", "slab_bwd_q") | TAPS_G2, "merge_views"),
    "g2-S40-mask": (REGION("gather_fwd_dropout", "slab_bwd_q_dropout", True), "merge_views"),
    "g1-S240": (REGION("gather_fwd_rows", "slab_bwd_q_rows") | TAPS, "merge_tap"),
    "g1-S240-mask": (REGION("gather_fwd_dropout", "bwd_q_dropout", True) | TAPS_DROP, "merge_views"),
    "g2-S240": (REGION("gather_fwd_rows", "slab_bwd_q_rows") | TAPS_G2, "merge_views"),
    "g1-S40-narrow": (REGION("gather_fwd", "bwd_q") | TAPS, "merge_tap"),
}
WANT_X3 = {
    "g1-S40": (REGION("gather_fwd_x3", "slab_bwd_q_x3") | TAPS, "merge_tap"),
    "g1-S40-mask": (REGION("fwd_dropout", "slab_bwd_q_x3_dropout", True) | TAPS_X3_DROP, "merge_views"),
    "g1-S240": (REGION("gather_fwd_x3", "bwd_q") | TAPS, "merge_tap"),
    "g2-S40": (REGION("gather_fwd_x3", "slab_bwd_q_x3"), "merge_views"),
    "g2-S40-mask": (REGION("fwd_dropout", "slab_bwd_q_x3_dropout", True), "merge_views"),
    "g1-S40-narrow": (REGION("gather_fwd_x3", "bwd_q") | TAPS, "merge_tap"),
}
# fp16 runs twice: cotangents of size 1 and of a mean-type loss (1e-5: fp16 subnormals without the power-of-two scale)
CORE_CASES = [(BF16, row, 1.0) for row in WANT_16] + [(F16, row, cs) for row in WANT_16 for cs in (1.0, 1e-5)] \
    + [(X3, row, 1.0) for row in WANT_X3]


def case_id(c):
    prec, row, cs = c
    return f"{MODE[prec]}-{row}" + ("" if cs == 1.0 else "-cot1e-5")


@functools.lru_cache(maxsize=None)
def inputs(row):
    """tests/test_gpu_random_sweep_routes.py::make's `tap` problem (float32, CPU): keys [0, split) scattered over the
    image, keys [split, N) pinned to pixel (0, 0) and moved by offsets inside the learned range, tanh(.) * 5 / (Hk - 1),
    5 / (Wk - 1).  One group: the pinned keys cell-sorted, as the module hands them over.  Two groups: every group its
    own position of every key, row p * 2 + g, and no order (tests/test_gpu_tap_groups.py::_problem: attention_core sorts
    per (problem, group) itself).  S = 240: the scattered keys in the modules' static k-d order (ops.kd_key_order), whose
    32-key tiles fit the gather window.  Wkv is randn / sqrt(C): not representable in bf16 or fp16, so the lo plane of
    bevr_kv_project_w2 is not zero (tests/test_gpu_kv_wsplit.py)."""
    g, S, D, mask = SHAPE_OF[row]
    Hi, Wi, N, split = SHAPES[(S, D)]
    B, V, C, h = 1, (1 if S > 211 else 2), 64, 2
    P, Hk, Wk, Wt = B * V, S // 2, S * D, 2 * S * D - 1
    gen = torch.Generator().manual_seed(1000 + 7 * S + D + 100 * g)
    query = torch.randn(B, C, S, S, generator=gen)
    table = torch.randn(h, 2 * S - 1, Wt, generator=gen) * 0.3
    feat = torch.randn(P, Hi, Wi, C, generator=gen)
    Wkv = torch.randn(2 * C, C, generator=gen) * C ** -0.5
    bkv = torch.randn(2 * C, generator=gen) * 0.3
    scat = (torch.rand(P * g, split, 2, generator=gen) * 2 - 1) * 1.05
    off = torch.tanh(torch.randn(P * g, N - split, 2, generator=gen) * 1.5) * torch.tensor([5.0 / (Hk - 1), 5.0 / (Wk - 1)])
    pin = off - 1.0
    rows = pick_rows(S, N_ROWS, 5) if S > 211 else None
    if g == 2:
        # tests/test_gpu_tap_groups.py holds d(pos) in the max-norm over EVERY key.  d(pos) jumps where a table coordinate
        # or the sampling position crosses an integer, and a key within float32 rounding of such a kink takes the other
        # side's derivative in any float32 evaluation (check_dpos, tests/test_gpu_fullsize.py): with 2 000 keys against 160
        # BEV columns one key lay 7e-7 from a kink and departed by 2.5e-2 of the largest entry -- the same figure in bf16,
        # in fp16 and with every switch unset.  The two-group inputs keep every key 1e-4 away from a kink, redrawn until
        # they do; the one-group rules judge the keys away from kinks themselves
        cols = None if rows is None else (rows % S).tolist()
        for t, redraw in ((scat, lambda n: (torch.rand(n, 2, generator=gen) * 2 - 1) * 1.05),
                          (pin, lambda n: torch.tanh(torch.randn(n, 2, generator=gen) * 1.5)
                           * torch.tensor([5.0 / (Hk - 1), 5.0 / (Wk - 1)]) - 1.0)):
            for _ in range(100):
                near = torch.minimum(kink_distance(t, S, Wt, cols), pixel_kink_distance(t, Hi, Wi)) < 1e-4
                if not near.any():
                    break
                t[near] = redraw(int(near.sum()))
            assert not near.any()
    if g == 1:
        a, b = ops.key_coords(pin, S, Wt, N - split)
        pin = pin.gather(1, ops.cell_order(a, b)[..., None].expand(-1, -1, 2))
    if S > 211:
        order = torch.from_numpy(np.asarray(ops.kd_key_order(scat[0].double().numpy(), S, Wt))).long()
        scat = scat[:, order].contiguous()
    ins = dict(query=query, feat=feat, Wkv=Wkv, bkv=bkv, pos=torch.cat((scat, pin), 1), table=table)
    meta = dict(row=row, g=g, S=S, D=D, mask=mask, B=B, V=V, C=C, h=h, N=N, split=split, Wt=Wt, Hi=Hi, Wi=Wi, rows=rows)
    return ins, meta


def oracle_core_rows(query, k, v, pos, table, h, g, V, rows, keep):
    """_oracle_core / _oracle_core_drop (tests/test_gpu_ops.py, tests/test_gpu_dropout.py) on the query rows `rows`:
    (B V, len(rows), C)"""
    B, C, S, _ = query.shape
    c = C // h
    Bp, N, _ = k.shape
    outs = []
    for bp in range(Bp):
        q = query[bp // V].reshape(h, c, S * S)
        kk = k[bp].reshape(N, h, c).permute(1, 2, 0)
        vv = v[bp].reshape(N, h, c).permute(1, 2, 0)
        o = O.attention_core(q, kk, vv, pos[bp * g:(bp + 1) * g], table, S, S, g, c ** -0.5, rows=rows,
                             keep=None if keep is None else keep[bp * h:(bp + 1) * h])
        outs.append(o.reshape(C, len(rows)).t())
    return torch.stack(outs, 0)


def gradient_terms_rows(ins, cot, h, V, rows):
    """gradient_terms (tests/test_gpu_random_sweep_routes.py) for a cotangent that lives on the query rows `rows` alone
    (one group, no mask): a row without cotangent has dO = 0, so dS = 0 and A = 0 -- it adds no term."""
    query, k, v, pos, table = [t.detach() for t in ins]
    B, C, S, _ = query.shape
    c, M = C // h, S * S
    Bp, N, _ = k.shape
    tab = table.clone().requires_grad_(True)
    q_grid = O.normalized_grid(S, S, torch.float64).reshape(1, M, 2)[:, rows]
    dq = torch.zeros(B, h, c, M, dtype=torch.float64)
    total = 0.0
    for bp in range(Bp):
        q = query[bp // V].reshape(h, c, M)[:, :, rows]
        kk = k[bp].reshape(N, h, c).permute(1, 2, 0)
        vv = v[bp].reshape(N, h, c).permute(1, 2, 0)
        disp = (q_grid.unsqueeze(2) - pos[bp:bp + 1].reshape(1, 1, N, 2)) * 0.5
        bias = F.grid_sample(tab.reshape(1, h, *tab.shape[-2:]), disp[..., (1, 0)], mode="bilinear",
                             align_corners=True).reshape(h, len(rows), N)
        P = torch.softmax(torch.einsum("bcm,bcn->bmn", q, kk) * c ** -0.5 + bias.detach(), dim=2)
        dO = cot[bp].t().reshape(h, c, len(rows))
        dP = torch.einsum("bcm,bcn->bmn", dO, vv)
        Ab = torch.einsum("bcm,bcn->bmn", dO.abs(), vv.abs())
        dS = P * (dP - (P * dP).sum(2, keepdim=True))
        mag = dS.abs() + P * (Ab + (P * Ab).sum(2, keepdim=True))
        total = total + (bias * mag).sum()
        dq[bp // V][:, :, rows] += c ** -0.5 * torch.einsum("bmn,bcn->bcm", mag, kk.abs())
    total.backward()
    return tab.grad, dq.reshape(B, C, S, S)


@functools.lru_cache(maxsize=None)
def reference(row):
    """float64, once per row of the table and left unchanged: the output (on the sampled rows at S = 240), the gradients
    for a cotangent of size 1 (every gradient is linear in it), and for the one-group rows without a mask the term
    magnitudes behind the table and query gradients (gradient_terms)."""
    ins, m = inputs(row)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cpu = {n: t.clone().double().requires_grad_(True) for n, t in ins.items()}
    k64, v64 = chain_kv(cpu["feat"], cpu["Wkv"], cpu["bkv"], cpu["pos"], m["g"])
    rows, keep = m["rows"], None
    if m["mask"]:       # ONE mask over all N keys: the region and the tap halves share it
        keep = drop_mult(SEED, P_DROP, m["B"] * m["V"] * m["h"], m["S"], m["N"], rows=rows)
    core = (cpu["query"], k64, v64, cpu["pos"], cpu["table"], m["h"], m["g"], m["V"])
    if rows is not None:
        want = oracle_core_rows(*core, rows, keep)
    else:
        want = _oracle_core(*core) if keep is None else _oracle_core_drop(*core, keep)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(77), dtype=torch.float64)
    want.backward(cot)
    terms = None
    if m["g"] == 1 and not m["mask"]:
        five = [cpu["query"], k64, v64, cpu["pos"], cpu["table"]]
        terms = gradient_terms(five, cot, m["h"], 1, m["V"]) if rows is None else gradient_terms_rows(five, cot, m["h"], m["V"], rows)
    return want.detach(), cot, {n: t.grad for n, t in cpu.items()}, terms


def clean_keys(ins, m):
    """run_case's keys away from kinks (tests/test_gpu_random_sweep_routes.py): table coordinates and sampling position,
    1e-4; at S = 240 over the BEV columns that carry cotangent"""
    cols = None if m["rows"] is None else (m["rows"] % m["S"]).tolist()
    return (kink_distance(ins["pos"], m["S"], m["Wt"], cols) >= 1e-4) & (pixel_kink_distance(ins["pos"], m["Hi"], m["Wi"]) >= 1e-4)


@pytest.mark.parametrize("row", list(SHAPE_OF))
def test_inputs_keep_their_checks_meaningful(row):
    """No GPU: the inputs alone decide how many keys the position checks can judge.  run_case asks for a clean share above
    0.5, check_keys for 0.3 at its 1e-3 -- held here with margin; the weights are off the 16-bit grids; the split is ragged
    and both segments hold several 32-key tiles."""
    ins, m = inputs(row)
    cols = None if m["rows"] is None else (m["rows"] % m["S"]).tolist()
    assert clean_keys(ins, m).float().mean().item() > 0.9                      # run_case asks for 0.5
    x3_share = (pos_kink_distance(ins["pos"], m["S"], m["Wt"], m["Hi"], m["Wi"], cols) >= 1e-3).double().mean().item()
    assert x3_share > 0.6                                                      # check_keys asks for 0.3
    assert (kink_distance(ins["pos"], m["S"], m["Wt"], cols) >= 2e-3).float().mean().item() > 0.3      # check_dpos: not vacuous
    for dt in (torch.bfloat16, torch.float16):
        assert (ins["Wkv"].to(dt).float() != ins["Wkv"]).float().mean().item() > 0.9
    assert m["split"] % 32 and (m["N"] - m["split"]) % 32 and m["split"] > 64 and m["N"] - m["split"] > 64
    wide = m["Wt"] - 1 >= 4 * (m["S"] - 1)
    assert wide == (not row.endswith("narrow"))
    # the pinned keys keep the tap contract (SCADeformableAttention._pinned_keys_tap)
    ky = (ins["pos"][:, m["split"]:, 0] + 1.0) * (0.5 * (m["Hi"] - 1))
    kx = (ins["pos"][:, m["split"]:, 1] + 1.0) * (0.5 * (m["Wi"] - 1))
    assert (ky < ops.TAP_R - 1).all() and (kx < ops.TAP_C - 1).all()


def run_core(ins, m, prec, cot_full):
    """ops.attention_core the way SCADeformableAttention.forward calls it under the switches in force: the fused K | V
    source where the kernel covers the call, the tap segment beside projected rows in bf16x3 (tap_pix), else projected
    rows of every key; the pinned split kept where the tap (or, one group, the cell) kernels take it."""
    gpu = {n: t.clone().to(DEV).requires_grad_(True) for n, t in ins.items()}
    g, h, C, split = m["g"], m["h"], m["C"], m["split"]
    drop = (P_DROP, SEED) if m["mask"] else None
    pinned = ops.tap_supported(prec, g)
    if not (g == 1 or (pinned and ops.tap_supported(prec, g, dropout=drop is not None))):
        split = None
    kw = dict(heads=h, groups=g, views=m["V"], precision=prec, attn_drop=drop)
    core = (gpu["query"], None, None, gpu["pos"], gpu["table"])
    xf = gpu["feat"].permute(0, 3, 1, 2)
    if ops.kv_source_supported(C, h, g, prec):
        how = "kv_source"
        if split is not None:
            kw.update(cell_split=split, tap_source="pinned" if pinned else False)
        out = ops.attention_core(*core, kv_source=(gpu["feat"], gpu["Wkv"], gpu["bkv"]), **kw)
    elif prec == X3 and pinned and split is not None and (drop is None or ops.tap_supported(prec, g, dropout=True)):
        how = "tap_pix"
        kv = F.linear(ops.sample_features(xf, gpu["pos"][:, :split].contiguous(), 1), gpu["Wkv"], gpu["bkv"])
        out = ops.attention_core(*core, kv=kv, cell_split=split, tap_source="pinned",
                                 tap_pix=(gpu["feat"], gpu["Wkv"], gpu["bkv"]), **kw)
    else:
        how = "kv"
        kv = F.linear(ops.sample_features(xf, gpu["pos"], g), gpu["Wkv"], gpu["bkv"])
        out = ops.attention_core(*core, kv=kv, cell_split=split, **kw)
    out.backward(cot_full)
    torch.cuda.synchronize()
    got = out.detach().double().cpu()
    if m["rows"] is not None:
        got = got[:, m["rows"]]
    return how, got, {n: t.grad.double().cpu() for n, t in gpu.items()}


def allclose_ratio(got, want, rtol, atol):
    """np.testing.assert_allclose as a figure: the largest |got - want| / (atol + rtol |want|); below 1 where it passes"""
    return ((got - want).abs() / (atol + rtol * want.abs())).max().item()


def held(fn, *args, **kw):
    """an existing rule with several conditions (check_dpos, check_keys): None where it holds, its message where not"""
    try:
        fn(*args, **kw)
    except AssertionError as e:
        return str(e) or "failed"
    return None


def judge(tag, prec, m, ins, got, grads, want, want_g, terms, cs):
    """[(quantity, error / carried limit)], [failures]: the limits of the existing test of the same route and mode."""
    figs, fails = [], []

    def fig(name, ratio):
        figs.append((name, ratio))
        if not ratio < 1.0:
            fails.append(f"{tag}: {name} at {ratio:.2f} x its limit")

    g, S, Wt, mask = m["g"], m["S"], m["Wt"], m["mask"]
    cols = None if m["rows"] is None else (m["rows"] % S).tolist()
    if prec == X3:
        # tests/test_gpu_tap_x3.py::test_attention_core_with_tap_pix_matches_the_oracle, and with a mask the same figures in
        # tests/test_gpu_tap_x3_dropout.py plus TOL / GRAD_LIM of tests/test_gpu_slab_x3_dropout.py (5e-4: no tighter)
        fig("out", rel_err(got, want) / 2e-4)
        if mask:
            fig("out (TOL)", allclose_ratio(got, want, **TOL[X3]))
        for n in ("query", "feat", "Wkv", "bkv", "table"):
            fig(n, rel_err(grads[n], want_g[n]) / (2.5e-4 if n == "table" else 5e-4))
        dist = pos_kink_distance(ins["pos"], S, Wt, m["Hi"], m["Wi"], cols)
        clean = dist >= 1e-3
        figs.append(("pos", ((grads["pos"] - want_g["pos"]).abs().amax(-1)[clean].max() / want_g["pos"].abs().max()).item() / 1e-3))
        msg = held(check_keys, f"{tag} d(pos)", grads["pos"], want_g["pos"], dist, 1e-3)
        if msg:
            fails.append(msg)
    elif mask:
        # tests/test_gpu_scatter_dropout.py::test_attention_core_with_the_switch_matches_the_oracle_and_the_region_route:
        # TOL on the output, GRAD_LIM on every gradient, the positions by check_dpos's rule
        fig("out", allclose_ratio(got, want, **TOL[prec]))
        for n in ("query", "feat", "Wkv", "bkv", "table"):
            fig(n, rel_err(grads[n], want_g[n]) / GRAD_LIM[prec])
        clean = kink_distance(ins["pos"], S, Wt, cols) >= 2e-3
        dw = want_g["pos"]
        figs.append(("pos", ((grads["pos"] - dw)[clean].norm() / dw[clean].norm()).item() / GRAD_LIM[prec]))
        msg = held(check_dpos, grads["pos"], dw, ins["pos"], S, Wt, GRAD_LIM[prec], tag, cols)
        if msg:
            fails.append(msg)
    elif g == 2:
        # tests/test_gpu_tap_groups.py: bf16 rtol 3e-2 / atol 1.5e-2 and 3e-2 on every gradient; fp16 2.5e-3 and 5e-3
        if prec == BF16:
            fig("out", allclose_ratio(got, want, 3e-2, 1.5e-2))
        else:
            fig("out", rel_err(got, want) / 2.5e-3)
        for n in NAMES:
            fig(n, rel_err(grads[n], want_g[n]) / (3e-2 if prec == BF16 else 5e-3))
    else:
        # run_case's `tap` route (tests/test_gpu_random_sweep_routes.py): TAP_OUT_LIM, TAP_GRAD_LIM, the gradient_terms
        # bound for the pinned keys' table and query gradients, POS_LIM in the 2-norm on keys away from kinks
        fig("out", rel_err(got, want) / TAP_OUT_LIM[prec])
        for n in NAMES:
            a, b = grads[n], want_g[n]
            if n == "pos":
                clean = clean_keys(ins, m)
                if not clean.float().mean().item() > 0.5:
                    fails.append(f"{tag}: kink neighbourhood too wide for this case")
                dg, dw = a[clean], b[clean]
                fig("pos", (dg - dw).norm().item() / max(dw.norm().item(), 2e-2 * cs * max(dw.numel(), 1) ** 0.5) / POS_LIM[prec])
                continue
            scale = max(b.abs().max().item(), 2e-2 * cs)
            if n in ("table", "query"):
                bound = 2.0 * UNIT[prec] * terms[n == "query"] * cs + TAP_GRAD_LIM[prec] * scale
                fig(n, ((a - b).abs() / bound).max().item())
                continue
            fig(n, (a - b).abs().max().item() / scale / TAP_GRAD_LIM[prec])
    for n in NAMES:
        if not torch.isfinite(grads[n]).all():
            fails.append(f"{tag}: grad {n} not finite")
    return figs, fails


def table_row(prec, m):
    """the point of tests/test_all_switches_routes_cpu.py's table this case is a call of"""
    width = "wide" if m["Wt"] - 1 >= 4 * (m["S"] - 1) else "narrow"
    for p, want in GRID:
        if (p["prec"], p["groups"], p["S"], p["width"], p["mask"]) == (prec, m["g"], m["S"], width, m["mask"]):
            return want
    raise AssertionError("not a point of the all-on table")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CORE_CASES, ids=[case_id(c) for c in CORE_CASES])
def test_attention_core_with_every_switch_on(case, monkeypatch):
    """One row of the all-on table in one mode: forward and one backward for query, feat, Wkv, bkv, pos and table under
    ALL_ON against the float64 oracle (one keep mask over all N keys where the row has one) at the limits `judge` carries
    over; the same call with every switch unset as a control; then the launches -- exactly the entry points the table of
    tests/test_all_switches_routes_cpu.py names for this call, bevr_kv_project_w2 wherever the fused source ran, the merge
    the table names."""
    prec, row, cs = case
    ins, m = inputs(row)
    want, cot, want_g, terms = reference(row)
    want_g = {n: t * cs for n, t in want_g.items()}
    tag = case_id(case)
    M = m["S"] ** 2
    cot_dev = (cot * cs).float().to(DEV)
    if m["rows"] is not None:
        full = torch.zeros(m["B"] * m["V"], M, m["C"], device=DEV)
        full[:, m["rows"].to(DEV)] = cot_dev
        cot_dev = full
    launches = Launches(monkeypatch)
    merges = []
    for fn in ("merge_tap", "merge_views"):
        orig = getattr(ops, fn)
        monkeypatch.setattr(ops, fn, lambda *a, _o=orig, _n=fn, **kw: (merges.append(_n), _o(*a, **kw))[1])

    set_switches(monkeypatch, ALL_ON)
    how, got, grads = run_core(ins, m, prec, cot_dev)
    names, symbols, entries = launches.take()
    merged, merges[:] = list(merges), []
    figs, fails = judge(tag, prec, m, ins, got, grads, want, want_g, terms, cs)
    set_switches(monkeypatch, {})
    how0, got0, grads0 = run_core(ins, m, prec, cot_dev)
    names0, symbols0, entries0 = launches.take()
    figs0, fails0 = judge(tag + " (control)", prec, m, ins, got0, grads0, want, want_g, terms, cs)
    ran = sorted(entries & FAMILY)
    print(f"\n[{tag}] {how}: {ran} + {sorted(e for e in entries if 'kv_project' in e or 'merge' in e)}")
    for (name, r1), (_, r0) in zip(figs, figs0):
        print(f"[{tag}] {name:6s} all on {r1:6.3f}  control {r0:6.3f}  (error / carried limit)")
        RECORD.append((tag, name, r1, r0, " ".join(e.replace(A, "") for e in ran)))
    if fails0:
        print(f"[{tag}] control ({how0}: {sorted(entries0 & FAMILY)}) beyond its limits: {fails0}")

    # ---- the launches: the set the route table promises, and nothing else of the attention kernels ----
    must, merge = (WANT_X3 if prec == X3 else WANT_16)[row]
    t = table_row(prec, m)
    promised = {t["region.fwd"], t["region.bwd_q"], t["region.bwd_k"]} | (set(t["second"][3:]) if t["second"] else set())
    assert must == promised and merge == t["merge"] and how == t["source"], (tag, sorted(must ^ promised), how)
    assert entries & FAMILY == must, (tag, sorted((entries & FAMILY) ^ must))
    fused = how == "kv_source"
    # the split-weight projection under the plain form's timer name, wherever the fused source ran
    assert ("bevr_kv_project_w2" in symbols) == fused and ("bevr_kv_project" in names) == fused, (sorted(names), sorted(symbols))
    assert "bevr_kv_project" not in symbols and ("bevr_pack_kv" in entries) == (not fused)
    two_halves = t["second"] is not None
    if merge == "merge_tap":
        assert merged.count("merge_tap") == 1 and "bevr_merge_tap_fwd" in entries and "bevr_merge_tap_bwd" in entries
    else:
        assert "merge_tap" not in merged and "bevr_merge_tap_fwd" not in entries
        assert "bevr_merge_views_fwd" in entries and ("bevr_merge_views_bwd" in entries)
    assert two_halves == bool(must & (TAPS | TAPS_DROP | TAPS_X3_DROP | TAPS_G2))
    if m["mask"]:       # a run that ignored the mask cannot pass: without it the result misses the output's limit twice over
        plain = got_plain(row, prec, monkeypatch)
        off = rel_err(plain, want) / 2e-4 if prec == X3 else allclose_ratio(plain, want, **TOL[prec])
        print(f"[{tag}] without the mask: out at {off:.1f} x its limit")
        assert off > 2.0, off
    assert not fails, "\n".join(fails)


def got_plain(row, prec, monkeypatch):
    """the same inputs without a mask, forward only, under ALL_ON"""
    ins, m = inputs(row)
    set_switches(monkeypatch, ALL_ON)
    m0 = dict(m, mask=False)
    gpu = {n: t.to(DEV) for n, t in ins.items()}
    with torch.no_grad():
        if prec == X3:
            kv = F.linear(ops.sample_features(gpu["feat"].permute(0, 3, 1, 2), gpu["pos"], m["g"]), gpu["Wkv"], gpu["bkv"])
            out = ops.attention_core(gpu["query"], None, None, gpu["pos"], gpu["table"], heads=m0["h"], groups=m0["g"],
                                     views=m0["V"], precision=prec, kv=kv)
        else:
            out = ops.attention_core(gpu["query"], None, None, gpu["pos"], gpu["table"], heads=m0["h"], groups=m0["g"],
                                     views=m0["V"], precision=prec, kv_source=(gpu["feat"], gpu["Wkv"], gpu["bkv"]))
    out = out.double().cpu()
    return out if m["rows"] is None else out[:, m["rows"]]


# ---------------------------------------------------------------------------------------------------------------------
# 2. the SCA module in training mode
# ---------------------------------------------------------------------------------------------------------------------
_MODULE_ORACLE = {}

# what the module's step must launch, and what it must not, written out
GATHER_SLAB = {A + "gather_fwd", A + "gather_fwd_rows", A + "gather_fwd_x3", A + "gather_fwd_dropout", A + "slab_bwd_q",
               A + "slab_bwd_q_rows", A + "slab_bwd_q_x3", A + "slab_bwd_q_dropout", A + "slab_bwd_q_x3_dropout"}
ALL_TAPS = TAPS | TAPS_DROP | TAPS_X3_DROP | TAPS_G2
MODULE_CASES = {
    # name: (switches, precision, attn_drop_rate, the attention entry points of the step)
    "all-on-bf16-drop": (ALL_ON, BF16, 0.3, REGION("gather_fwd_dropout", "slab_bwd_q_dropout", True) | TAPS_DROP),
    "all-on-f16-drop": (ALL_ON, F16, 0.3, REGION("gather_fwd_dropout", "slab_bwd_q_dropout", True) | TAPS_DROP),
    "all-on-bf16x3-drop": (ALL_ON, X3, 0.3, REGION("fwd_dropout", "slab_bwd_q_x3_dropout", True) | TAPS_X3_DROP),
    "floor-bf16": (FLOOR, BF16, 0.0, TILE),
    "floor-bf16-drop": (FLOOR, BF16, 0.3, TILE_DROP),
    "floor-bf16x3": (FLOOR, X3, 0.0, TILE),
    "floor-bf16x3-drop": (FLOOR, X3, 0.3, TILE_DROP),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODULE_CASES))
def test_sca_module_in_training(name, monkeypatch):
    """tests/test_gpu_scatter_dropout.py::test_sca_module_in_training_takes_the_scatter_dropout_route's recipe: SpatialCrossAttn
    at S = 72 (24 x 64 features, six views), training mode, 256 sampled BEV rows; the (p, seed) draw and the per-call
    cell_order permutation captured and the kernels' mask put into the oracle's key order; O.sca_forward(keep=...) the
    reference.  Limits: out 2e-2 and _check_module_grads' classes in the 16-bit modes (tests/test_gpu_fullsize.py); bf16x3: out
    3e-4 and the f32 class, as tests/test_gpu_slab_x3_dropout.py holds its module case.
    FLOOR: sample -> F.linear -> bevr_pack_kv -> the query-tile kernels alone."""
    from bevrender_amd.model import SCA_deform_attn as SCAmod
    from bevrender_amd.model.SCA import SpatialCrossAttn
    from bevrender_amd.model.bev_cmr_proj import BEV2CameraProjector
    from test_gpu_fullsize import _check_module_grads, _randomize, ring_rig
    from test_gpu_fullsize import rel_err as rel_err_rows
    env, prec, rate, must = MODULE_CASES[name]
    set_switches(monkeypatch, env)
    S, img_w, img_h, n_rows = 72, 256, 96, 256
    D, V, Cc, h, B, Hi, Wi = 5, 6, 64, 2, 1, img_h // 4, img_w // 4
    N = (S // 2) * S * D
    T, K = ring_rig(V, img_w, img_h)
    proj = BEV2CameraProjector(imu_to_rgb={0: T}, K={0: K}, vehicle_type_code=0, img_width=img_w, img_height=img_h,
                               ori_img_width=img_w, ori_img_height=img_h, device=DEV)
    bound = {"X": 50, "Y": 50, "Z": 2}
    sca = SpatialCrossAttn(bound, proj, S, D, -1.0, Cc, h, 1, 1, 3, B, True, n_views=V, attn_drop_rate=rate, precision=prec)
    _randomize(sca, 11)
    gen = torch.Generator().manual_seed(12)
    query, x = torch.randn(B, Cc, S, S, generator=gen), torch.randn(B, V, Cc, Hi, Wi, generator=gen)
    rows = pick_rows(S, n_rows, 5)
    cot = torch.randn(B, Cc, len(rows), generator=gen)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    att = sca.spatial_deform_attn
    used_p = [n for n, _ in att.named_parameters() if not n.startswith(("proj_q", "proj_views"))]
    draws, orders = [], []
    orig_drop, orig_order = SCAmod.attention_dropout, ops.cell_order

    def spy_drop(mod):
        r = orig_drop(mod)
        draws.append(r)
        return r

    def spy_order(a, b, n_tail=0):
        r = orig_order(a, b, n_tail)
        orders.append((r.cpu(), n_tail))
        return r
    monkeypatch.setattr(SCAmod, "attention_dropout", spy_drop)
    monkeypatch.setattr(ops, "cell_order", spy_order)
    launches = Launches(monkeypatch)
    sca = sca.to(DEV).train()
    qg, xg = query.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    cot_full = torch.zeros(B, Cc, S * S, device=DEV)
    cot_full[:, :, rows.to(DEV)] = cot.to(DEV)
    torch.manual_seed(20260101)         # the draw's seed comes from torch's CPU generator
    out, _ = sca(qg, xg.reshape(B * V, Cc, Hi, Wi), torch.tensor(0), None, False)
    out.backward(cot_full.reshape(B, Cc, S, S))
    torch.cuda.synchronize()
    names, symbols, entries = launches.take()
    _, order, cs = sca.reference_points(0, qg.device)
    floor = env is FLOOR
    assert len(draws) == 1 and (draws[0] is not None) == (rate > 0)
    assert (cs == N and not orders) if floor else (0 < cs < 10000 and len(orders) == 1)

    # ---- the launches ----
    ran = entries & FAMILY
    print(f"\n[sca module {name}] {sorted(ran)} + {sorted(e for e in entries if 'kv_project' in e or 'pack_kv' in e or 'sample' in e)}")
    assert ran == must, sorted(ran ^ must)
    if floor:
        assert {"bevr_sample_fwd", "bevr_pack_kv"} <= entries and "bevr_sample_bwd" in entries
        assert not [e for e in entries | names | symbols if e.startswith("bevr_kv_project")], sorted(entries)
        assert not (GATHER_SLAB | CELL | ALL_TAPS) & (entries | names | symbols)
        assert A + "bwd_k_ws" not in symbols and "bevr_merge_tap_fwd" not in entries
    elif prec == X3:
        assert "bevr_pack_kv" in entries and not [e for e in entries if e.startswith("bevr_kv_project")]
    else:
        assert "bevr_kv_project_w2" in symbols and "bevr_kv_project" in names and "bevr_kv_project" not in symbols
        assert "bevr_pack_kv" not in entries

    # ---- the reference, with the kernels' mask in the oracle's key order ----
    keep = None
    key = (name if not floor else "floor", rate)
    if rate > 0:
        pd, sd = draws[0]
        m_k = drop_mult(sd, pd, B * V * h, S, N, rows=rows)
        keep = torch.empty_like(m_k)
        order_c = order.cpu()
        for pv in range(B * V):
            tail = cs + orders[0][0][pv] if orders else torch.arange(0)
            keep[pv * h:(pv + 1) * h][:, :, order_c[pv % V][torch.cat((torch.arange(cs), tail))]] = m_k[pv * h:(pv + 1) * h]
        del m_k
        key = key + (sd,)
    if key not in _MODULE_ORACLE:       # shared by the cases with the same draw and key order (FLOOR: bf16 and bf16x3)
        pw = {k_: v_.detach().cpu().clone().double().requires_grad_(k_ in used_p) for k_, v_ in att.state_dict().items()}
        qc, xc = query.clone().double().requires_grad_(True), x.clone().double().requires_grad_(True)
        pts = O.sample_3d_points(bound, S, D, -1.0)
        ref = O.sca_reference_points(O.bev_grid_to_camera(pts, T, K, img_w, img_h, img_w, img_h), B).double()
        want = O.sca_forward(pw, xc, qc, ref, n_heads=h, depth_dim=D, rows=rows, keep=keep)
        (want * cot.double()).sum().backward()
        wnt = {n: pw[n].grad for n in used_p}
        wnt.update({"in.query": qc.grad, "in.x": xc.grad})
        _MODULE_ORACLE[key] = (want.detach(), wnt)
    want, wnt = _MODULE_ORACLE[key]
    e = rel_err_rows(out.detach().reshape(B, Cc, S * S)[:, :, rows.to(DEV)].cpu(), want)
    lim_out = {BF16: 2e-2, F16: 2e-2, X3: 3e-4}[prec]
    print(f"[sca module {name}] out rel err {e:.3e} (limit {lim_out:.0e})")
    got = {n: prm.grad for n, prm in att.named_parameters()}
    got.update({"in.query": qg.grad, "in.x": xg.grad})
    code = {BF16: 1, F16: 2, X3: 0}[prec]       # _check_module_grads' classes; its limits restated for the record alone
    lim_g, lim_off = {0: 3e-3, 1: 6e-2, 2: 1e-2}[code], {0: 1.5e-2, 1: 6e-2, 2: 2e-2}[code]
    worst = max(rel_err_rows(got[n].cpu(), w) / (lim_off if "conv_offset" in n else lim_g)
                for n, w in wnt.items() if not n.endswith("proj_k.bias"))
    RECORD.append((f"sca module {name}", "out", e / lim_out, float("nan"), " ".join(x_.replace(A, "") for x_ in sorted(ran))))
    RECORD.append((f"sca module {name}", "worst parameter / input gradient", worst, float("nan"), ""))
    assert e < lim_out, f"out: {e:.3e}"
    _check_module_grads(f"sca module {name}", got, wnt, code)


@pytest.mark.gpu
def test_sca_module_with_two_groups_and_every_switch_on(monkeypatch):
    """tests/test_gpu_tap_groups.py::test_sca_module_with_two_groups_on_the_pinned_route, its seed-0 case (S = 32, D = 5, more
    than 1 024 pinned keys per view) in bf16 under ALL_ON, no dropout: the two-group tap kernels beside the gather forward,
    the slab bwd_q and the split-weight projection with two groups.  That test's comparison (compare)."""
    from bevrender_amd.model.SCA_deform_attn import SCADeformableAttention
    from test_gpu_random_sweep_modules import compare, randomize_
    from test_gpu_tap_groups import _module_case
    set_switches(monkeypatch, ALL_ON)
    seed, prec = 0, BF16
    hh, C, S, D, V, B, Hi, Wi, frac = _module_case(seed)
    Hk, Wk = S // 2, S * D
    gen = torch.Generator().manual_seed(seed)
    query = torch.randn(B, C, S, S, generator=gen)
    x = torch.randn(B, V, C, Hi, Wi, generator=gen)
    ref_v = torch.rand(V, Hk, Wk, 2, generator=gen) * 2.4 - 1.2
    n_pin = int(Hk * Wk * frac)
    ref_v.view(V, Hk * Wk, 2)[:, :n_pin] = -1.0
    ref = ref_v[None].expand(B, -1, -1, -1, -1)
    yx = ref_v.reshape(V, -1, 2)[..., (1, 0)].double().numpy()
    order, split = ops.split_key_order(yx, S, 2 * S * D - 1, min_cell_keys=64)
    assert Hk * Wk - split > 1024
    mod = SCADeformableAttention(bev_feat_shape=S, bev_depth_dim=D, dim_embed=C, n_heads=hh, n_groups=2, stride=1,
                                 kernel_size=3, scale_offset_range=True, batch_size=B, n_views=V, precision=prec).to(DEV)
    randomize_(mod, 2500 + seed)
    assert mod._pinned_keys_tap(S, Hi, Wi)
    p_cpu = {n: v.detach().cpu().double().requires_grad_(True) for n, v in mod.state_dict().items()}
    qc, xc = query.double().requires_grad_(True), x.double().requires_grad_(True)
    want = O.sca_forward(p_cpu, xc, qc, ref.double(), n_heads=hh, n_groups=2, depth_dim=D, scale_offset_range=True)
    qg, xg = query.clone().to(DEV).requires_grad_(True), x.clone().to(DEV).requires_grad_(True)
    launches = Launches(monkeypatch)
    out, _ = mod(xg, qg, ref.to(DEV), None, False, key_order=order.to(DEV), cell_split=split, split_is_pinned=True)
    tag = f"sca g2 all on C{C} h{hh} S{S} D{D} V{V} B{B} {Hi}x{Wi} split {split}"
    compare(mod, out, want, (qg, xg), (qc, xc), p_cpu, tag, bf16=True)
    names, symbols, entries = launches.take()
    ran = entries & FAMILY
    print(f"\n[{tag}] {sorted(ran)}")
    RECORD.append((tag, "compare() of tests/test_gpu_random_sweep_modules.py", float("nan"), float("nan"),
                   " ".join(x_.replace(A, "") for x_ in sorted(ran))))
    assert ran == REGION("gather_fwd", "slab_bwd_q") | TAPS_G2, sorted(ran)
    assert "bevr_kv_project_w2" in symbols and "bevr_kv_project" in names and "bevr_kv_project" not in symbols


# ---------------------------------------------------------------------------------------------------------------------
# 3. the whole model
# ---------------------------------------------------------------------------------------------------------------------
REGION_16 = {A + "gather_fwd", A + "slab_bwd_q", A + "bwd_k"}
X3_ENTRIES = {A + "gather_fwd_x3", A + "slab_bwd_q_x3"}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_full_bevrender_with_every_switch_on(mode, monkeypatch):
    """tests/test_gpu_kv_wsplit.py::test_full_bevrender_with_split_weights under ALL_ON, on the fixture whose projection
    weights are off the bf16 grid (tests/golden/full_bevrender_cond_w.npz): its procedure, its limits (output
    max(2e-3, 3 s_out), every gradient max(2e-2, 3 s)), its launches."""
    from test_gpu_kv_wsplit import _whole_model
    set_switches(monkeypatch, {})
    launched, e_out, lim_out, rows = _whole_model(mode, monkeypatch, True, env=ALL_ON)
    print(f"[all on {mode}] launched: {sorted(launched)}")
    print("\n".join(r[1] for r in rows))
    print(f"[all on {mode}] out {e_out:.3e} limit {lim_out:.3e}; beyond their limit {sum(not r[0] for r in rows)}")
    worst = max(r[2] / r[3] for r in rows)
    RECORD.append((f"whole model {mode}", "out", e_out / lim_out, float("nan"),
                   " ".join(sorted(x_.replace(A, "") for x_ in launched if x_.startswith(A)))))
    RECORD.append((f"whole model {mode}", "worst parameter gradient", worst, float("nan"), ""))
    assert REGION_16 | TAPS | {"bevr_kv_project_w2", "bevr_kv_project"} <= launched, sorted(launched)
    assert not (CELL | X3_ENTRIES | TAPS_G2 | TILE_DROP) & launched, sorted(launched)
    assert e_out <= lim_out, (mode, e_out, lim_out)
    bad = [r[1] for r in rows if not r[0]]
    assert not bad, f"{mode}: {len(bad)} gradients beyond their limit, in backward order:\n" + "\n".join(bad)


@pytest.mark.gpu
def test_full_bevrender_bf16x3_with_every_switch_on(monkeypatch):
    """tests/test_gpu_full_model.py::test_full_bevrender_conditioned, mode bf16x3-split, under ALL_ON
    (tests/golden/full_bevrender_cond.npz): its procedure, limits and assertions."""
    from bevrender_amd.model.bevrender import BEVRender
    from test_gpu_full_model import _cond_fixture, _gen
    g, z = _gen(), _cond_fixture()
    set_switches(monkeypatch, ALL_ON)
    launched = set()

    def recorder(name, flops, fn, *args, nbytes=0.0, tag=""):
        launched.update((name, getattr(fn, "__name__", repr(fn))))
        return fn(*args)
    monkeypatch.setattr(ops.KERNEL_TIMER, "run", recorder)
    cfg = g.cond_config()
    cfg["PRECISION"], cfg["STAGE_DTYPE"] = "bf16x3", None
    torch.manual_seed(int(z["seed"]))
    model = BEVRender(cfg, logging.getLogger("t"), "train")
    g.condition_(model.state_dict())
    assert len(model.state_dict()) == int(z["n_state"])
    model = model.to("cuda")
    img, pose, vtype = g.full_inputs()
    out, _ = model(img.cuda(), pose.cuda(), vtype.cuda(), {}, False)
    assert tuple(out.shape) == tuple(z["out_shape"])
    (out.float() * g.cond_cotangent(out.shape).cuda()).sum().backward()
    torch.cuda.synchronize()
    got = out.detach().float().flatten().cpu()[torch.tensor(z["out_idx"])].numpy()
    params = dict(model.named_parameters())
    missing = [n for n in z["names"] if n not in params or params[n].grad is None]
    assert not missing, missing
    rows = []
    for i, n in enumerate(z["names"]):
        v = params[n].grad.detach().float().flatten().cpu()[torch.tensor(z["idx"][i])].numpy()
        if z["null"][i]:
            err, lim, what = float(np.linalg.norm(v.astype(np.float64))), 10.0 * float(z["null_bound"][i]), "null |g|"
        else:
            err, lim, what = g.rel2(v, z["val"][i]), max(2e-2, 3.0 * float(z["s_f32"][i])), "rel"
        rows.append((err <= lim, f"  {i:3d} {n:90s} {what:8s} {err:.3e} limit {lim:.3e}{'' if err <= lim else '  FAIL'}", err, lim))
    emb = rows[z["names"].index("bev_embedding.weight")]
    print(f"[all on bf16x3] launched: {sorted(launched)}")
    print("\n".join(r[1] for r in rows))
    RECORD.append(("whole model bf16x3", "out (2-norm, for the record)", g.rel2(got, z["out_val"]) / 2e-3, float("nan"),
                   " ".join(sorted(x_.replace(A, "") for x_ in launched if x_.startswith(A)))))
    RECORD.append(("whole model bf16x3", "worst parameter gradient", max(r[2] / r[3] for r in rows), float("nan"), ""))
    assert X3_ENTRIES | TAPS | {A + "bwd_k"} <= launched, sorted(launched)
    assert not (CELL | TAPS_X3_DROP | TILE_DROP | {"bevr_kv_project", "bevr_kv_project_w2"}) & launched, sorted(launched)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, z["out_val"], rtol=2e-3, atol=2e-3 * np.abs(z["out_val"]).max())
    nonfinite = [n for n, p in params.items() if p.grad is not None and not torch.isfinite(p.grad).all()]
    assert not nonfinite, nonfinite
    assert emb[3] <= 0.18
    bad = [r[1] for r in rows if not r[0]]
    assert not bad, f"bf16x3: {len(bad)} gradients beyond their limit, in backward order:\n" + "\n".join(bad)


def teardown_module(module):
    if not RECORD:
        return
    print("\n\n==== every opt-in switch on: error / carried limit (all on | control: every switch unset) ====")
    print(f"{'case':44s} {'quantity':32s} {'all on':>8s} {'control':>8s}  launched")
    for case, quantity, r1, r0, ran in RECORD:
        c0 = "" if r0 != r0 else f"{r0:8.3f}"
        c1 = "" if r1 != r1 else f"{r1:8.3f}"
        print(f"{case:44s} {quantity:32s} {c1:>8s} {c0:>8s}  {ran}")
