"""Attention dropout (reference model/SCA_deform_attn.py:155-156,402-409,420; model/TSA_deform_attn.py:90-91,323,336).

The kernels do not store a mask: the keep decision of a (problem-head, query, key) pair is a hash of (seed, ph, mq, n)
(csrc/bevr_common.h:bevr_drop_keep) evaluated alike in the forward and in both backward kernels.  The tests rebuild that
mask on the host (ops.dropout_keep_mask), hand it to the oracle's materialised attention as the multiplier nn.Dropout
applies (0 or 1 / (1 - p)) and compare forward and every gradient."""
import os

import numpy as np
import pytest
import torch

from bevrender_amd import _lib, ops
from oracle import bevrender_oracle as O
from test_gpu_fullsize import LIMITS, check_dpos, kink_distance, oracle_rows, pick_rows
from test_gpu_ops import CORE_CFGS, GRAD_LIM, TOL, _core_problem, rel_err
from test_gpu_random_sweep_routes import OUT_LIM, POS_LIM, UNIT, gradient_terms

DEV = "cuda"


def test_keep_mask_is_a_pure_function_with_the_requested_rate():
    thr = int(round(0.3 * 65536))
    a = ops.dropout_keep_mask(77, thr, 4, 12, 500)
    b = ops.dropout_keep_mask(77, thr, 4, 12, 500)
    c = ops.dropout_keep_mask(78, thr, 4, 12, 500)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert abs(a.float().mean().item() - 0.7) < 5e-3
    # no structure along any axis: per problem-head, per query and per key the rate holds
    for dim in ((1, 2), (0, 2), (0, 1)):
        assert (a.float().mean(dim) - 0.7).abs().max().item() < 0.08


def _oracle_core_drop(query, k, v, pos, table, h, g, V, keep):
    B, C, S, _ = query.shape
    c = C // h
    Bp, N, _ = k.shape
    outs = []
    for bp in range(Bp):
        q = query[bp // V].reshape(h, c, S * S)
        kk = k[bp].reshape(N, h, c).permute(1, 2, 0)
        vv = v[bp].reshape(N, h, c).permute(1, 2, 0)
        o = O.attention_core(q, kk, vv, pos[bp * g:(bp + 1) * g], table, S, S, g, c ** -0.5, keep=keep[bp * h:(bp + 1) * h])
        outs.append(o.reshape(C, S * S).t())
    return torch.stack(outs, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [_lib.PREC_F32, _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16])
@pytest.mark.parametrize("cfg", [CORE_CFGS[1], CORE_CFGS[4], CORE_CFGS[5]])
def test_attention_core_with_dropout_matches_the_oracle_with_the_same_mask(cfg, prec):
    B, V, C, h, g, S, D, N = cfg
    p, seed = 0.3, 0x5eed1234
    thr = int(round(p * 65536))
    query, k, v, pos, table = _core_problem(B, V, C, h, g, S, D, N, seed=sum(cfg))
    keep = ops.dropout_keep_mask(seed, thr, B * V * h, S, N).to(torch.float32) * (65536.0 / (65536.0 - thr))
    ins_cpu = [t.clone().requires_grad_(True) for t in (query, k, v, pos, table)]
    want = _oracle_core_drop(*ins_cpu, h, g, V, keep)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(1))
    want.backward(cot)
    ins_gpu = [t.clone().to(DEV).requires_grad_(True) for t in (query, k, v, pos, table)]
    got = ops.attention_core(*ins_gpu, heads=h, groups=g, views=V, precision=prec, attn_drop=(p, seed))
    got.backward(cot.to(DEV))
    torch.cuda.synchronize()
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().numpy(), **TOL[prec])
    for n, a, b in zip(["query", "k", "v", "pos", "table"], ins_gpu, ins_cpu):
        e = rel_err(a.grad.cpu(), b.grad)
        assert e < GRAD_LIM[prec], f"grad {n}: rel err {e:.3e}"
    # and the mask did something: without it the output differs
    plain = ops.attention_core(*[t.detach() for t in ins_gpu], heads=h, groups=g, views=V, precision=prec)
    assert rel_err(plain.cpu(), want.detach()) > 0.05


@pytest.mark.gpu
def test_modules_accept_dropout_rates_and_apply_them_in_training_mode_only():
    from bevrender_amd.model.SCA_deform_attn import SCADeformableAttention
    from bevrender_amd.model.TSA_deform_attn import TSADeformableAttention
    torch.manual_seed(3)
    B, C, h, S, D, Hi, Wi = 2, 64, 2, 12, 3, 8, 20
    mods = [TSADeformableAttention(S, C, h, 1, 1, 3, True, B, n_views=1, attn_drop_rate=0.2, proj_drop_rate=0.1,
                                   precision=_lib.PREC_F32).to(DEV),
            SCADeformableAttention(S, D, C, h, 1, 1, 3, True, B, n_views=2, attn_drop_rate=0.2, proj_drop_rate=0.1,
                                   precision=_lib.PREC_F32).to(DEV)]
    plain = [TSADeformableAttention(S, C, h, 1, 1, 3, True, B, n_views=1, precision=_lib.PREC_F32).to(DEV),
             SCADeformableAttention(S, D, C, h, 1, 1, 3, True, B, n_views=2, precision=_lib.PREC_F32).to(DEV)]
    q = torch.randn(B, C, S, S, device=DEV, requires_grad=True)
    prev = torch.randn(B, C, S, S, device=DEV)
    x = torch.randn(B, 2, C, Hi, Wi, device=DEV)
    ref = (torch.rand(1, 2, S // 2, S * D, 2, device=DEV) * 2.2 - 1.1).expand(B, -1, -1, -1, -1).contiguous()
    for m, pm, args in ((mods[0], plain[0], (prev, q, {}, False)), (mods[1], plain[1], (x, q, ref, {}, False))):
        with torch.no_grad():
            for t in m.parameters():
                t.copy_(torch.randn_like(t) * 0.1)
        pm.load_state_dict(m.state_dict())
        m.train()
        a, _ = m(*args)
        b, _ = m(*args)
        assert torch.isfinite(a).all() and not torch.allclose(a, b)          # a fresh mask per call
        a.square().mean().backward()
        assert torch.isfinite(q.grad).all() and m.rpe_table.grad.abs().sum() > 0
        m.eval()
        pm.eval()
        e, _ = m(*args)
        w, _ = pm(*args)
        assert torch.allclose(e, w, rtol=1e-5, atol=1e-6)                   # eval mode: dropout is the identity
        # training-mode output is an unbiased estimate of the plain one: the mean over many masks approaches it
        m.train()
        acc = torch.zeros_like(w)
        for _ in range(48):
            acc += m(*args)[0].detach()
        assert rel_err(acc / 48, w.detach()) < 0.35


# ---- scales at high drop rates -----------------------------------------------------------------------------------------
# With dropout the kernels form dS = P (D dP - delta) and the dV operand D P', D = 1 / (1 - p): the backward's scales
# (ops.backward_scales, include/bevrender_hip.h grad_scale) must count D Pmax, or a fixed-point table-gradient
# contribution passes 2^31 (clamped by the 32-bit round-to-integer) and fp16's D P' passes 65504; the fp16 forward must
# not multiply its weights (up to 2^12 there) by D before the PV product.
STRESS_P = [0.5, 0.75, 0.9, 0.97, 0.99]
ALL_PREC = [_lib.PREC_F32, _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16]


def drop_mult(seed, p, n_ph, S, N, rows=None):
    """the oracle's multiplier: keep / (1 - p) with p rounded to 1/65536 as the kernels round it; (n_ph, M, N) float64
    (rows: the (n_ph, len(rows), N) rows of it)."""
    thr = int(round(p * 65536))
    return ops.dropout_keep_mask(seed, thr, n_ph, S, N, rows=rows).double() * (65536.0 / (65536.0 - thr))


@pytest.mark.gpu
@pytest.mark.parametrize("p", STRESS_P)
@pytest.mark.parametrize("prec", ALL_PREC)
def test_dropout_high_rates_one_dominant_key_per_row(prec, p):
    """(a) Random keys, the query scaled so that one key dominates each row (Pmax ~ 1): the fp16 operands D P' and the
    forward's weights sit at the top of their range.  Forward and every gradient against float64 with the exact mask."""
    B, V, C, h, g, S, D, N = 1, 1, 64, 2, 1, 12, 3, 96
    query, k, v, pos, table = _core_problem(B, V, C, h, g, S, D, N, seed=77)
    query = query * 12.0                # logits spread ~12: the largest weight of a row is ~1
    seed = 0x51ce + int(p * 1000)
    keep = drop_mult(seed, p, B * V * h, S, N)
    ins_cpu = [t.clone().double().requires_grad_(True) for t in (query, k, v, pos, table)]
    want = _oracle_core_drop(*ins_cpu, h, g, V, keep)
    # the premise: rows are dominated by one key
    with torch.no_grad():
        q = ins_cpu[0][0].reshape(h, C // h, S * S)
        kk = ins_cpu[1][0].reshape(N, h, C // h).permute(1, 2, 0)
        pl = torch.softmax(torch.einsum("bcm,bcn->bmn", q, kk) * (C // h) ** -0.5, -1)
        assert pl.amax(-1).median().item() > 0.9
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    want.backward(cot)
    ins_gpu = [t.clone().to(DEV).requires_grad_(True) for t in (query, k, v, pos, table)]
    got = ops.attention_core(*ins_gpu, heads=h, groups=g, views=V, precision=prec, attn_drop=(p, seed))
    got.backward(cot.float().to(DEV))
    torch.cuda.synchronize()
    tag = f"p={p} prec={prec}"
    e = rel_err(got.detach().cpu().double(), want.detach())
    assert e < OUT_LIM[prec], f"{tag}: out {e:.3e}"
    terms = gradient_terms(ins_cpu, cot, h, g, V, keep=keep, keys=True)
    for n, a, b in zip(["query", "k", "v", "pos", "table"], ins_gpu, ins_cpu):
        a, b = a.grad.cpu().double(), b.grad
        assert torch.isfinite(a).all(), f"{tag}: grad {n} not finite"
        if n == "pos":
            clean = kink_distance(pos, S, 2 * S * D - 1) >= 1e-4
            dg, dw = a[clean], b[clean]
            ep = (dg - dw).norm().item() / max(dw.norm().item(), 1e-30)
            assert ep < POS_LIM[prec], f"{tag}: grad pos 2-norm {ep:.3e}"
            continue
        scale = b.abs().max().item()
        if n in ("table", "query", "k"):
            # one key per row near P = 1: D dP - delta cancels there, the 16-bit roundings apply to the terms
            bound = 2.0 * UNIT[prec] * terms[("table", "query", "k").index(n)] + GRAD_LIM[prec] * scale
            worst = ((a - b).abs() / bound).max().item()
            assert worst < 1.0, f"{tag}: grad {n} {worst:.2f} x its term bound"
            continue
        e = (a - b).abs().max().item() / scale
        assert e < GRAD_LIM[prec], f"{tag}: grad {n} {e:.3e}"


def _both_kept_seed(p, h, S, start):
    """a dropout seed under which some (head, query) rows keep both of N = 2 keys."""
    for seed in range(start, start + 200000):
        m = ops.dropout_keep_mask(seed, int(round(p * 65536)), h, S, 2)
        both = m.all(-1)
        if both.sum().item() >= 1:
            return seed, both
    raise AssertionError("no seed found")


@pytest.mark.gpu
@pytest.mark.parametrize("p", STRESS_P)
@pytest.mark.parametrize("prec", ALL_PREC)
def test_dropout_high_rates_meet_the_scale_bound_exactly(prec, p):
    """(b) A problem at the bound of the backward's scales: N = 2 equal K rows and a zero table (P = 1/2 exactly), V rows
    +v e and -v e, the cotangent e on the rows where the mask keeps both keys (0 elsewhere).  Then delta = 0 wherever
    dO != 0 and |P (D dP - delta)| = D Pmax bound: every fixed-point table-gradient contribution of key 0 (a table grid
    point: one tap of weight 1) is D times the largest the scales allow without dropout.  Key 1 sits between grid points
    in both axes (four taps of weight 1/4): with rx = ry = 1 some of its taps for one query share a cell with key 0's
    tap for another and carry the opposite sign, so the cell SUMS partly cancel -- but each contribution is rounded to
    32 bits on its own before it is added to its cell, so one of key 0's past 2^31 is clamped whatever the cell's sum,
    and the cells key 1 does not reach hold key 0's contributions alone.  d(table), dK and dV against float64; dQ
    (sum_n dS_n K_n with dS_0 = -dS_1) and d(pos) (zero table) are zero."""
    B, V, C, h, g, S, D, N = 1, 1, 64, 2, 1, 9, 1, 2
    c = C // h
    gen = torch.Generator().manual_seed(5)
    query = torch.randn(B, C, S, S, generator=gen)
    k = torch.randn(1, 1, C, generator=gen).expand(1, N, C).contiguous()
    unit = torch.zeros(C)
    unit[::c] = 1.0                                      # channel 0 of every head: a unit vector per head
    vnorm = 1.9                                          # just under 2: s Pmax bound lands just under 2^30
    v = torch.stack((vnorm * unit, -vnorm * unit))[None]
    # table coordinates (1 - y)(S - 1)/2, (1 - x)(Wt - 1)/4 = 4 (1 - y), 4 (1 - x): key 0 on the grid point (2, 2), key 1
    # at (5.5, 4.5)
    pos = torch.tensor([[[0.5, 0.5], [-0.375, -0.125]]])
    table = torch.zeros(h, 2 * S - 1, 2 * S * D - 1)
    seed, both = _both_kept_seed(p, h, S, 0x7e57 + int(p * 100000))
    keep = drop_mult(seed, p, B * V * h, S, N)
    cot = torch.zeros(B * V, S * S, C, dtype=torch.float64)
    for hh in range(h):
        cot[0, both[hh], hh * c] = 1.0
    ins_cpu = [t.clone().double().requires_grad_(True) for t in (query, k, v, pos, table)]
    want = _oracle_core_drop(*ins_cpu, h, g, V, keep)
    want.backward(cot)
    ins_gpu = [t.clone().to(DEV).requires_grad_(True) for t in (query, k, v, pos, table)]
    got = ops.attention_core(*ins_gpu, heads=h, groups=g, views=V, precision=prec, attn_drop=(p, seed))
    got.backward(cot.float().to(DEV))
    torch.cuda.synchronize()
    tag = f"p={p} prec={prec}"
    e = rel_err(got.detach().cpu().double(), want.detach())
    assert e < OUT_LIM[prec], f"{tag}: out {e:.3e}"
    grads = {n: a.grad.cpu().double() for n, a in zip(["query", "k", "v", "pos", "table"], ins_gpu)}
    for n in grads:
        assert torch.isfinite(grads[n]).all(), f"{tag}: grad {n} not finite"
    for n, b in (("k", ins_cpu[1].grad), ("v", ins_cpu[2].grad), ("table", ins_cpu[4].grad)):
        err = (grads[n] - b).abs().max().item() / b.abs().max().item()
        assert err < GRAD_LIM[prec], f"{tag}: grad {n} {err:.3e}"
    ref = ins_cpu[1].grad.abs().max().item()
    assert ref > 0 and ins_cpu[4].grad.abs().max().item() > 0
    for n in ("query", "pos"):
        assert grads[n].abs().max().item() < 1e-5 * ref, f"{tag}: grad {n} {grads[n].abs().max().item():.3e}"


MODULE_CASES = [(p, False) for p in ALL_PREC] + [(_lib.PREC_BF16, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec,pinned", MODULE_CASES, ids=[f"prec{p}" + ("-pinned" if q else "") for p, q in MODULE_CASES])
def test_modules_with_dropout_match_the_oracle_with_the_exact_mask(prec, pinned, monkeypatch):
    """TSA and SCA in training mode with attn_drop_rate > 0 (proj_drop_rate = 0) against the oracle's module forwards
    with the exact mask: the (p, seed) each module draws is captured, the kernels' mask rebuilt on the host and put in
    the oracle's key order (TSA: its static k-d order; SCA: per view, ph = (b V + v) h + head).  SCA with
    split_is_pinned=True and a cell split: dropout keeps every key on the region kernels.  Output and d(table)."""
    from bevrender_amd.model import SCA_deform_attn as SCAmod, TSA_deform_attn as TSAmod
    torch.manual_seed(3)
    B, C, h, S, D, Hi, Wi, V = 2, 64, 2, 12, 3, 8, 20, 2
    tsa = TSAmod.TSADeformableAttention(S, C, h, 1, 1, 3, True, B, n_views=1, attn_drop_rate=0.3, precision=prec)
    sca = SCAmod.SCADeformableAttention(S, D, C, h, 1, 1, 3, True, B, n_views=V, attn_drop_rate=0.4, precision=prec)
    for mod in (tsa, sca):
        with torch.no_grad():
            for t in mod.parameters():
                t.copy_(torch.randn_like(t) * (0.1 if t.ndim > 1 else 0.05))
    draws = []
    for modname in (TSAmod, SCAmod):
        orig = modname.attention_dropout

        def spy(m, _orig=orig):
            r = _orig(m)
            draws.append(r)
            return r
        monkeypatch.setattr(modname, "attention_dropout", spy)
    q, prev = torch.randn(B, C, S, S), torch.randn(B, C, S, S)
    x = torch.randn(B, V, C, Hi, Wi)
    ref = (torch.rand(1, V, S // 2, S * D, 2) * 2.2 - 1.1).expand(B, -1, -1, -1, -1).contiguous()
    p_t = {k: t.detach().double().clone().requires_grad_(k == "rpe_table") for k, t in tsa.state_dict().items()}
    p_s = {k: t.detach().double().clone().requires_grad_(k == "rpe_table") for k, t in sca.state_dict().items()}
    tsa, sca = tsa.to(DEV).train(), sca.to(DEV).train()
    ops.KERNEL_TIMER.start()
    got_t, _ = tsa(prev.to(DEV), q.to(DEV), {}, False)
    N_s = (S // 2) * S * D
    kw = dict(cell_split=N_s // 2, split_is_pinned=True) if pinned else {}
    got_s, _ = sca(x.to(DEV), q.to(DEV), ref.to(DEV), {}, False, **kw)
    cot_t = torch.randn(got_t.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    cot_s = torch.randn(got_s.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    ((got_t * cot_t.float().to(DEV)).sum() + (got_s * cot_s.float().to(DEV)).sum()).backward()
    used = set(ops.KERNEL_TIMER.stop())
    assert len(draws) == 2 and all(d is not None for d in draws), draws
    for k in ("bevr_attn_fwd_dropout", "bevr_attn_bwd_q_dropout", "bevr_attn_bwd_k_dropout"):
        assert k in used, sorted(used)
    assert not {n for n in used if n.startswith(("bevr_attn_cell", "bevr_attn_tap", "bevr_attn_gather", "bevr_attn_slab"))}, \
        sorted(used)
    assert not {"bevr_attn_fwd", "bevr_attn_bwd_q", "bevr_attn_bwd_k"} & used, sorted(used)

    # TSA: kernel key nk is the oracle's key order[nk] (the module's static k-d order of the S x S key grid)
    (pt, st), (ps, ss) = draws
    N_t = S * S
    m_t = drop_mult(st, pt, B * h, S, N_t)
    order = tsa._key_order(S, S, "cpu")
    keep_t = torch.empty_like(m_t)
    keep_t[..., order] = m_t
    keep_s = drop_mult(ss, ps, B * V * h, S, N_s)           # SCA without key_order: the oracle's key order
    want_t = O.tsa_forward(p_t, q.double(), prev.double(), n_heads=h, keep=keep_t)
    want_s = O.sca_forward(p_s, x.double(), q.double(), ref.double(), n_heads=h, depth_dim=D, keep=keep_s)
    ((want_t * cot_t).sum() + (want_s * cot_s).sum()).backward()
    out_lim = {_lib.PREC_F32: 3e-4, _lib.PREC_BF16X3: 3e-4, _lib.PREC_BF16: 3e-2, _lib.PREC_F16: 6e-3}[prec]
    with torch.no_grad():
        plain_t = O.tsa_forward(p_t, q.double(), prev.double(), n_heads=h)
        plain_s = O.sca_forward(p_s, x.double(), q.double(), ref.double(), n_heads=h, depth_dim=D)
    for name, got, want, plain, mod, ps_ in (("tsa", got_t, want_t, plain_t, tsa, p_t),
                                             ("sca", got_s, want_s, plain_s, sca, p_s)):
        e = rel_err(got.detach().cpu().double(), want.detach())
        assert e < out_lim, f"{name}: out {e:.3e}"
        assert rel_err(got.detach().cpu().double(), plain) > 0.05, f"{name}: the mask changed nothing"
        eg = rel_err(mod.rpe_table.grad.cpu().double(), ps_["rpe_table"].grad)
        assert eg < GRAD_LIM[prec], f"{name}: grad rpe_table {eg:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [_lib.PREC_BF16, _lib.PREC_F16])
def test_dropout_tsa_geometry_bev200_rows_and_gradients(prec):
    """The S = 200 TSA launch of tests/test_gpu_fullsize.py test_tsa_geometry_bev200_rows_and_gradients with attention
    dropout: N = 40 000 keys on the regular grid in the static k-d order, table 399 x 399, 7 row blocks per BEV column,
    Pmax far below 1 -- what training with attn_drop_rate > 0 launches (the region kernels with the mask, not the gather
    forward / slab backward the plain call takes).  256 query rows against the float64 oracle with the kernels' mask on
    those rows (dropout_keep_mask(rows=): the host mask stays (h, R, N)); forward and every gradient at the fullsize
    limits."""
    S, C, h, p = 200, 64, 2, 0.3
    gen = torch.Generator().manual_seed(200)
    grid = O.normalized_grid(S, S, torch.float32).reshape(1, -1, 2)
    N = S * S
    pos = grid + torch.tanh(torch.randn(1, N, 2, generator=gen)) * (0.5 / (S - 1.0))
    order = torch.from_numpy(ops.kd_key_order(grid[0].double().numpy(), S, 2 * S - 1))
    pr = dict(query=torch.randn(1, C, S, S, generator=gen), k=torch.randn(1, N, C, generator=gen),
              v=torch.randn(1, N, C, generator=gen), pos=pos[:, order].contiguous(),
              table=torch.randn(h, 2 * S - 1, 2 * S - 1, generator=gen) * 0.3)
    rows = pick_rows(S, 256, 3)
    cot = torch.randn(1, len(rows), C, generator=torch.Generator().manual_seed(7))
    seed = 0xb200 + prec
    # keys in the order the caller passes them (here the k-d order): the kernels' key index
    keep = drop_mult(seed, p, h, S, N, rows=rows)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    want, grads = oracle_rows(pr, h, rows, cot, keep=keep)
    ins = {n: pr[n].clone().to(DEV).requires_grad_(True) for n in ("query", "k", "v", "pos", "table")}
    ops.KERNEL_TIMER.start()
    out = ops.attention_core(ins["query"], ins["k"], ins["v"], ins["pos"], ins["table"], heads=h, groups=1, views=1,
                             precision=prec, attn_drop=(p, seed))
    cot_full = torch.zeros_like(out)
    cot_full[:, rows.to(DEV)] = cot.to(DEV)
    out.backward(cot_full)
    used = set(ops.KERNEL_TIMER.stop())
    for k in ("bevr_attn_fwd_dropout", "bevr_attn_bwd_q_dropout", "bevr_attn_bwd_k_dropout"):
        assert k in used, sorted(used)
    assert not {"bevr_attn_fwd", "bevr_attn_gather_fwd", "bevr_attn_bwd_q", "bevr_attn_slab_bwd_q", "bevr_attn_bwd_k"} & used
    lim = LIMITS[prec]
    tag = f"tsa S=200 dropout p={p} prec={prec}"
    e = rel_err(out.detach()[:, rows.to(DEV)].cpu().double(), want)
    print(f"\n[{tag}] out rel err {e:.3e}")
    assert e < lim["out"], f"{tag}: out {e:.3e}"
    for n in ("query", "k", "v", "table"):
        e = rel_err(ins[n].grad.cpu().double(), grads[n])
        print(f"[{tag}] grad {n:6s} rel err {e:.3e}")
        assert e < lim[n], f"{tag}: grad {n} {e:.3e}"
    check_dpos(ins["pos"].grad, grads["pos"], pr["pos"], S, 2 * S - 1, lim["pos"], tag, cols=(rows % S).tolist(),
               min_clean=0.3)
