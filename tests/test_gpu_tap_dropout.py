"""Attention dropout on the tap kernels (csrc/attn_tap_*_drop.hip): the projector-pinned keys keep their segment when
DAT_ATTN_DROP_RATE > 0.

Four levels: the three dropout entry points against a float64 restatement of their definition with the host twin of the
keep mask (tools/tap_drop_check.py); the host path ops.attention_core(tap_source=True, attn_drop=...) -- region dropout
kernels on the scattered keys, tap dropout kernels on the pinned ones, ONE mask over all keys -- against the oracle's
materialised attention with that mask; the same call on the all-region route; and SCADeformableAttention in training mode."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bevrender_amd import _lib, ops
from oracle import bevrender_oracle as O
from test_gpu_dropout import STRESS_P, drop_mult
from test_gpu_ops import GRAD_LIM
from test_gpu_tap import KERNEL_CASES, TAP_CFGS, _tap_problem, rel_err

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAP_DROP = ("bevr_attn_tap_fwd_dropout", "bevr_attn_tap_bwd_q_dropout", "bevr_attn_tap_bwd_k_dropout")
REGION_DROP = ("bevr_attn_fwd_dropout", "bevr_attn_bwd_q_dropout", "bevr_attn_bwd_k_dropout")
TAP_PLAIN = ("bevr_attn_tap_fwd", "bevr_attn_tap_bwd_q", "bevr_attn_tap_bwd_k")


@pytest.mark.parametrize("name", ["sorted", "ragged", "unsorted_wide", "three_row_blocks", "fp16", "two_blocks_per_wave",
                                  "four_blocks_per_wave"])
def test_tap_dropout_entry_points_match_their_float64_definition(name):
    """The cases and limits of tests/test_gpu_tap.py::test_tap_entry_points_match_their_float64_definition (lim_f, lim_g =
    1e-3, 4e-3 in fp16 and 4e-3, 3e-2 in bf16; LSE at 10 lim_f), p = 0.3, the segment's keys hashed from key0 = 1234.
    `unsorted_wide`: every 32-key tile is emitted in several masked passes -- a key has one keep decision in all of them.
    `two_blocks_per_wave`, `four_blocks_per_wave`: the NB = 2 and NB = 4 instantiations (S = 120, S = 232)."""
    import tap_drop_check
    r = tap_drop_check.check_case(name, key0=1234, p=0.3, **KERNEL_CASES[name])
    f16 = KERNEL_CASES[name].get("prec") == _lib.PREC_F16
    lim_f, lim_g = (1e-3, 4e-3) if f16 else (4e-3, 3e-2)
    assert r["flagged"] == 0 and r["dead"] == 0.0
    assert 0.6 < r["kept"] < 0.8, r
    assert r["Rk"] < lim_f and r["LSE"] < 10 * lim_f, r
    for k in ("dG", "dGb", "dtable", "da", "db", "dys", "dxs"):
        assert r[k] < lim_g, (k, r)


def _oracle_chain_drop(query, feat, Wkv, bkv, pos, table, h, V, keep):
    """tests/test_gpu_tap.py:_oracle_chain (sample -> proj_k | proj_v -> materialised attention, per view) with the
    dropout multiplier keep (P h, M, N) on the softmax weights."""
    B, C, S, _ = query.shape
    c = C // h
    P, N, _ = pos.shape
    grid = pos[:, None, :, (1, 0)]
    xs = F.grid_sample(feat.permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    kv = F.linear(xs[:, :, 0].permute(0, 2, 1), Wkv, bkv)
    outs = []
    for p in range(P):
        q = query[p // V].reshape(h, c, S * S)
        kk = kv[p, :, :C].reshape(N, h, c).permute(1, 2, 0)
        vv = kv[p, :, C:].reshape(N, h, c).permute(1, 2, 0)
        o = O.attention_core(q, kk, vv, pos[p:p + 1], table, S, S, 1, c ** -0.5, keep=keep[p * h:(p + 1) * h])
        outs.append(o.reshape(C, S * S).t())
    return torch.stack(outs, 0)


def _run_host_path(cfg, prec, p, seed, cot_scale, problem_seed):
    B, V, C, h, S, D, Hi, Wi, n_pin = cfg
    ins = _tap_problem(B, V, C, h, S, D, Hi, Wi, n_pin, seed=problem_seed)
    split = ins[-1]
    N = ins[4].shape[1]
    keep = drop_mult(seed, p, B * V * h, S, N)              # over ALL N keys: both segments share it
    cpu = [t.clone().double().requires_grad_(True) for t in ins[:-1]]
    want = _oracle_chain_drop(*cpu, h, V, keep)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * cot_scale
    want.backward(cot)
    gpu = [t.clone().to(DEV).requires_grad_(True) for t in ins[:-1]]
    query, feat, Wkv, bkv, pos, table = gpu
    ops.KERNEL_TIMER.start()
    got = ops.attention_core(query, None, None, pos, table, heads=h, groups=1, views=V, precision=prec,
                             kv_source=(feat, Wkv, bkv), cell_split=split, tap_source=True, attn_drop=(p, seed))
    got.backward(cot.float().to(DEV))
    used = set(ops.KERNEL_TIMER.stop())
    for k in TAP_DROP + REGION_DROP:
        assert k in used, sorted(used)
    assert not {n for n in used if n.startswith(("bevr_attn_cell", "bevr_attn_gather", "bevr_attn_slab"))}, sorted(used)
    assert "bevr_attn_tap_fwd" not in used, sorted(used)
    with torch.no_grad():
        plain = ops.attention_core(query, None, None, pos, table, heads=h, groups=1, views=V, precision=prec,
                                   kv_source=(feat, Wkv, bkv), cell_split=split, tap_source=True)
    assert rel_err(plain.double().cpu(), want.detach()) > 0.05, "the mask changed nothing"
    return got, want, gpu, cpu


@pytest.mark.parametrize("cfg", TAP_CFGS)
def test_attention_core_tap_dropout_matches_the_oracle_with_the_same_mask(cfg):
    """bf16, p = 0.3, at the limits tests/test_gpu_tap.py::test_attention_core_with_tap_source_matches_the_oracle applies
    to the same route without dropout: rtol 3e-2 / atol 1.5e-2 on the output, 3e-2 on every gradient."""
    got, want, gpu, cpu = _run_host_path(cfg, _lib.PREC_BF16, 0.3, 0x5eed1234, 1.0, sum(cfg))
    for n, a, b in zip(["query", "feat", "Wkv", "bkv", "pos", "table"], gpu, cpu):
        print(f"[tap dropout bf16 {cfg}] grad {n}: {rel_err(a.grad.double().cpu(), b.grad):.3e}")
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().float().numpy(), rtol=3e-2, atol=1.5e-2)
    for n, a, b in zip(["query", "feat", "Wkv", "bkv", "pos", "table"], gpu, cpu):
        e = rel_err(a.grad.double().cpu(), b.grad)
        assert e < 3e-2, f"grad {n}: rel err {e:.3e}"


@pytest.mark.parametrize("cfg", TAP_CFGS[:3])
def test_attention_core_tap_dropout_in_fp16_matches_the_oracle_with_the_same_mask(cfg):
    """fp16 operands, a mean-type loss (cotangents ~1e-5), at the limits of
    tests/test_gpu_tap.py::test_attention_core_with_tap_source_in_fp16_matches_the_oracle: 2.5e-3 and 5e-3."""
    got, want, gpu, cpu = _run_host_path(cfg, _lib.PREC_F16, 0.3, 0x5eed4321, 1e-5, sum(cfg) + 1)
    e = rel_err(got.detach().double().cpu(), want.detach())
    print(f"[tap dropout fp16 {cfg}] out: {e:.3e}")
    for n, a, b in zip(["query", "feat", "Wkv", "bkv", "pos", "table"], gpu, cpu):
        print(f"[tap dropout fp16 {cfg}] grad {n}: {rel_err(a.grad.double().cpu(), b.grad):.3e}")
    assert e < 2.5e-3, f"out: rel err {e:.3e}"
    for n, a, b in zip(["query", "feat", "Wkv", "bkv", "pos", "table"], gpu, cpu):
        e = rel_err(a.grad.double().cpu(), b.grad)
        assert e < 5e-3, f"grad {n}: rel err {e:.3e}"


@pytest.mark.parametrize("p", [0.3, max(STRESS_P)])
def test_tap_and_region_routes_evaluate_one_mask(p):
    """The call of tests/test_gpu_tap.py::test_tap_and_cell_kernels_agree_on_the_same_keys with dropout: the pinned keys
    on the tap dropout kernels (tap_source=True) and every key on the region dropout kernels (no tap_source: the route
    before the tap kernels had a mask).  Same seed, so the same mask; both in bf16 operands; that test's 3e-2."""
    B, V, C, h, S, D, Hi, Wi, n_pin = 1, 2, 64, 2, 34, 3, 12, 30, 1024
    ins = _tap_problem(B, V, C, h, S, D, Hi, Wi, n_pin, seed=9)
    split = ins[-1]
    res, names = [], []
    for tap in (True, False):
        gpu = [t.clone().to(DEV).requires_grad_(True) for t in ins[:-1]]
        query, feat, Wkv, bkv, pos, table = gpu
        ops.KERNEL_TIMER.start()
        out = ops.attention_core(query, None, None, pos, table, heads=h, groups=1, views=V, precision=_lib.PREC_BF16,
                                 kv_source=(feat, Wkv, bkv), cell_split=split, tap_source=tap, attn_drop=(p, 0xabc + int(p * 100)))
        out.square().mean().backward()
        names.append(set(ops.KERNEL_TIMER.stop()))
        res.append([out.detach()] + [t.grad for t in gpu])
    assert set(TAP_DROP) <= names[0] and not {n for n in names[1] if n.startswith("bevr_attn_tap")}, names
    assert set(REGION_DROP) <= names[0] and set(REGION_DROP) <= names[1], names
    errs = {n: rel_err(a, b) for n, a, b in zip(["out", "query", "feat", "Wkv", "bkv", "pos", "table"], *res)}
    print(f"[two routes p={p}] " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for n, e in errs.items():
        assert e < 3e-2, f"{n}: {e:.3e}"


def test_sca_module_with_dropout_keeps_the_pinned_keys_on_the_tap_kernels(monkeypatch):
    """SCADeformableAttention in training mode, attn_drop_rate > 0, bf16, split_is_pinned=True at a geometry where
    _pinned_keys_tap holds (S = 32, D = 3, Hi = 8, Wi = 20: 2.5 * 7 / 15 < 3, 2.5 * 19 / 95 < 2) with 1136 keys per view
    pinned exactly at (-1, -1).  The (p, seed) draw and the module's per-call cell_order permutation are captured, the
    kernels' mask is put into the oracle's key order, and the output and d(rpe_table) are held to O.sca_forward(keep=...)
    at the bf16 limits of tests/test_gpu_dropout.py::test_modules_with_dropout_match_the_oracle_with_the_exact_mask (3e-2,
    GRAD_LIM).  In eval() the module launches what a module without dropout launches."""
    from bevrender_amd.model import SCA_deform_attn as SCAmod
    torch.manual_seed(11)
    B, C, h, S, D, Hi, Wi, V = 2, 64, 2, 32, 3, 8, 20, 2
    prec = _lib.PREC_BF16
    Hk, Wk = S // 2, S * D
    N = Hk * Wk
    cs = 400                                    # keys [400, N): 1136 pinned keys per view
    sca = SCAmod.SCADeformableAttention(S, D, C, h, 1, 1, 3, True, B, n_views=V, attn_drop_rate=0.4, precision=prec)
    with torch.no_grad():
        for t in sca.parameters():
            t.copy_(torch.randn_like(t) * (0.1 if t.ndim > 1 else 0.05))
    assert sca._pinned_keys_tap(S, Hi, Wi)
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
    q = torch.randn(B, C, S, S)
    x = torch.randn(B, V, C, Hi, Wi)
    ref = (torch.rand(1, V, N, 2) * 2.2 - 1.1)
    ref[:, :, cs:] = -1.0
    ref = ref.reshape(1, V, Hk, Wk, 2).expand(B, -1, -1, -1, -1).contiguous()
    p_s = {k: t.detach().double().clone().requires_grad_(k == "rpe_table") for k, t in sca.state_dict().items()}
    sca = sca.to(DEV).train()
    ops.KERNEL_TIMER.start()
    got, _ = sca(x.to(DEV), q.to(DEV), ref.to(DEV), {}, False, cell_split=cs, split_is_pinned=True)
    cot = torch.randn(got.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    (got * cot.float().to(DEV)).sum().backward()
    used = set(ops.KERNEL_TIMER.stop())
    for k in TAP_DROP + REGION_DROP:
        assert k in used, sorted(used)
    assert not set(TAP_PLAIN) & used, sorted(used)
    assert len(draws) == 1 and draws[0] is not None and len(orders) == 1
    (pd, sd), (dyn, n_tail) = draws[0], orders[0]
    assert n_tail > 0                           # the keys of the sparsest cells joined the region segment
    # kernel key nk < cs is the oracle's key nk; nk >= cs is the oracle's key cs + dyn[view problem][nk - cs]
    m_k = drop_mult(sd, pd, B * V * h, S, N)
    keep = torch.empty_like(m_k)
    for pv in range(B * V):
        perm = torch.cat((torch.arange(cs), cs + dyn[pv]))
        keep[pv * h:(pv + 1) * h][:, :, perm] = m_k[pv * h:(pv + 1) * h]
    want = O.sca_forward(p_s, x.double(), q.double(), ref.double(), n_heads=h, depth_dim=D, keep=keep)
    (want * cot).sum().backward()
    with torch.no_grad():
        plain = O.sca_forward(p_s, x.double(), q.double(), ref.double(), n_heads=h, depth_dim=D)
    e = rel_err(got.detach().cpu().double(), want.detach())
    eg = rel_err(sca.rpe_table.grad.cpu().double(), p_s["rpe_table"].grad)
    print(f"[sca tap dropout] out {e:.3e}  grad rpe_table {eg:.3e}")
    assert e < 3e-2, f"out {e:.3e}"
    # the comparison can tell a wrong mask: without the mask the oracle is farther away than the limit held above
    assert rel_err(got.detach().cpu().double(), plain) > 3e-2, "the mask changed nothing"
    assert eg < GRAD_LIM[prec], f"grad rpe_table {eg:.3e}"

    # eval(): dropout is the identity -- the launches of a module that has no dropout at all
    def launches(mod):
        ops.KERNEL_TIMER.start()
        o, _ = mod(x.to(DEV), q.to(DEV), ref.to(DEV), {}, False, cell_split=cs, split_is_pinned=True)
        o.square().mean().backward()
        return set(ops.KERNEL_TIMER.stop())
    nodrop = SCAmod.SCADeformableAttention(S, D, C, h, 1, 1, 3, True, B, n_views=V, precision=prec).to(DEV)
    nodrop.load_state_dict(sca.state_dict())
    ev = launches(sca.eval())
    assert not {n for n in ev if "dropout" in n}, sorted(ev)
    assert set(TAP_PLAIN) <= ev, sorted(ev)
    assert ev == launches(nodrop.train()), sorted(ev)
