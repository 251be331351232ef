"""Tap kernels for two channel groups (csrc/attn_tap_*_g2.hip, behind BEVR_TAP_GROUPS): the entry points against the
float64 restatement of their definition (tools/tap_g2_check.py) and against the one-group entry points they reduce to;
ops.attention_core(kv_source, tap_source, groups=2) against the oracle's materialised attention on per-group samples
(reference model/SCA_deform_attn.py:290-413), forward and every gradient; and SCADeformableAttention(n_groups=2) on
the pinned route against the oracle's SCA forward, with the switch set and unset."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bevrender_amd import _lib, ops
from oracle import bevrender_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
DEV = "cuda"
G2 = ("bevr_attn_tap_g2_fwd", "bevr_attn_tap_g2_bwd_q", "bevr_attn_tap_g2_bwd_k")


def rel_err(got, want):
    return (got - want).abs().max().item() / (want.abs().max().item() + 1e-12)


# ---- 1. the entry points against their float64 definition -------------------------------------------------------
def _cases():
    import tap_g2_check
    return tap_g2_check.CASES


@pytest.mark.parametrize("name", ["sorted", "two_heads_per_group", "ragged", "unsorted_wide", "fp16", "two_blocks_per_wave",
                                  "four_blocks_per_wave"])
def test_entry_points_match_their_float64_definition(name):
    """The limits of tests/test_gpu_tap.py::test_tap_entry_points_match_their_float64_definition, unraised (the logit sums
    two rounded tap products instead of one; the measured figures are in profiles/tap_groups_errors.txt)."""
    import tap_g2_check
    kw = dict(_cases()[name])
    r = tap_g2_check.check_case(name, **kw)
    f16 = kw.get("prec") == _lib.PREC_F16
    lim_f, lim_g = (1e-3, 4e-3) if f16 else (4e-3, 3e-2)
    assert r["flagged"] == 0 and r["dead"] == 0.0
    assert r["exact"][0] < lim_f and r["exact"][1] < 10 * lim_f, r          # Rn, LSE (log2 units)
    assert r["mimic"][0] < 2e-3 and r["mimic"][1] < 1e-2, r                 # on the operands as the kernels round them
    for k in ("dG", "dGb", "dtable", "da", "db", "dys", "dxs"):
        assert r[k] < lim_g, (k, r)


# ---- 2. reduction to the one-group kernels -----------------------------------------------------------------------
def test_with_an_empty_second_block_the_kernels_are_the_one_group_kernels():
    """G / H block 1 zero: per (problem, group) the one-group entry points' results, up to the order of float atomics;
    then both groups at the same positions with the same G rows: group 1's weight sums are group 0's."""
    import tap_g2_check
    r = tap_g2_check.reduction_case()
    assert r["finite"]
    for k in ("R", "mref", "dG", "dtable", "dkey_a", "dkey_b", "dkey_y"):
        diff, big = r[k]
        assert big > 0 and diff <= 1e-5 * big, (k, r[k])
    diff, big = r["twin"]
    assert big > 0 and diff <= 1e-6 * big, r["twin"]


# ---- 3. attention_core against the oracle chain ------------------------------------------------------------------
def _problem(B, V, C, h, S, D, Hi, Wi, n_pin, seed):
    """An SCA-shaped call with two channel groups: per view N keys, the first N - n_pin scattered over the image, the
    last n_pin pinned to pixel (0, 0); every group has its own position of every key (offsets inside the learned range,
    tanh * 5 / (Hk - 1), 5 / (Wk - 1)).  pos (B V 2, N, 2), row p * 2 + g."""
    gen = torch.Generator().manual_seed(seed)
    Hk, Wk = S // 2, S * D
    N = Hk * Wk
    P = B * V
    query = torch.randn(B, C, S, S, generator=gen)
    feat = torch.randn(P, Hi, Wi, C, generator=gen)
    Wkv = torch.randn(2 * C, C, generator=gen) * C ** -0.5
    bkv = torch.randn(2 * C, generator=gen) * 0.3
    table = torch.randn(h, 2 * S - 1, 2 * S * D - 1, generator=gen) * 0.3
    scat = (torch.rand(P * 2, N - n_pin, 2, generator=gen) * 2 - 1) * 1.05
    off = torch.tanh(torch.randn(P * 2, n_pin, 2, generator=gen) * 1.5) * torch.tensor([5.0 / (Hk - 1), 5.0 / (Wk - 1)])
    pos = torch.cat((scat, off - 1.0), 1)
    return query, feat, Wkv, bkv, pos, table, N - n_pin


def _oracle_chain(query, feat, Wkv, bkv, pos, table, h, V):
    """per-group sample of the group's channels -> proj_k | proj_v -> materialised attention with n_groups = 2"""
    B, C, S, _ = query.shape
    c, g = C // h, 2
    P, Hi, Wi, _ = feat.shape
    N = pos.shape[1]
    grid = pos[:, None, :, (1, 0)]                                                  # (P g, 1, N, 2) in (x, y)
    xs = F.grid_sample(feat.permute(0, 3, 1, 2).reshape(P * g, C // g, Hi, Wi), grid, mode="bilinear",
                       padding_mode="zeros", align_corners=True).reshape(P, C, N)
    kv = F.linear(xs.permute(0, 2, 1), Wkv, bkv)                                     # (P, N, 2C)
    outs = []
    for p in range(P):
        q = query[p // V].reshape(h, c, S * S)
        kk = kv[p, :, :C].reshape(N, h, c).permute(1, 2, 0)
        vv = kv[p, :, C:].reshape(N, h, c).permute(1, 2, 0)
        o = O.attention_core(q, kk, vv, pos[p * g:(p + 1) * g], table, S, S, g, c ** -0.5)
        outs.append(o.reshape(C, S * S).t())
    return torch.stack(outs, 0)


CFGS = [
    # B, V, C, h, S, D, Hi, Wi, pinned keys per view (the shapes of tests/test_gpu_tap.py's twins, an even number of heads)
    (1, 2, 64, 2, 12, 3, 6, 20, 128),
    (2, 1, 32, 4, 16, 5, 6, 10, 448),
    (1, 1, 64, 2, 34, 2, 16, 44, 704),
]


def _core_case(cfg, prec, seed, cot_scale):
    B, V, C, h, S, D, Hi, Wi, n_pin = cfg
    ins = _problem(B, V, C, h, S, D, Hi, Wi, n_pin, seed)
    split = ins[-1]
    cpu = [t.clone().double().requires_grad_(True) for t in ins[:-1]]
    want = _oracle_chain(*cpu, h, V)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * cot_scale
    want.backward(cot)
    gpu = [t.clone().to(DEV).requires_grad_(True) for t in ins[:-1]]
    query, feat, Wkv, bkv, pos, table = gpu
    assert ops.tap_supported(prec, 2)
    ops.KERNEL_TIMER.start()
    got = ops.attention_core(query, None, None, pos, table, heads=h, groups=2, views=V, precision=prec,
                             kv_source=(feat, Wkv, bkv), cell_split=split, tap_source=True)
    got.backward(cot.float().to(DEV))
    torch.cuda.synchronize()
    used = set(ops.KERNEL_TIMER.stop())
    for k in G2:
        assert k in used, f"{k} did not run ({sorted(used)})"
    assert not {"bevr_attn_tap_fwd", "bevr_attn_tap_bwd_q", "bevr_attn_tap_bwd_k"} & used
    return got, want, gpu, cpu


@pytest.mark.parametrize("cfg", CFGS)
def test_attention_core_with_two_groups_matches_the_oracle(cfg, monkeypatch):
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    got, want, gpu, cpu = _core_case(cfg, _lib.PREC_BF16, sum(cfg), 1.0)
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().float().numpy(), rtol=3e-2, atol=1.5e-2)
    for n, a, b in zip(["query", "feat", "Wkv", "bkv", "pos", "table"], gpu, cpu):
        e = rel_err(a.grad.double().cpu(), b.grad)
        print(f"bf16 {cfg} grad {n}: {e:.3e}")
        assert e < 3e-2, f"grad {n}: rel err {e:.3e}"
    # both groups' positions carry a gradient of their own
    g = gpu[4].grad.reshape(-1, 2, *gpu[4].shape[1:])
    assert g[:, 0].abs().max() > 0 and g[:, 1].abs().max() > 0


@pytest.mark.parametrize("cfg", CFGS[:2])
def test_attention_core_with_two_groups_in_fp16_matches_the_oracle(cfg, monkeypatch):
    """a mean-type loss (cotangents ~1e-5: fp16 subnormals without _TapAttnG2's power-of-two scale)"""
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    got, want, gpu, cpu = _core_case(cfg, _lib.PREC_F16, sum(cfg) + 1, 1e-5)
    e = rel_err(got.detach().double().cpu(), want.detach())
    assert e < 2.5e-3, f"out: rel err {e:.3e}"
    for n, a, b in zip(["query", "feat", "Wkv", "bkv", "pos", "table"], gpu, cpu):
        e = rel_err(a.grad.double().cpu(), b.grad)
        print(f"fp16 {cfg} grad {n}: {e:.3e}")
        assert e < 5e-3, f"grad {n}: rel err {e:.3e}"


# ---- 4. the module -----------------------------------------------------------------------------------------------
def _module_case(seed):
    """test_sca_module_pinned_route_random's draw with n_groups = 2; seed 0: S = 32, D = 5 (more than 1 024 pinned keys
    per view)."""
    r = np.random.RandomState(2300 + seed)
    for _ in range(1000):
        h = int(r.choice([2, 4]))
        C = h * int(r.choice([8, 16, 32]))
        big = seed == 0
        S = 32 if big else int(r.choice([8, 12, 14, 16]))
        D = 5 if big else int(r.choice([1, 2, 3, 5]))
        V = int(r.choice([1, 1, 2, 3]))
        B = int(r.choice([1, 2]))
        Hk, Wk = S // 2, S * D
        frac = 2 / 3 if big else float(r.choice([1 / 3, 2 / 3]))
        hi_max = min(20, max(ops.TAP_R, int(np.ceil(1 + (ops.TAP_R - 1 - 1e-3) * (Hk - 1) / 2.5)) - 1))
        wi_max = min(24, max(ops.TAP_C, int(np.ceil(1 + (ops.TAP_C - 1 - 1e-3) * (Wk - 1) / 2.5)) - 1))
        Hi, Wi = int(r.randint(2, hi_max + 1)), int(r.randint(2, wi_max + 1))
        if C % 16 == 0 and (C // 2) % 4 == 0 and int(Hk * Wk * frac) >= 64:
            return h, C, S, D, V, B, Hi, Wi, frac
    raise AssertionError("no case drawn")


@pytest.mark.parametrize("prec", [_lib.PREC_BF16, _lib.PREC_F16])
@pytest.mark.parametrize("switch", ["on", "unset"])
@pytest.mark.parametrize("seed", list(range(6)))
def test_sca_module_with_two_groups_on_the_pinned_route(seed, switch, prec, monkeypatch):
    """SpatialCrossAttn's call (static key order and split of ops.split_key_order, the pinned keys at exactly (-1, -1),
    split_is_pinned=True) with n_groups = 2.  Switch on: the pinned keys on the two-group tap kernels, the scattered ones
    through bevr_kv_project.  Unset: today's behaviour -- no tap kernel, the same comparison."""
    from bevrender_amd.model.SCA_deform_attn import SCADeformableAttention
    from test_gpu_random_sweep_modules import compare, randomize_
    if switch == "on":
        monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    else:
        monkeypatch.delenv("BEVR_TAP_GROUPS", raising=False)
    h, C, S, D, V, B, Hi, Wi, frac = _module_case(seed)
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
    assert split < Hk * Wk
    if seed == 0:
        assert Hk * Wk - split > 1024
    m = SCADeformableAttention(bev_feat_shape=S, bev_depth_dim=D, dim_embed=C, n_heads=h, n_groups=2, stride=1,
                               kernel_size=3, scale_offset_range=True, batch_size=B, n_views=V, precision=prec).to(DEV)
    randomize_(m, 2500 + seed)
    assert m._pinned_keys_tap(S, Hi, Wi) == (switch == "on")
    p_cpu = {n: v.detach().cpu().double().requires_grad_(True) for n, v in m.state_dict().items()}
    qc, xc = query.double().requires_grad_(True), x.double().requires_grad_(True)
    want = O.sca_forward(p_cpu, xc, qc, ref.double(), n_heads=h, n_groups=2, depth_dim=D, scale_offset_range=True)
    qg, xg = query.clone().to(DEV).requires_grad_(True), x.clone().to(DEV).requires_grad_(True)
    ops.KERNEL_TIMER.start()
    out, _ = m(xg, qg, ref.to(DEV), None, False, key_order=order.to(DEV), cell_split=split, split_is_pinned=True)
    tag = f"sca g2 {switch} seed {seed} C{C} h{h} S{S} D{D} V{V} B{B} {Hi}x{Wi} split {split} prec{prec}"
    compare(m, out, want, (qg, xg), (qc, xc), p_cpu, tag, bf16=prec == _lib.PREC_BF16, f16=prec == _lib.PREC_F16)
    used = set(ops.KERNEL_TIMER.stop())
    assert "bevr_kv_project" in used, f"{tag}: {sorted(used)}"
    if switch == "on":
        for k in G2:
            assert k in used, f"{tag}: {k} did not run ({sorted(used)})"
    else:
        assert not [k for k in used if k.startswith("bevr_attn_tap")], f"{tag}: {sorted(used)}"
