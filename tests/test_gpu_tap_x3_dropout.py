"""Attention dropout on the tap kernels in the split-bf16 mode (BEVR_PREC_BF16X3, csrc/attn_tap_*_x3_drop.hip, behind
BEVR_TAP_X3=1 and BEVR_TAP_X3_DROP=1) at the project's f32 limits.

The levels of tests/test_gpu_tap_dropout.py, in the split mode and at the limits of tests/test_gpu_tap_x3.py: the three
entry points against the float64 restatement of their definition with the host twin of the keep mask
(tools/tap_drop_check.py, operands built from the header's words); the EXACT recompute of flagged columns under the mask;
ops.attention_core(tap_pix=..., attn_drop=...) -- region dropout kernels on the projected rows of the scattered keys, the
new kernels on the pinned ones, ONE mask over all keys -- against the oracle's materialised attention with that mask,
forward and every gradient; the same mask on the all-region route; and the SCA module in training mode, which must take
the route and neither sample nor project the pinned keys."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from bevrender_amd import _lib, ops
from oracle import bevrender_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from test_gpu_dropout import STRESS_P, drop_mult  # noqa: E402
from test_gpu_tap import TAP_CFGS, _tap_problem  # noqa: E402
from test_gpu_tap_dropout import REGION_DROP, TAP_DROP, TAP_PLAIN, _oracle_chain_drop  # noqa: E402
from test_gpu_tap_x3 import LIM, check_keys, pos_kink_distance, rel_err  # noqa: E402
from test_tap_x3_dropout_capi import NB2_CASE, NEW, TWO_ROUTES_CFG  # noqa: E402
from test_tap_x3_host import X3_KERNEL_CASES, kink_shares  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
X3 = _lib.PREC_BF16X3
CASES = dict(X3_KERNEL_CASES, nb2=NB2_CASE)
OTHER = ("bevr_attn_cell", "bevr_attn_gather", "bevr_attn_slab")


@pytest.fixture(autouse=True)
def switches_on(monkeypatch):
    monkeypatch.setenv("BEVR_TAP_X3", "1")
    monkeypatch.setenv("BEVR_TAP_X3_DROP", "1")


@pytest.mark.parametrize("name", list(CASES))
def test_tap_x3_dropout_entry_points_match_their_float64_definition(name):
    """p = 0.3, the segment's keys hashed from key0 = 1234, LIM of tests/test_gpu_tap_x3.py; the kept mass (slot 15 of R
    over lsum) at the Rn limit.  `unsorted_wide`: every tile is emitted in several masked passes -- one keep decision per
    key in all of them; `nb2`, `nb4`: the NB = 2 (3 waves per SIMD) and NB = 4 instantiations (S = 120, S = 232)."""
    import tap_drop_check
    kw = CASES[name]
    r = tap_drop_check.check_case(name + " x3 drop", key0=1234, p=0.3, prec=X3, host_rng=True, **kw)
    print({k: v for k, v in r.items() if k != "keys"})
    assert r["flagged"] == 0 and r["dead"] == 0.0
    assert 0.6 < r["kept"] < 0.8, r["kept"]
    assert r["Rk"] < LIM["Rn"] and r["mass"] < LIM["Rn"] and r["LSE"] < LIM["LSE"], (r["Rk"], r["mass"], r["LSE"])
    for k in ("dG", "dGb", "dtable"):
        assert r[k] < LIM[k], (k, r[k])
    ks = r["keys"]
    geom = ks["geom"]
    dist = kink_shares(ks["a"], ks["b"], ks["ys"], ks["xs"], geom.S, geom.Wt, kw.get("h_cols"))[2]
    for k in ("da", "db", "dys", "dxs"):
        check_keys(f"{name} drop {k}", ks[k][0], ks[k][1], dist, LIM["dpos"])


def test_tap_x3_dropout_forward_recomputes_flagged_columns_under_the_mask():
    """The set-up of test_tap_forward_in_the_split_mode_recomputes_flagged_columns (logit scale 200) with the mask: the
    columns are flagged on the UNMASKED mass (lsum) and recomputed by the EXACT instantiation, which rescales lsum with the
    running maximum.  Compared with the restatement on the same split operands: Rn, the kept mass and LSE at their limits."""
    import tap_drop_check
    r = tap_drop_check.check_case("big logits x3 drop", key0=1234, p=0.3, P=1, h=2, S=16, N=300, Wt=2 * 16 * 3 - 1,
                                  gscale=200.0, seed=4, prec=X3, host_rng=True)
    print({k: v for k, v in r.items() if k != "keys"})
    assert r["flagged"] > 0
    assert 0.6 < r["kept"] < 0.8
    assert r["mimic"][0] < LIM["Rn"] and r["mimic"][2] < LIM["Rn"] and r["mimic"][1] < LIM["LSE"], r["mimic"]


def run_route(ins, split, h, V, drop, tap=True):
    """The SCA module's branches on (query, feat, Wkv, bkv, pos, table) leaves.  tap: only the scattered keys are sampled
    and projected, the pinned ones are attention_core's tap segment (the promise without the check, as the module gives
    it); else every key is sampled and projected and there is no split: the all-region route."""
    query, feat, Wkv, bkv, pos, table = ins
    xf = feat.permute(0, 3, 1, 2)
    if tap:
        kv = F.linear(ops.sample_features(xf, pos[:, :split].contiguous(), 1), Wkv, bkv)
        return ops.attention_core(query, None, None, pos, table, heads=h, groups=1, views=V, precision=X3, kv=kv,
                                  cell_split=split, tap_source="pinned", tap_pix=(feat, Wkv, bkv), attn_drop=drop)
    kv = F.linear(ops.sample_features(xf, pos, 1), Wkv, bkv)
    return ops.attention_core(query, None, None, pos, table, heads=h, groups=1, views=V, precision=X3, kv=kv, attn_drop=drop)


NAMES = ["query", "feat", "Wkv", "bkv", "pos", "table"]


@pytest.mark.parametrize("cfg", TAP_CFGS)
def test_attention_core_tap_pix_with_dropout_matches_the_oracle_with_the_same_mask(cfg):
    """The limits of tests/test_gpu_tap_x3.py::test_attention_core_with_tap_pix_matches_the_oracle (out 2e-4, gradients
    5e-4, table 2.5e-4, d(pos) 1e-3 by the kink rule) with p = 0.3 and one mask over all N keys."""
    B, V, C, h, S, D, Hi, Wi, n_pin = cfg
    p, seed = 0.3, 0x5eed1234
    ins = _tap_problem(B, V, C, h, S, D, Hi, Wi, n_pin, seed=sum(cfg))
    split = ins[-1]
    N = ins[4].shape[1]
    keep = drop_mult(seed, p, B * V * h, S, N)
    cpu = [t.clone().double().requires_grad_(True) for t in ins[:-1]]
    want = _oracle_chain_drop(*cpu, h, V, keep)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    want.backward(cot)
    gpu = [t.clone().to(DEV).requires_grad_(True) for t in ins[:-1]]
    ops.KERNEL_TIMER.start()
    got = run_route(gpu, split, h, V, (p, seed))
    got.backward(cot.float().to(DEV))
    used = set(ops.KERNEL_TIMER.stop())
    for k in NEW + REGION_DROP:
        assert k in used, sorted(used)
    assert not (set(TAP_PLAIN) | set(TAP_DROP)) & used, sorted(used)
    assert not {n for n in used if n.startswith(OTHER)}, sorted(used)
    e = rel_err(got.detach().cpu(), want.detach())
    errs = {n: rel_err(a.grad.cpu(), b.grad) for n, a, b in zip(NAMES, gpu, cpu) if n != "pos"}
    print(f"\n[tap_pix dropout {cfg}] out {e:.3e}  gradients " + " ".join(f"{n} {v:.3e}" for n, v in errs.items()))
    with torch.no_grad():
        plain = run_route(gpu, split, h, V, None)
    assert rel_err(plain.cpu(), want.detach()) > 0.05, "the mask changed nothing"
    assert e < 2e-4, f"out: {e:.3e}"
    for n, v in errs.items():
        assert v < (2.5e-4 if n == "table" else 5e-4), f"grad {n}: {v:.3e}"
    dist = pos_kink_distance(ins[4], S, 2 * S * D - 1, Hi, Wi)
    check_keys(f"tap_pix dropout {cfg} d(pos)", gpu[4].grad, cpu[4].grad, dist, 1e-3)


@pytest.mark.parametrize("p", [0.3, max(STRESS_P)])
def test_tap_pix_and_region_routes_evaluate_one_mask(p):
    """test_tap_and_cell_kernels_agree_in_the_split_mode's geometry with dropout: the pinned keys on the new kernels
    against every key's projected rows on the region dropout kernels, the same seed and so the same mask.  Both routes are
    held to the float64 limits, so they may differ by at most twice each limit of the test above."""
    B, V, C, h, S, D, Hi, Wi, n_pin = TWO_ROUTES_CFG
    ins = _tap_problem(B, V, C, h, S, D, Hi, Wi, n_pin, seed=9)
    split = ins[-1]
    res, names = [], []
    for tap in (True, False):
        gpu = [t.clone().to(DEV).requires_grad_(True) for t in ins[:-1]]
        ops.KERNEL_TIMER.start()
        out = run_route(gpu, split, h, V, (p, 0xabc + int(p * 100)), tap)
        out.square().mean().backward()
        names.append(set(ops.KERNEL_TIMER.stop()))
        res.append([out.detach()] + [t.grad for t in gpu])
    assert set(NEW) <= names[0] and not {n for n in names[1] if n.startswith("bevr_attn_tap")}, names
    assert set(REGION_DROP) <= names[0] and set(REGION_DROP) <= names[1], names
    errs = {n: rel_err(a, b) for n, a, b in zip(["out"] + NAMES, *res)}
    print(f"\n[two routes x3 p={p}] " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert errs["out"] < 4e-4, errs["out"]
    for n in ("query", "feat", "Wkv", "bkv"):
        assert errs[n] < 1e-3, (n, errs[n])
    assert errs["table"] < 5e-4, errs["table"]
    dist = pos_kink_distance(ins[4], S, 2 * S * D - 1, Hi, Wi)
    check_keys(f"two routes x3 p={p} d(pos)", res[0][5], res[1][5], dist, 2e-3)


def _sampled_keys(rec, nb, Hi, Wi, C):
    """keys per problem of the ONE bevr_sample_fwd launch in a kernel-timer record, out of its byte count
    (ops.sample_features: 4 nb (Hi Wi C + N C + 2 N))"""
    assert rec["n"] == 1, rec
    return round((rec["bytes"] / (4.0 * nb) - Hi * Wi * C) / (C + 2))


def test_sca_module_in_training_takes_the_split_mode_tap_dropout_route(monkeypatch):
    """SpatialCrossAttn (its SCADeformableAttention) with precision bf16x3 in training mode, attn_drop_rate = 0.3, at the
    size of tests/test_gpu_tap_x3.py::test_sca_module_takes_the_tap_route_in_the_split_mode (S = 72, 24 x 64 features, six
    views, 256 sampled BEV rows) and its module limits (out 3e-4, gradients 3e-3, offset heads 1.5e-2:
    tests/test_gpu_fullsize.py).  The (p, seed) draw and the per-call cell_order permutation are captured, the kernels'
    mask is put into the oracle's key order (static k-d order, then the per-call order of the pinned keys) and the module is
    held to O.sca_forward(keep=...).  The launches: the three new entry points beside the region dropout kernels, and the
    ONE sampling launch covers the region segment's keys alone -- the pinned keys are neither sampled nor projected.
    With BEVR_TAP_X3_DROP unset the same module launches the all-region dropout set and samples every key."""
    from bevrender_amd.model import SCA_deform_attn as SCAmod
    from bevrender_amd.model.SCA import SpatialCrossAttn
    from bevrender_amd.model.bev_cmr_proj import BEV2CameraProjector
    from test_gpu_fullsize import _check_module_grads, _randomize, pick_rows, ring_rig
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
        return out.detach(), ran
    out, ran = step()
    _, order, cs = sca.reference_points(0, qg.device)
    assert 0 < cs < 10000 and len(draws) == 1 and draws[0] is not None and len(orders) == 1
    for k in NEW + REGION_DROP:
        assert k in ran and ran[k]["n"] >= 1, sorted(ran)
    assert not (set(TAP_PLAIN) | set(TAP_DROP)) & set(ran), sorted(ran)
    assert not {n for n in ran if n.startswith(OTHER)}, sorted(ran)
    (pd, sd), (dyn, n_tail) = draws[0], orders[0]
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
    e = rel_err(out.reshape(B, C, S * S)[:, :, rows.to(DEV)].cpu(), want.detach())
    print(f"\n[sca module x3 tap dropout S={S}] out rel err {e:.3e}")
    got = {n: prm.grad for n, prm in att.named_parameters()}
    got.update({"in.query": qg.grad, "in.x": xg.grad})
    wnt = {n: pw[n].grad for n in used}
    wnt.update({"in.query": qc.grad, "in.x": xc.grad})
    assert e < 3e-4, f"out: {e:.3e}"
    _check_module_grads(f"sca module x3 tap dropout S={S}", got, wnt, 0)
    # the switch unset: every key sampled, projected and sent through the region dropout kernels
    monkeypatch.delenv("BEVR_TAP_X3_DROP")
    _, ran0 = step()
    assert set(REGION_DROP) <= set(ran0), sorted(ran0)
    assert not {n for n in ran0 if n.startswith(("bevr_attn_tap",) + OTHER)}, sorted(ran0)
    assert _sampled_keys(ran0["bevr_sample_fwd"], B * V, Hi, Wi, C) == N, ran0["bevr_sample_fwd"]
