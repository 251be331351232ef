"""Tap kernels in the split-bf16 mode (BEVR_PREC_BF16X3, csrc/attn_tap_*_x3.hip): the projector-pinned keys attended
without K and V at the project's f32 limits (tests/test_gpu_fullsize.py: LIMITS[PREC_BF16X3]).

The levels of tests/test_gpu_tap.py, in the split mode: the entry points against the float64 restatement of their
definition (tools/tap_check.py, operands built from the header's words); ops.attention_core(tap_pix=...) -- region kernels
on the projected rows of the scattered keys, tap kernels on the pinned ones, merged through (O, LSE) -- against the
oracle's materialised attention, forward and every gradient; the tap route against the cell kernels on the same keys; one
view at the benchmark's size on sampled BEV rows; and the SCA module, which must take the route.

d(pos) is judged with check_dpos's rule (tests/test_gpu_fullsize.py), restated in check_keys below: every key away from
a kink meets the limit; keys over it are at most 2 % and all within 2e-3 of a kink (an integer crossing of a_n, of
j rx + b_n for a compared column, or of the sampling position ys / xs)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from bevrender_amd import _lib, ops
from oracle import bevrender_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from test_gpu_tap import TAP_CFGS, _oracle_chain, _tap_problem  # noqa: E402
from test_tap_x3_host import KINK, X3_KERNEL_CASES, kink_shares  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
X3 = _lib.PREC_BF16X3
# LIMITS[PREC_BF16X3] mapped onto the entry points' outputs
LIM = dict(Rn=2e-4, LSE=2e-3, dG=5e-4, dGb=5e-4, dtable=2.5e-4, dpos=1e-3)


def rel_err(got, want):
    return (got.double() - want.double()).abs().max().item() / (want.abs().max().item() + 1e-30)


def check_keys(tag, got, want, dist, lim):
    """check_dpos's rule on per-key gradients: got, want (..., N[, 2]); dist (..., N) the key's distance to its nearest
    kink.  Prints the figures before it asserts."""
    got, want, dist = got.double().cpu(), want.double().cpu(), dist.cpu()
    err = (got - want).abs()
    if err.dim() > dist.dim():
        err = err.amax(-1)
    tol = lim * want.abs().max().item()
    bad = err > tol
    clean = dist >= KINK
    n_bad, n = int(bad.sum()), bad.numel()
    worst_clean = err[clean].max().item() / want.abs().max().item() if clean.any() else 0.0
    print(f"[{tag}] {n_bad} of {n} keys over {lim:.0e} x max (all within {dist[bad].max().item() if n_bad else 0:.1e} of a "
          f"kink); away from kinks ({int(clean.sum())} keys): worst {worst_clean:.3e}")
    assert clean.double().mean().item() >= 0.3, f"{tag}: only {int(clean.sum())} of {n} keys away from kinks: vacuous"
    assert n_bad <= 0.02 * n, f"{tag}: {n_bad} of {n} keys differ"
    assert n_bad == 0 or dist[bad].max().item() < KINK, f"{tag}: a key away from any kink differs"


def pos_kink_distance(pos, S, Wt, Hi, Wi, cols=None):
    """(P, N, 2) key positions (y, x) -> distance of every key to its nearest kink (table coordinates and sampling
    position), float64."""
    p = pos.detach().double().cpu()
    a = (1 - p[..., 0]) * (S - 1) / 2
    b = (1 - p[..., 1]) * (Wt - 1) / 4
    ys, xs = (p[..., 0] + 1) * 0.5 * (Hi - 1), (p[..., 1] + 1) * 0.5 * (Wi - 1)
    return kink_shares(a, b, ys, xs, S, Wt, cols)[2]


@pytest.mark.parametrize("name", list(X3_KERNEL_CASES))
def test_tap_entry_points_in_the_split_mode_match_their_float64_definition(name):
    import tap_check
    kw = X3_KERNEL_CASES[name]
    r = tap_check.check_case(name + " x3", prec=X3, host_rng=True, **kw)
    print({k: v for k, v in r.items() if k != "keys"})
    assert r["flagged"] == 0 and r["dead"] == 0.0
    assert r["exact"][0] < LIM["Rn"] and r["exact"][1] < LIM["LSE"], r["exact"]
    for k in ("dG", "dGb", "dtable"):
        assert r[k] < LIM[k], (k, r[k])
    ks = r["keys"]
    geom = ks["geom"]
    dist = kink_shares(ks["a"], ks["b"], ks["ys"], ks["xs"], geom.S, geom.Wt, kw.get("h_cols"))[2]
    for k in ("da", "db", "dys", "dxs"):
        check_keys(f"{name} {k}", ks[k][0], ks[k][1], dist, LIM["dpos"])


def test_tap_forward_in_the_split_mode_recomputes_flagged_columns():
    """logit scale 200 (test_tap_forward_recomputes_rows_whose_weights_underflow_the_static_reference): every weight
    underflows against the static reference, the columns are flagged and recomputed with an online maximum.  Compared with
    the restatement on the SAME split operands (G, tap weights and table as hi + lo pairs)."""
    import tap_check
    r = tap_check.check_case("big logits x3", P=1, h=2, S=16, N=300, Wt=2 * 16 * 3 - 1, gscale=200.0, seed=4, prec=X3,
                             host_rng=True)
    print({k: v for k, v in r.items() if k != "keys"})
    assert r["flagged"] > 0
    assert r["mimic"][0] < LIM["Rn"] and r["mimic"][1] < LIM["LSE"], r["mimic"]


def run_route(ins, split, h, V, Hi, Wi):
    """The SCA module's unfused branch on (query, feat, Wkv, bkv, pos, table) leaves: with the tap kernels available in
    the split mode only the scattered keys are sampled and projected and the pinned ones go to attention_core as the tap
    segment; otherwise (BEVR_TAP_X3=0: the earlier routing) every key is sampled and projected and [split, N) is the
    cell segment."""
    query, feat, Wkv, bkv, pos, table = ins
    xf = feat.permute(0, 3, 1, 2)
    if ops.tap_supported(X3, 1):
        kv = F.linear(ops.sample_features(xf, pos[:, :split].contiguous(), 1), Wkv, bkv)
        return ops.attention_core(query, None, None, pos, table, heads=h, groups=1, views=V, precision=X3, kv=kv,
                                  cell_split=split, tap_source=True, tap_pix=(feat, Wkv, bkv))
    kv = F.linear(ops.sample_features(xf, pos, 1), Wkv, bkv)
    return ops.attention_core(query, None, None, pos, table, heads=h, groups=1, views=V, precision=X3, kv=kv,
                              cell_split=split)


@pytest.mark.parametrize("cfg", TAP_CFGS)
def test_attention_core_with_tap_pix_matches_the_oracle(cfg, monkeypatch):
    monkeypatch.setenv("BEVR_TAP_X3", "1")
    B, V, C, h, S, D, Hi, Wi, n_pin = cfg
    ins = _tap_problem(B, V, C, h, S, D, Hi, Wi, n_pin, seed=sum(cfg))
    split = ins[-1]
    cpu = [t.clone().double().requires_grad_(True) for t in ins[:-1]]
    want = _oracle_chain(*cpu, h, V)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    want.backward(cot)
    gpu = [t.clone().to(DEV).requires_grad_(True) for t in ins[:-1]]
    ops.KERNEL_TIMER.start()
    got = run_route(gpu, split, h, V, Hi, Wi)
    got.backward(cot.float().to(DEV))
    ran = ops.KERNEL_TIMER.stop()
    assert all(k in ran for k in ("bevr_attn_tap_fwd", "bevr_attn_tap_bwd_q", "bevr_attn_tap_bwd_k")), sorted(ran)
    assert not any(k.startswith("bevr_attn_cell") for k in ran), sorted(ran)
    e = rel_err(got.detach().cpu(), want.detach())
    print(f"\n[tap_pix {cfg}] out rel err {e:.3e}")
    errs = {n: rel_err(a.grad.cpu(), b.grad) for n, a, b in zip(["query", "feat", "Wkv", "bkv", "table"],
                                                               gpu[:4] + gpu[5:], cpu[:4] + cpu[5:])}
    print(f"[tap_pix {cfg}] gradients " + " ".join(f"{n} {v:.3e}" for n, v in errs.items()))
    assert e < 2e-4, f"out: {e:.3e}"
    for n, v in errs.items():
        assert v < (2.5e-4 if n == "table" else 5e-4), f"grad {n}: {v:.3e}"
    dist = pos_kink_distance(ins[4], S, 2 * S * D - 1, Hi, Wi)
    check_keys(f"tap_pix {cfg} d(pos)", gpu[4].grad, cpu[4].grad, dist, 1e-3)


def test_tap_and_cell_kernels_agree_in_the_split_mode(monkeypatch):
    """test_tap_and_cell_kernels_agree_on_the_same_keys' geometry with BEVR_TAP_X3 toggled: two routes to one softmax, both
    held to the float64 limits elsewhere, so they may differ by at most twice each limit."""
    B, V, C, h, S, D, Hi, Wi, n_pin = 1, 2, 64, 2, 34, 3, 12, 30, 1024
    ins = _tap_problem(B, V, C, h, S, D, Hi, Wi, n_pin, seed=9)
    split = ins[-1]
    res = []
    for sw in ("1", "0"):
        monkeypatch.setenv("BEVR_TAP_X3", sw)
        gpu = [t.clone().to(DEV).requires_grad_(True) for t in ins[:-1]]
        ops.KERNEL_TIMER.start()
        out = run_route(gpu, split, h, V, Hi, Wi)
        out.square().mean().backward()
        ran = ops.KERNEL_TIMER.stop()
        assert ("bevr_attn_tap_fwd" in ran) == (sw == "1") and ("bevr_attn_cell_fwd" in ran) == (sw == "0"), sorted(ran)
        res.append([out.detach()] + [t.grad for t in gpu])
    names = ["out", "query", "feat", "Wkv", "bkv", "pos", "table"]
    errs = {n: rel_err(a, b) for n, a, b in zip(names, *res)}
    print("\n[tap vs cell x3] " + " ".join(f"{n} {v:.3e}" for n, v in errs.items()))
    assert errs["out"] < 4e-4
    for n in ("query", "feat", "Wkv", "bkv"):
        assert errs[n] < 1e-3, (n, errs[n])
    assert errs["table"] < 5e-4
    dist = pos_kink_distance(ins[4], S, 2 * S * D - 1, Hi, Wi)
    check_keys("tap vs cell x3 d(pos)", res[0][5], res[1][5], dist, 2e-3)


def test_one_view_at_the_benchmark_size_on_sampled_rows(monkeypatch):
    """One view of config 2's SCA attention (S = 200, D = 5, 100 000 keys, about two thirds pinned, offsets over the
    learned range, 64 x 176 feature map) through the new route, against the float64 oracle chain on 128 sampled BEV rows
    with a cotangent that is zero elsewhere (the method of tests/test_gpu_fullsize.py).  All of LIMITS[PREC_BF16X3]."""
    from test_gpu_fullsize import LIMITS, cell_split_perm, lift_problem, permute_keys, pick_rows
    monkeypatch.setenv("BEVR_TAP_X3", "1")
    S, D, C, h, Hi, Wi = 200, 5, 64, 2, 64, 176
    Wt = 2 * S * D - 1
    p = lift_problem(S, D, 6, C, h, 704, 256, {"X": 50, "Y": 50, "Z": 2}, seed=2024)
    perm, split = cell_split_perm(p, S)
    pos = permute_keys(p["pos"], perm)[:1].contiguous()                      # view 0: scattered keys, then the pinned ones
    N = pos.shape[1]
    assert 0.5 < (N - split) / N < 0.8
    gen = torch.Generator().manual_seed(77)
    feat = torch.randn(1, Hi, Wi, C, generator=gen)
    Wkv = torch.randn(2 * C, C, generator=gen) * C ** -0.5
    bkv = torch.randn(2 * C, generator=gen) * 0.3
    query, table = p["query"], p["table"]
    rows = pick_rows(S, 128, 1)
    cot = torch.randn(1, len(rows), C, generator=torch.Generator().manual_seed(5))
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    # float64 oracle: sample -> proj_k | proj_v -> materialised attention on the sampled rows
    cpu = [t.clone().double().requires_grad_(True) for t in (query, feat, Wkv, bkv, pos, table)]
    qc, fc, wc, bc, pc, tc = cpu
    xs = F.grid_sample(fc.permute(0, 3, 1, 2), pc[:, None, :, (1, 0)], mode="bilinear", padding_mode="zeros", align_corners=True)
    kv = F.linear(xs[:, :, 0].permute(0, 2, 1), wc, bc)
    c = C // h
    o = O.attention_core(qc[0].reshape(h, c, S * S), kv[0, :, :C].reshape(N, h, c).permute(1, 2, 0),
                         kv[0, :, C:].reshape(N, h, c).permute(1, 2, 0), pc, tc, S, S, 1, c ** -0.5, rows=rows)
    want = o.reshape(C, len(rows)).t()[None]
    (want * cot.double()).sum().backward()
    gpu = [t.clone().to(DEV).requires_grad_(True) for t in (query, feat, Wkv, bkv, pos, table)]
    ops.KERNEL_TIMER.start()
    out = run_route(gpu, split, h, 1, Hi, Wi)
    cot_full = torch.zeros_like(out)
    cot_full[:, rows.to(DEV)] = cot.to(DEV)
    out.backward(cot_full)
    ran = ops.KERNEL_TIMER.stop()
    assert "bevr_attn_tap_fwd" in ran and "bevr_attn_tap_bwd_k" in ran, sorted(ran)
    lim = LIMITS[X3]
    e = rel_err(out.detach()[:, rows.to(DEV)].cpu(), want.detach())
    print(f"\n[one view S=200 x3 tap] out rel err {e:.3e} (tap segment: {N - split} of {N} keys)")
    errs = {n: rel_err(a.grad.cpu(), b.grad) for n, a, b in zip(["query", "feat", "Wkv", "bkv", "table"],
                                                               gpu[:4] + gpu[5:], cpu[:4] + cpu[5:])}
    print("[one view S=200 x3 tap] gradients " + " ".join(f"{n} {v:.3e}" for n, v in errs.items()))
    assert e < lim["out"], f"out: {e:.3e}"
    # query: its own limit; feat, Wkv, bkv carry d(k), d(v): the k / v limits (the same figure); table: its own
    for n, v in errs.items():
        assert v < (lim["table"] if n == "table" else lim["query"] if n == "query" else lim["k"]), f"grad {n}: {v:.3e}"
    dist = pos_kink_distance(pos, S, Wt, Hi, Wi, cols=(rows % S).tolist())
    check_keys("one view S=200 x3 tap d(pos)", gpu[4].grad, cpu[4].grad, dist, lim["pos"])


def test_sca_module_takes_the_tap_route_in_the_split_mode(monkeypatch):
    """SpatialCrossAttn with precision bf16x3 at a small size (S = 72, 24 x 64 features, six views): the projector's pinned
    keys are split off (split_is_pinned) and must run on the tap kernels -- asserted through the kernel timer's record of
    the launches, not through the result -- and the module matches oracle.sca_forward at the module limits of
    tests/test_gpu_fullsize.py (out 3e-4, gradients 3e-3, offset heads 1.5e-2: _sca_module_rows).
    The size is chosen by the reference's own error: d(query) contains the offset heads' path, a sum of d(pos) over the
    keys, and d(pos) jumps at kinks, so ANY float32 evaluation of a small geometry can land on the other side of a kink
    for a key that carries a visible share of that sum.  The oracle evaluated in float32 against itself in float64 (CPU)
    gives for d(query) / the worst offset-head tensor: S = 40 (16 x 44 features), 64 rows 4.6e-3 / 4.4e-3, 1 200 rows
    1.4e-2 / 1.0e-2 -- over the 3e-3 limit before any kernel runs (on an MI355X this route gave 3.7e-3 and 4.8e-3 there);
    S = 56: 1.3e-3 / 4.2e-3; S = 100: 2.3e-3 / 1.9e-3; S = 72 (24 x 64 features), 256 rows: 5.0e-4 / 2.2e-3, six times
    under the limits: the size used here."""
    from test_gpu_fullsize import _sca_module_rows
    monkeypatch.setenv("BEVR_TAP_X3", "1")
    ops.KERNEL_TIMER.start()
    try:
        _sca_module_rows(X3, S=72, img_w=256, img_h=96, n_rows=256, max_split=10000)
    finally:
        ran = ops.KERNEL_TIMER.stop()
    for k in ("bevr_attn_tap_fwd", "bevr_attn_tap_bwd_q", "bevr_attn_tap_bwd_k"):
        assert k in ran and ran[k]["n"] >= 1, sorted(ran)
    assert not any(k.startswith("bevr_attn_cell") for k in ran), sorted(ran)
