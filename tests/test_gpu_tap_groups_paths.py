"""ops.attention_core(groups=2, tap_source=True) (behind BEVR_TAP_GROUPS) on the routes and under the gradient patterns
tests/test_gpu_tap_groups.py does not take: every key pinned (no region segment, no merge, dLSE None), concat_views,
B > 1 with V > 1, an image inside the tap grid, three heads per group, a bf16 feature map, a loose static bound (the
forward's exact pass, and in fp16 rows whose weights are all subnormal); gradient subsets, forwards without a backward,
replayed backwards, strided cotangents, and a cotangent on one of _TapAttnG2's two outputs alone.
The reference is the oracle chain of tests/test_gpu_tap_groups.py in float64; the limits are that file's."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from dataclasses import replace as dc_replace

from bevrender_amd import _lib, ops
from oracle import bevrender_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from test_gpu_tap_groups import G2, _core_case, _oracle_chain, _problem, rel_err  # noqa: E402
from tap_route_check import LOOSE, fp16_gap_case  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = _lib.PREC_BF16, _lib.PREC_F16
NAMES = ["query", "feat", "Wkv", "bkv", "pos", "table"]
G1 = {"bevr_attn_tap_fwd", "bevr_attn_tap_bwd_q", "bevr_attn_tap_bwd_k"}
GRAD_LIM = {BF16: 3e-2, F16: 5e-3}
COT = {BF16: 1.0, F16: 1e-5}                 # fp16: a mean-type loss (test_gpu_tap_groups.py)


def _assert_out(got, want, prec, tag=""):
    got, want = got.detach().double().cpu(), want.detach()
    e = rel_err(got, want)
    print(f"{tag} out: rel err {e:.3e}")
    if prec == F16:
        assert e < 2.5e-3, f"{tag} out: rel err {e:.3e}"
    else:
        np.testing.assert_allclose(got.float().numpy(), want.float().numpy(), rtol=3e-2, atol=1.5e-2)


def _assert_grads(gpu, cpu, prec, tag="", names=NAMES):
    for n in names:
        a, b = gpu[NAMES.index(n)], cpu[NAMES.index(n)]
        e = rel_err(a.grad.double().cpu(), b.grad)
        print(f"{tag} grad {n}: {e:.3e}")
        assert e < GRAD_LIM[prec], f"{tag} grad {n}: rel err {e:.3e}"


def _concat(want, B, V):
    """(B V, M, C) -> (B, M, V C): the views side by side in the channel axis"""
    P, M, C = want.shape
    return want.reshape(B, V, M, C).permute(0, 2, 1, 3).reshape(B, M, V * C)


def _run(cfg, prec, seed, cot_scale, concat_views=False, feat_bf16=False, change=None, grad_names=NAMES, cot=None,
         backward=True, no_grad=False):
    """_core_case of tests/test_gpu_tap_groups.py with the call's other arguments open: returns (got, want, gpu, cpu, used).
    change(ins): edits the drawn inputs in place.  feat_bf16: the feature map is a bf16 tensor on the GPU and the oracle
    gets the rounded values.  grad_names: the GPU inputs with requires_grad.  no_grad: the GPU call under torch.no_grad()."""
    B, V, C, h, S, D, Hi, Wi, n_pin = cfg
    ins = list(_problem(B, V, C, h, S, D, Hi, Wi, n_pin, seed))
    split = ins[-1]
    if change is not None:
        change(ins)
    if feat_bf16:
        ins[1] = ins[1].to(torch.bfloat16)
    cpu = [t.clone().double().requires_grad_(True) for t in ins[:-1]]
    want = _oracle_chain(*cpu, h, V)
    if concat_views:
        want = _concat(want, B, V)
    if cot is None:
        cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * cot_scale
    want.backward(cot)
    gpu = [t.clone().to(DEV).requires_grad_(n in grad_names) for n, t in zip(NAMES, ins[:-1])]
    query, feat, Wkv, bkv, pos, table = gpu
    assert ops.tap_supported(prec, 2)
    ops.KERNEL_TIMER.start()
    try:
        with torch.set_grad_enabled(not no_grad):
            got = ops.attention_core(query, None, None, pos, table, heads=h, groups=2, views=V, precision=prec,
                                     kv_source=(feat, Wkv, bkv), cell_split=split, tap_source=True, concat_views=concat_views)
        if backward:
            got.backward(cot.float().to(DEV))
        torch.cuda.synchronize()
    finally:
        used = set(ops.KERNEL_TIMER.stop())
    # (bkv alone reaches the output through Gb and bv, beside _TapAttnG2: its backward has nothing to do)
    tap_bwd = backward and bool(set(grad_names) - {"bkv"})
    for k in G2:
        assert (k in used) == (tap_bwd or k == G2[0]), f"{k} ({sorted(used)})"
    assert not G1 & used
    return got, want, gpu, cpu, used


# ---- B. routes ------------------------------------------------------------------------------------------------------
BV = (2, 3, 32, 2, 12, 3, 6, 20, 128)        # B and V both above 1: (B, V, 24) reshapes differ from their transpose


@pytest.mark.parametrize("concat_views", [False, True])
def test_batch_and_views_both_above_one(concat_views, monkeypatch):
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    got, want, gpu, cpu, _ = _run(BV, BF16, sum(BV), 1.0, concat_views=concat_views)
    assert tuple(got.shape) == ((2, 144, 96) if concat_views else (6, 144, 32))
    _assert_out(got, want, BF16, f"B2 V3 concat {concat_views}")
    _assert_grads(gpu, cpu, BF16, f"B2 V3 concat {concat_views}")


@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "fp16"])
def test_every_key_pinned(prec, monkeypatch):
    """cell_split = 0: no region segment, O_r is None, no merge, and _TapAttnG2.backward gets dLSE = None"""
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    cfg = (1, 2, 64, 2, 12, 3, 6, 20, 6 * 36)
    seen = []
    real = ops._TapAttnG2.backward

    def spy(ctx, dRn, dLSE):
        seen.append((dRn is None, dLSE is None))
        return real(ctx, dRn, dLSE)
    monkeypatch.setattr(ops._TapAttnG2, "backward", staticmethod(spy))
    got, want, gpu, cpu, used = _run(cfg, prec, sum(cfg), COT[prec])
    assert seen == [(False, True)], seen
    region = [k for k in used if k.startswith("bevr_attn") and not k.startswith("bevr_attn_tap_g2")]
    assert not region and "bevr_kv_project" not in used, sorted(used)
    _assert_out(got, want, prec, f"all pinned prec {prec}")
    _assert_grads(gpu, cpu, prec, f"all pinned prec {prec}")


def test_image_inside_the_tap_grid(monkeypatch):
    """a 3 x 2 image: the 4 x 3 tap grid's missing pixel rows are zero padding"""
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    cfg = (1, 2, 16, 2, 10, 3, 3, 2, 64)
    got, want, gpu, cpu = _core_case(cfg, BF16, sum(cfg), 1.0)
    _assert_out(got, want, BF16, "3x2 image")
    _assert_grads(gpu, cpu, BF16, "3x2 image")


def test_three_heads_per_group(monkeypatch):
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    cfg = (1, 1, 96, 6, 12, 2, 6, 14, 64)
    got, want, gpu, cpu = _core_case(cfg, BF16, sum(cfg), 1.0)
    _assert_out(got, want, BF16, "h = 6")
    _assert_grads(gpu, cpu, BF16, "h = 6")


def test_bf16_feature_map(monkeypatch):
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    got, want, gpu, cpu, _ = _run(BV, BF16, sum(BV) + 2, 1.0, feat_bf16=True)
    assert gpu[1].dtype == torch.bfloat16 and gpu[1].grad.dtype == torch.bfloat16
    _assert_out(got, want, BF16, "bf16 feat")
    _assert_grads(gpu, cpu, BF16, "bf16 feat")


# ---- the loose static bound ------------------------------------------------------------------------------------------
def _inflate(factor):
    def change(ins):
        ins[1][:, 3, 2, :] *= factor
    return change


def test_loose_logit_bound_takes_the_exact_pass(monkeypatch):
    """test_tap_path_with_a_loose_logit_bound_takes_the_exact_pass (tests/test_gpu_tap.py) with two groups -- and with the
    forward's flags in hand: the namespace of the K.TAP_G2_FWD launch is kept, and columns were flagged."""
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    kept = []
    real = ops._run

    def spy(name, o):
        if name == ops.K.TAP_G2_FWD:
            kept.append(o)
        return real(name, o)
    monkeypatch.setattr(ops, "_run", spy)
    B, V, C, h, S, D, Hi, Wi, n_pin = LOOSE
    ins = list(_problem(B, V, C, h, S, D, Hi, Wi, n_pin, 21))
    _inflate(300.0)(ins)
    cpu = [t.clone().double().requires_grad_(True) for t in ins[:-1]]
    want = _oracle_chain(*cpu, h, V)
    want.square().mean().backward()
    gpu = [t.clone().to(DEV).requires_grad_(True) for t in ins[:-1]]
    query, feat, Wkv, bkv, pos, table = gpu
    ops.KERNEL_TIMER.start()
    try:
        got = ops.attention_core(query, None, None, pos, table, heads=h, groups=2, views=V, precision=BF16,
                                 kv_source=(feat, Wkv, bkv), cell_split=ins[-1], tap_source=True)
        got.square().mean().backward()
        torch.cuda.synchronize()
    finally:
        used = set(ops.KERNEL_TIMER.stop())
    assert set(G2) <= used and not G1 & used, sorted(used)
    assert len(kept) == 1
    n_flag = int(kept[0].flags.sum())
    print(f"loose bound bf16: flagged columns {n_flag} of {kept[0].flags.numel()}")
    assert n_flag > 0
    assert torch.isfinite(got).all()
    _assert_out(got, want, BF16, "loose bound bf16")
    _assert_grads(gpu, cpu, BF16, "loose bound bf16", names=["query", "pos", "table"])


def test_loose_logit_bound_in_fp16_leaves_only_subnormal_weights(monkeypatch):
    """tools/tap_route_check.py, fp16_gap_case: at least half the rows with their bound 22 .. 33 binades loose"""
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    fp16_gap_case(2, _problem, _oracle_chain)


# ---- C. gradient patterns of _TapAttnG2 ------------------------------------------------------------------------------
_full = {}


def _full_run(prec):
    """the all-inputs run of configuration BV: computed once per precision, read-only afterwards"""
    if prec not in _full:
        got, want, gpu, cpu, _ = _run(BV, prec, 77, COT[prec])
        _full[prec] = (got.detach().clone(), want.detach(), [t.grad.detach().clone() for t in gpu], cpu)
    return _full[prec]


def _close(a, b, tag):
    """the same gradient from two runs: the order of float atomics is the only difference (the reduction test's bound)"""
    d, big = (a.double() - b.double()).abs().max().item(), b.double().abs().max().item()
    assert big > 0 and d <= 1e-5 * big, f"{tag}: differs by {d:.3e} of {big:.3e}"


PATTERNS = [("query",), ("feat",), ("Wkv",), ("bkv",), ("pos",), ("table",), ("query", "table"), ("feat", "Wkv", "bkv")]


@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("names", PATTERNS, ids=["+".join(p) for p in PATTERNS])
def test_gradient_subsets(names, prec, monkeypatch):
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    out_all, _, grads_all, cpu = _full_run(prec)
    got, want, gpu, _, _ = _run(BV, prec, 77, COT[prec], grad_names=names)
    assert torch.equal(got.detach(), out_all)
    for n, t in zip(NAMES, gpu):
        if n in names:
            _close(t.grad, grads_all[NAMES.index(n)], f"{n} alone vs all inputs")
        else:
            assert t.grad is None, n
    _assert_grads(gpu, cpu, prec, f"subset {names} prec {prec}", names=list(names))


@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "fp16"])
def test_forward_without_a_backward(prec, monkeypatch):
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    out_all, _, grads_all, _ = _full_run(prec)
    got, *_ = _run(BV, prec, 77, COT[prec], backward=False, no_grad=True)
    assert not got.requires_grad and torch.equal(got, out_all)
    got, *_ = _run(BV, prec, 77, COT[prec], grad_names=(), backward=False)
    assert not got.requires_grad and torch.equal(got, out_all)
    # a graded forward that is never backpropagated, then a fresh forward and backward
    got, *_ = _run(BV, prec, 77, COT[prec], backward=False)
    assert got.requires_grad and torch.equal(got.detach(), out_all)
    del got
    got, _, gpu, _, _ = _run(BV, prec, 77, COT[prec])
    assert torch.equal(got.detach(), out_all)
    for n, t in zip(NAMES, gpu):
        _close(t.grad, grads_all[NAMES.index(n)], f"{n} after an abandoned forward")


@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "fp16"])
def test_replayed_backward_and_strided_cotangents(prec, monkeypatch):
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    B, V, C, h, S, D, Hi, Wi, n_pin = BV
    ins = _problem(B, V, C, h, S, D, Hi, Wi, n_pin, 77)

    def forward():
        gpu = [t.clone().to(DEV).requires_grad_(True) for t in ins[:-1]]
        query, feat, Wkv, bkv, pos, table = gpu
        out = ops.attention_core(query, None, None, pos, table, heads=h, groups=2, views=V, precision=prec,
                                 kv_source=(feat, Wkv, bkv), cell_split=ins[-1], tap_source=True)
        return out, gpu
    out_all, _, grads_all, _ = _full_run(prec)
    cot = (torch.randn(out_all.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * COT[prec]).float().to(DEV)
    # backward twice over one graph: the gradients accumulate
    out, gpu = forward()
    out.backward(cot, retain_graph=True)
    first = [t.grad.clone() for t in gpu]
    out.backward(cot)
    for n, t, f, g in zip(NAMES, gpu, first, grads_all):
        _close(f, g, f"{n}, first backward")
        _close(t.grad, 2.0 * f, f"{n}, second backward")
    # the cotangent as a transposed view
    out, gpu = forward()
    cot_t = cot.transpose(1, 2).contiguous().transpose(1, 2)
    assert not cot_t.is_contiguous() and torch.equal(cot_t, cot)
    out.backward(cot_t)
    for n, t, g in zip(NAMES, gpu, grads_all):
        _close(t.grad, g, f"{n}, transposed cotangent")
    # the cotangent as a stride-0 expand (what .sum().backward() hands over) against the same values, contiguous
    k = COT[prec]
    out, gpu = forward()
    (out.sum() * k).backward()
    out2, gpu2 = forward()
    out2.backward(torch.full_like(out2, k))
    for n, t, t2 in zip(NAMES, gpu, gpu2):
        _close(t.grad, t2.grad, f"{n}, expanded cotangent")


def _segment(gpu, prec):
    """attention_core's tap segment of configuration BV as attention_core forms its operands: (O_c, LSE_c) of
    ops._tap_groups_segment in the oracle's layout, O (B', h, M, c), LSE (B', h, M)."""
    B, V, C, h, S, D, Hi, Wi, n_pin = BV
    query, feat, Wkv, bkv, pos, table = gpu
    N = pos.shape[1]
    n = N - n_pin
    Wt = table.shape[-1]
    route = ops.attention_route(prec, 2, S, Wt, N, n, True, False, "kv_source", C, h)
    seg = route.segments[-1]
    assert seg.fwd == ops.K.TAP_G2_FWD
    geom = ops.AttnGeom(n_prob=B * V, q_div=V, heads=h, groups=2, S=S, N=n, Wt=Wt, precision=prec)
    Qp = ops.pack_query(query.float(), h)
    a, b = ops.key_coords(pos.float(), S, Wt, N)
    Tt = ops.pack_table(table.float(), geom)
    O_c, LSE_c = ops._tap_groups_segment(Qp, feat, Wkv, bkv, pos[:, n:], a[:, n:], b[:, n:], Tt, dc_replace(geom, N=N - n),
                                         seg, B, V)
    c = C // h
    Oo = O_c.reshape(B * V, h, S, geom.Sp, -1)[:, :, :, :S, :c].transpose(2, 3).reshape(B * V, h, S * S, c)
    Lo = LSE_c.reshape(B * V, h, S, geom.Sp)[..., :S].transpose(2, 3).reshape(B * V, h, S * S)
    return Oo, Lo


def _segment_lse_float64(query, feat, Wkv, bkv, pos, table, h, V):
    """log2 sum_n 2^(log2(e) (c^-0.5 q . K_n + bias)) over the keys `pos`, K_n = Wk (the groups' samples) + bk: (B', h, M)"""
    B, C, S, _ = query.shape
    c, M, g = C // h, S * S, 2
    P, Hi, Wi, _ = feat.shape
    N = pos.shape[1]
    hg = h // g
    xs = F.grid_sample(feat.permute(0, 3, 1, 2).reshape(P * g, C // g, Hi, Wi), pos[:, None, :, (1, 0)], mode="bilinear",
                       padding_mode="zeros", align_corners=True).reshape(P, C, N)
    kk = F.linear(xs.permute(0, 2, 1), Wkv[:C], bkv[:C]).reshape(P, N, h, c)
    q_grid = O.normalized_grid(S, S, torch.float64).reshape(1, M, 2)
    out = []
    for p in range(P):
        q = query[p // V].reshape(h, c, M)
        rows = []
        for gi in range(g):
            hs = slice(gi * hg, (gi + 1) * hg)
            disp = (q_grid.unsqueeze(2) - pos[p * g + gi].reshape(1, 1, N, 2)) * 0.5
            bias = F.grid_sample(table[hs][None], disp[..., (1, 0)], mode="bilinear", align_corners=True)[0]
            rows.append(torch.logsumexp(torch.einsum("hcm,nhc->hmn", q[hs], kk[p][:, hs]) * c ** -0.5 + bias, 2) * ops.LOG2E)
        out.append(torch.cat(rows, 0))
    return torch.stack(out, 0)


@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("which", ["lse", "out"])
def test_cotangent_on_one_output_of_the_segment_alone(which, prec, monkeypatch):
    """_TapAttnG2.backward with dRn None (a loss on LSE_c alone) and with dLSE None (a loss on O_c alone): the Function sets
    set_materialize_grads(False) and handles the None itself.  attention_core's merge always sends both, so
    ops._tap_groups_segment is called as attention_core calls it."""
    monkeypatch.setenv("BEVR_TAP_GROUPS", "1")
    B, V, C, h, S, D, Hi, Wi, n_pin = BV
    ins = _problem(B, V, C, h, S, D, Hi, Wi, n_pin, 78)
    n = ins[-1]
    seen = []
    real = ops._TapAttnG2.backward

    def spy(ctx, dRn, dLSE):
        seen.append((dRn is None, dLSE is None))
        return real(ctx, dRn, dLSE)
    monkeypatch.setattr(ops._TapAttnG2, "backward", staticmethod(spy))
    cpu = [t.clone().double().requires_grad_(True) for t in ins[:-1]]
    pos_tap = cpu[4][:, n:]
    if which == "lse":
        want = _segment_lse_float64(cpu[0], cpu[1], cpu[2], cpu[3], pos_tap, cpu[5], h, V)
        names = NAMES            # bkv: its K half
    else:
        want = _oracle_chain(cpu[0], cpu[1], cpu[2], cpu[3], pos_tap, cpu[5], h, V)          # the softmax over the tap keys alone
        want = want.reshape(B * V, S * S, h, C // h).permute(0, 2, 1, 3)
        names = NAMES
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(11), dtype=torch.float64) * COT[prec]
    want.backward(cot)
    gpu = [t.clone().to(DEV).requires_grad_(True) for t in ins[:-1]]
    ops.KERNEL_TIMER.start()
    try:
        Oo, Lo = _segment(gpu, prec)
        got = Lo if which == "lse" else Oo
        got.backward(cot.float().to(DEV))
        torch.cuda.synchronize()
    finally:
        used = set(ops.KERNEL_TIMER.stop())
    assert set(G2) <= used and not G1 & used, sorted(used)
    assert seen == [(which == "lse", which == "out")], seen
    if which == "lse":
        e = (got.detach().double().cpu() - want.detach()).abs().max().item()
        lim = 10 * (1e-3 if prec == F16 else 4e-3)
        print(f"LSE alone prec {prec}: LSE err {e:.3e} (limit {lim:.0e})")
        assert e < lim
    else:
        _assert_out(got, want, prec, f"O alone prec {prec}")
    assert not gpu[4].grad[:, :n].ne(0).any(), "a key outside the segment got a gradient"
    _assert_grads(gpu, cpu, prec, f"{which} alone prec {prec}", names=names)
