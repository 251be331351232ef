"""The slab query-side backward in the split-bf16 mode (csrc/attn_slab_bwd_q_x3.hip, bevr_attn_slab_bwd_q_x3,
BEVR_SLAB_X3=1) against the float64 oracle (oracle/bevrender_oracle.py: attention_core, the reference's
model/SCA_deform_attn.py:331-413 differentiated by autograd) at the project's f32 limits (tests/test_gpu_fullsize.py:
LIMITS[PREC_BF16X3], query 5e-4, table 2.5e-4, max |err| / max |want| per tensor), and against the parent's route for
that mode, the query-tile kernel bevr_attn_bwd_q (switch off), on the same inputs.

The switch is set through monkeypatch, and WHICH entry point ran is read off a recorder around ops._launch: a case in
which bevr_attn_slab_bwd_q_x3 did not run exactly once on the new route, or ran at all on the parent's, fails.  The
parent's route is asserted first, with a message of its own: if it misses a limit the inputs are at fault.  Every case
prints both routes' errors before it asserts (-s).  Shapes: tests/test_gpu_slab.py's CASES (S = 12 ... 70, ragged sizes,
three row blocks, channel groups, keys far outside the table -- the clamped body --, a single key, a table two orders of
magnitude wider than a slab), an operand-split case (large Q . K), a bias-path case (large table) and the SCA module."""
import functools

import pytest
import torch

from bevrender_amd import _lib, ops
from oracle import bevrender_oracle as O
from test_gpu_fullsize import LIMITS, rel_err
from test_gpu_slab import CASES, _problem

pytestmark = pytest.mark.gpu
DEV = "cuda"
X3 = _lib.PREC_BF16X3
LIM = LIMITS[X3]          # query 5e-4, table 2.5e-4
NAME = "bevr_attn_slab_bwd_q_x3"
TILE = "bevr_attn_bwd_q"


class Recorder:
    """Around ops._launch: the entry points in the order they ran."""

    def __init__(self):
        self.names, self.orig = [], ops._launch

    def __call__(self, entry, *a, **kw):
        self.names.append(entry)
        return self.orig(entry, *a, **kw)


def run(ins, h, g, V, monkeypatch, new):
    """ops.attention_core in split mode, forward and backward, on the new route (BEVR_SLAB_X3=1 and BEVR_SLAB=2: the slab
    kernel for every table width) or the parent's (the switch off).  Returns (out, dQ, dT, dKV, dPos)."""
    rec = Recorder()
    with monkeypatch.context() as m:
        for name in ("BEVR_SLAB", "BEVR_SLAB_ROWS", "BEVR_GATHER_X3", "BEVR_TAP_X3"):
            m.delenv(name, raising=False)
        m.setenv("BEVR_SLAB_X3", "1" if new else "0")
        if new:
            m.setenv("BEVR_SLAB", "2")
        m.setattr(ops, "_launch", rec)
        query, kv, pos, table = (t.clone().to(DEV).requires_grad_(True) for t in ins)
        out = ops.attention_core(query, None, None, pos, table, heads=h, groups=g, views=V, precision=X3, kv=kv)
        cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(77)).to(DEV)
        out.backward(cot)
        torch.cuda.synchronize()
    assert rec.names.count(NAME) == (1 if new else 0), rec.names
    assert rec.names.count(TILE) == (0 if new else 1), rec.names
    assert not any(n.startswith("bevr_attn_slab") and n not in (NAME, "bevr_attn_slab_x3_prep") for n in rec.names), rec.names
    return out.detach(), query.grad, table.grad, kv.grad, pos.grad


def oracle_grads(ins, B, V, C, h, g, S, N):
    """dQ and d(table) of the oracle's materialised attention in float64, as tests/test_gpu_slab.py builds it"""
    query, kv, pos, table = (t.clone().double().requires_grad_(True) for t in ins)
    c = C // h
    outs = []
    for p in range(B * V):
        q = query[p // V].reshape(h, c, S * S)
        kk = kv[p, :, :C].reshape(N, h, c).permute(1, 2, 0)
        vv = kv[p, :, C:].reshape(N, h, c).permute(1, 2, 0)
        o = O.attention_core(q, kk, vv, pos[p * g:(p + 1) * g], table, S, S, g, c ** -0.5)
        outs.append(o.reshape(C, S * S).t())
    want = torch.stack(outs, 0)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(77)).double()
    want.backward(cot)
    return query.grad, table.grad


@functools.lru_cache(maxsize=None)
def case(name, q_scale=1.0, k_scale=1.0, t_scale=1.0):
    """inputs and the oracle's gradients of a case, computed once and left unchanged"""
    B, V, C, h, g, S, N, Wt, extra = CASES[name]
    query, kv, pos, table = _problem(B, V, C, h, g, S, N, Wt, seed=3 + S, **extra)
    kv = torch.cat((kv[..., :C] * k_scale, kv[..., C:]), -1)
    ins = (query * q_scale, kv, pos, table * t_scale)
    return ins, oracle_grads(ins, B, V, C, h, g, S, N)


def max_logit(ins, B, V, C, h, N, S):
    """largest |Q . K| c^-0.5 log2 e over all pairs"""
    query, kv = ins[0], ins[1]
    c = C // h
    s = torch.einsum("bhcm,bnhc->bhmn", query.reshape(B, h, c, S * S).repeat_interleave(V, 0), kv[..., :C].reshape(B * V, N, h, c))
    return s.abs().max().item() * c ** -0.5 * ops.LOG2E


def both_routes(tag, name, ins, want, monkeypatch):
    B, V, C, h, g, S, N, Wt, extra = CASES[name]
    dq_w, dt_w = want
    o1, dq1, dt1, dkv1, dp1 = run(ins, h, g, V, monkeypatch, True)
    o0, dq0, dt0, dkv0, dp0 = run(ins, h, g, V, monkeypatch, False)
    if N == 1:
        # one key: P = 1 and dS = P (dP - delta) = 0 for every pair: the oracle's gradients are zero to the last bit of float64
        # and max |want| normalises nothing.  What the kernels compute is the DIFFERENCE of dP = dO . V and delta = dO . O,
        # each as large as ||dO|| ||V|| (the bound the backward's own fixed-point scale is made of), so the error is
        # normalised by the gradients' size before that cancellation: d(table) sums dS over <= 1 tap weight per cell and
        # row, dQ = dS K c^-0.5
        assert dq_w.abs().max().item() < 1e-12 and dt_w.abs().max().item() < 1e-12
        c = C // h
        cot = torch.randn(B * V, S * S, C, generator=torch.Generator().manual_seed(77)).double()
        dp = (cot.reshape(B * V, S * S, h, c).norm(dim=-1).amax(1)
              * ins[1][..., C:].double().reshape(B * V, N, h, c).norm(dim=-1).amax(1)).max().item()
        scale = dict(query=dp * ins[1][..., :C].abs().max().item() * c ** -0.5, table=dp)
        err = lambda got, w, k: got.cpu().double().abs().max().item() / scale[k]
        print(f"\n[slab x3 {tag}] the oracle's gradients are zero; max |dQ| slab_x3 {dq1.abs().max().item():.3e} query-tile "
              f"{dq0.abs().max().item():.3e}, max |d(table)| {dt1.abs().max().item():.3e} {dt0.abs().max().item():.3e}; "
              f"normalised by {scale['query']:.3e} and {scale['table']:.3e}")
    else:
        err = lambda got, w, k: rel_err(got.cpu(), w)
    e1 = dict(query=err(dq1, dq_w, "query"), table=err(dt1, dt_w, "table"))
    e0 = dict(query=err(dq0, dq_w, "query"), table=err(dt0, dt_w, "table"))
    print(f"\n[slab x3 {tag}] slab_x3: dQ {e1['query']:.3e} d(table) {e1['table']:.3e} | query-tile: dQ {e0['query']:.3e} "
          f"d(table) {e0['table']:.3e} | limits {LIM['query']:.1e} {LIM['table']:.1e}")
    assert torch.equal(o1, o0), "the forward does not depend on the switch"
    # nor does the key side (float atomics in the position gradient: equal up to their order)
    assert rel_err(dkv1, dkv0) < 1e-5 and rel_err(dp1, dp0) < 1e-4
    for k in ("query", "table"):
        assert e0[k] < LIM[k], f"{tag}: the PARENT route misses the limit on these inputs: {k} {e0[k]:.3e}"
    assert torch.isfinite(dq1).all() and torch.isfinite(dt1).all()
    for k in ("query", "table"):
        assert e1[k] < LIM[k], f"{tag}: {k} {e1[k]:.3e}"
    assert dt1.abs().sum() > 0 or N == 1
    return e1, e0


@pytest.mark.parametrize("name", list(CASES))
def test_cases_against_the_oracle_and_the_query_tile_kernel(name, monkeypatch):
    ins, want = case(name)
    both_routes(name, name, ins, want, monkeypatch)


def test_operand_split_at_large_logits(monkeypatch):
    """The three_row_blocks shape with Q and K scaled by 3.6 each: |Q . K| c^-0.5 log2 e reaches ~100 log2 units (the region
    kernels pass up to 163).  A product of single bf16 images (2^-9 relative per operand) would be off by
    100 x 2^-8 ~ 0.4 log2 units per logit, a relative error of ~0.3 in P and in every gradient: three orders of magnitude
    over the limits; a missing lo term shows alike."""
    name = "three_row_blocks"
    B, V, C, h, g, S, N, Wt, extra = CASES[name]
    ins, want = case(name, q_scale=3.6, k_scale=3.6)
    big = max_logit(ins, B, V, C, h, N, S)
    print(f"\n[slab x3 operand split] max |Q.K| {big:.0f} log2 units")
    assert 80.0 < big < 163.0
    both_routes("operand split", name, ins, want, monkeypatch)


def test_bias_path_at_a_large_table(monkeypatch):
    """The table scaled by 30 (a standard deviation of 13 log2 units, +-50 at its tails, as tests/test_gpu_gather_x3.py's
    "table" case): a bias path rounded to 16 bits (2^-9 of ~50 units: 0.1 log2 units per logit) would miss the limits by two
    orders of magnitude; the f32 pair table, f32 tap weights and f32 interpolation are exact to 2^-24."""
    name = "three_row_blocks"
    ins, want = case(name, t_scale=30.0)
    print(f"\n[slab x3 bias path] max |bias| {ins[3].abs().max().item() * ops.LOG2E:.0f} log2 units")
    both_routes("bias path", name, ins, want, monkeypatch)


# ---- the module ----------------------------------------------------------------------------------------------------
from test_gpu_modules import SCA, _sca, check          # noqa: E402  (the small golden shapes of that file)


@pytest.mark.parametrize("name", SCA)
def test_sca_module(name, monkeypatch):
    """Split-mode SCADeformableAttention on the golden shapes of tests/test_gpu_modules.py with every split-mode switch on
    (BEVR_TAP_X3, BEVR_GATHER_X3, BEVR_SLAB_X3; BEVR_SLAB=2: these small tables are narrower than SCA's): output and every
    gradient at that file's f32 limits (check: the split mode is held to the f32 limits), through the new entry point."""
    rec = Recorder()
    with monkeypatch.context() as mp:
        for k, v in (("BEVR_TAP_X3", "1"), ("BEVR_GATHER_X3", "1"), ("BEVR_SLAB_X3", "1"), ("BEVR_SLAB", "2")):
            mp.setenv(k, v)
        mp.delenv("BEVR_SLAB_ROWS", raising=False)
        mp.setattr(ops, "_launch", rec)
        m, z, query, x, ref = _sca(name, X3)
        out, _ = m(x, query, ref, None, False)
        torch.cuda.synchronize()
        e = (out.detach().cpu().double() - torch.tensor(z["out"]).double()).abs().max().item()
        print(f"\n[slab x3 SCA {name}] max |out - golden| {e:.3e}")
        check(m, z, out, {"query": query, "x": x}, _lib.PREC_F32)
    assert NAME in rec.names and TILE not in rec.names, rec.names
