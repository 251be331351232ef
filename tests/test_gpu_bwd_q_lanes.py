"""The per-key constants of the query-side backward kernels' key-row loops (csrc/attn_slab_bwd_q.hip, csrc/attn_bwd_q.hip)
come out of registers by DPP: lane l of a wave preloads the constants of key crow(l & 15, l >> 5) of a 32-key half and key
row t takes them from lane t of its own 16-lane row (csrc/attn_tile.h: bcast_key, row_bcast).  What can go wrong there is a
wrong preload lane, a wrong broadcast index, or a key count that leaves preload lanes past the list -- so:

  * every key count around a half (32 keys) and an emission / key step (64 keys): N = 1 .. 97 on a table no wider than one
    slab (every column's run is the whole key list), in bf16 and fp16;
  * the slab kernel's clamped body (keys whose table rows leave the window) in the first and in the second half of an
    emission -- far_halves() below replays the kernel's runs on the CPU and the test asserts that the inputs do that;
  * two row blocks, the second one ragged.

Both kernels run every case (BEVR_SLAB=2: the slab kernel; BEVR_SLAB=0: the query-tile kernel) against the float64 oracle,
compared as tests/test_gpu_slab.py compares them: the slab kernel within 1.5x + 1e-3 of the query-tile kernel's error, and
dQ and d(table) of both under the mode's gradient limits of tests/test_gpu_fullsize.py."""
import functools
import math

import pytest
import torch

from bevrender_amd import _lib, ops
from oracle import bevrender_oracle as O
from test_gpu_fullsize import LIMITS
from test_gpu_slab import CASES, _problem, _run

pytestmark = pytest.mark.gpu
PRECS = [_lib.PREC_BF16, _lib.PREC_F16]
TAG = {_lib.PREC_BF16: "bf16", _lib.PREC_F16: "f16"}

# csrc/attn_slab_bwd_q.hip
SLAB_W, SLAB_ROW0, SLAB_PADR, SLAB_EPS = 24, 10, 8, 0.02

#           B  V  C   h  g  S   Wt  extra
NARROW = (1, 1, 64, 2, 1, 12, 23, {})
FAR = CASES["far_keys"][:6] + (CASES["far_keys"][7], {"far": 0.5})      # far_keys' geometry; N and the far share are ours
FAR_NARROW = (1, 1, 64, 2, 1, 12, 23, {"far": 0.5})
TWO_BLOCKS = (1, 1, 64, 2, 1, 40, 2 * 40 * 3 - 1, {})
KEY_COUNTS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97]


def far_halves(pos, S, Wt):
    """The slab kernel's emissions replayed on the CPU (slab_ranges_kernel and the producer's constants): which 32-key
    halves (0, 1) of some emission hold a live key whose table rows leave the slab's window -- the halves that take the
    clamped body.  pos (P, N, 2)."""
    N = pos.shape[1]
    a, b = ops.key_coords(pos.float(), S, Wt, N)
    Sp, Ht = 32 * ((S + 31) // 32), 2 * S - 1
    a = a.clamp(-(Sp + 1.0), Ht + 1.0)
    b = b.clamp(-(Wt // 2 + 2.0), Wt + 1.0)
    rx = (Wt - 1) / (2.0 * (S - 1))
    xmin = -(Wt // 2 + 2) - 1
    xmax = int((S - 1) * rx) + Wt + 3
    halves = set()
    for p in range(pos.shape[0]):
        bs, order = b[p].sort()
        A = a[p][order].floor()
        far = (A + SLAB_ROW0 < 0) | (A > S - 1 + SLAB_PADR)
        for slab in range((xmax - xmin + SLAB_W) // SLAB_W):
            x0 = xmin + slab * SLAB_W
            for j in range(S):
                beg = int(torch.searchsorted(bs, torch.tensor(x0 - j * rx - SLAB_EPS)))
                end = int(torch.searchsorted(bs, torch.tensor(x0 + SLAB_W - j * rx + SLAB_EPS)))
                X = (j * rx + bs[beg:end]).floor()
                hit = torch.nonzero((X >= x0) & (X < x0 + SLAB_W) & far[beg:end]).flatten()
                halves.update(((hit % 64) // 32).tolist())
    return halves


@functools.lru_cache(maxsize=None)
def problem_and_oracle(geom, N, seed):
    """inputs (CPU, float32), the float64 oracle's dQ and d(table) and the size of the TERMS of either gradient: once per
    case, shared by the precisions.  dS = P (dP - delta), dQ = scale dS K and d(table) sums dS over pairs: max |dP| max |K|
    scale and max |dP| are what one pair contributes before delta is taken off.  With ONE key P = 1 and delta = dP: both
    gradients are exactly zero in the oracle, and what the kernels return is the rounding of O (16-bit) in delta times
    those terms -- err() measures such a gradient against the terms, every other against its own largest entry."""
    B, V, C, h, g, S, Wt, extra = geom
    ins = _problem(B, V, C, h, g, S, N, Wt, seed=seed, **dict(extra))
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
    with torch.no_grad():
        dp = torch.einsum("pmhc,pnhc->pmnh", cot.reshape(B * V, S * S, h, c), kv[:, :, C:].reshape(B * V, N, h, c)).abs().max()
        terms = (float(dp * kv[:, :, :C].abs().max() * c ** -0.5), float(dp))
    return ins, query.grad, table.grad, terms


def err(got, want, term):
    return (got - want).abs().max().item() / (want.abs().max().item() or term)


def check(geom, N, prec, seed, label):
    B, V, C, h, g, S, Wt, extra = geom
    ins, want_q, want_t, terms = problem_and_oracle(geom[:7] + (tuple(sorted(extra.items())),), N, seed)
    assert ops.slab_supported(prec, S)
    _, dq1, dt1, _, _ = _run(ins, h, g, V, prec, slab=True)
    _, dq0, dt0, _, _ = _run(ins, h, g, V, prec, slab=False)
    e1 = (err(dq1.cpu().double(), want_q, terms[0]), err(dt1.cpu().double(), want_t, terms[1]))
    e0 = (err(dq0.cpu().double(), want_q, terms[0]), err(dt0.cpu().double(), want_t, terms[1]))
    print(f"[bwd_q lanes {label} N={N} {TAG[prec]}] slab dQ {e1[0]:.2e} d(table) {e1[1]:.2e} | "
          f"tile dQ {e0[0]:.2e} d(table) {e0[1]:.2e}")
    assert math.isfinite(sum(e1) + sum(e0))
    lim = (LIMITS[prec]["query"], LIMITS[prec]["table"])
    for a, b_, l in zip(e1, e0, lim):
        assert a < l and b_ < l, (e1, e0, lim)
        assert a < 1.5 * b_ + 1e-3, (e1, e0)
        if prec == _lib.PREC_BF16:
            assert a < 1.5e-2, e1            # tests/test_gpu_slab.py: half the bf16 limit of tests/test_gpu_ops.py


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", KEY_COUNTS)
def test_key_counts_at_every_half_and_emission_boundary(N, prec):
    """every preload lane, every broadcast index and the masked tail of a partial half"""
    B, V, C, h, g, S, Wt, _ = NARROW
    assert Wt <= SLAB_W          # no wider than one slab: a column's run is (up to the slab cut) the whole key list
    check(NARROW, N, prec, seed=11 + N, label="narrow")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", [40, 70])
def test_clamped_body_far_keys_geometry(N, prec):
    """far_keys' geometry.  Its table is six slabs wide, so a column's run is a fraction of these key lists -- under 32
    keys: the far keys sit in the FIRST half of their emissions (asserted; seeds 1 .. 8 of either N give no other
    input).  The second half is the next test's"""
    ins = problem_and_oracle(FAR[:7] + (tuple(sorted(FAR[7].items())),), N, 5 + N)[0]
    assert 0 in far_halves(ins[2], FAR[5], FAR[6])
    check(FAR, N, prec, seed=5 + N, label="far")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", [40, 70])
def test_clamped_body_in_both_halves(N, prec):
    """the same share of far keys on the narrow table, where a run is most of the key list: both halves of an emission
    hold a key whose rows leave the window (asserted; the seed is one of those for which N = 40 does that)"""
    ins = problem_and_oracle(FAR_NARROW[:7] + (tuple(sorted(FAR_NARROW[7].items())),), N, 6)[0]
    assert far_halves(ins[2], FAR_NARROW[5], FAR_NARROW[6]) == {0, 1}
    check(FAR_NARROW, N, prec, seed=6, label="far-narrow")


@pytest.mark.parametrize("prec", PRECS)
def test_two_row_blocks_with_a_ragged_second_one(prec):
    S = TWO_BLOCKS[5]
    assert S == 31 + 9
    check(TWO_BLOCKS, 65, prec, seed=3, label="two-blocks")
