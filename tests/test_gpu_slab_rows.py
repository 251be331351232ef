"""The slab query-side backward in row bands (csrc/attn_slab_bwd_q_rows.hip, bevr_attn_slab_bwd_q_rows; BEV sides up to
448) through ops.attention_core, behind its switch BEVR_SLAB_ROWS:

  * small grids through the tall instantiation, cut into bands of one and of two row blocks (ops.SLAB_BAND_BLOCKS
    patched), against the query-tile kernel on a dense cotangent and against the float64 materialised oracle -- the rules
    of tests/test_gpu_slab.py;
  * tall grids (two and three bands, both row pitches) against the float64 oracle on sampled rows -- the rules of
    tests/test_gpu_gather_rows.py:test_tall_grids_rows_and_gradients; the cotangent is zero on every other row, so a band
    that wrote dQ outside its rows would fail the full-tensor comparison;
  * S = 400 against the query-tile kernel on a dense cotangent.

Every test prints its figures before it asserts (-s); the recorded run is profiles/r12_slab_rows.txt."""
import os

import pytest
import torch

from bevrender_amd import _lib, ops
from test_gpu_fullsize import LIMITS, check_dpos, oracle_rows, pick_rows
from test_gpu_fullsize import rel_err as rel_err_rows
from test_gpu_gather import _problem as _problem_kv
from test_gpu_slab import _problem, rel_err
from oracle import bevrender_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = _lib.PREC_BF16, _lib.PREC_F16
TAG = {BF16: "bf16", F16: "f16"}
SLAB, TILE = "bevr_attn_slab_bwd_q", "bevr_attn_bwd_q"          # the timer's names of the two routes
AB_LIM = {BF16: 1e-2, F16: 2e-3}          # tests/test_gpu_slab.py: the modes' own errors (one tap-weight rounding apart)


def _route_env(monkeypatch, rows):
    """rows: the BEVR_SLAB_ROWS value of the route under test; None: the query-tile kernel (both slab routes off)"""
    if rows is None:
        monkeypatch.setenv("BEVR_SLAB", "0")
        monkeypatch.delenv("BEVR_SLAB_ROWS", raising=False)
    else:
        monkeypatch.delenv("BEVR_SLAB", raising=False)
        monkeypatch.setenv("BEVR_SLAB_ROWS", rows)


def _run_kv(ins, h, g, V, prec):
    """ops.attention_core on (query, kv, pos, table) with test_gpu_slab.py's dense cotangent: outputs, gradients and the
    kernels the timer saw"""
    query, kv, pos, table = (t.clone().to(DEV).requires_grad_(True) for t in ins)
    ops.KERNEL_TIMER.start()
    out = ops.attention_core(query, None, None, pos, table, heads=h, groups=g, views=V, precision=prec, kv=kv)
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(77)).to(DEV)
    out.backward(cot)
    used = ops.KERNEL_TIMER.stop()
    return dict(out=out.detach(), dq=query.grad, dt=table.grad, dkv=kv.grad, dp=pos.grad), used


# ---- small grids through the tall instantiation -----------------------------------------------------------------------
SMALL = {
    #                 B  V  C   h  g  S   N     Wt                extra
    "three_blocks": (1, 1, 64, 2, 1, 70, 1500, 2 * 70 * 2 - 1, {}),
    "ragged_wide": (1, 1, 64, 2, 1, 63, 333, 2 * 63 * 5 - 1, {}),          # row block 2 holds one row; a table of 52 slabs
    "far_two_views": (1, 2, 64, 2, 1, 70, 700, 2 * 70 * 3 - 1, {"far": 0.3}),          # the clamped body at rb0 > 0
    "groups": (1, 1, 64, 4, 2, 40, 400, 2 * 40 * 3 - 1, {}),
    "one_key": (1, 1, 64, 2, 1, 33, 1, 2 * 33 * 5 - 1, {}),
}
_small_ref = {}


def _small_reference(name, prec, monkeypatch):
    """the query-tile route's results (per mode) and the float64 oracle's gradients (once per case), computed once"""
    B, V, C, h, g, S, N, Wt, extra = SMALL[name]
    ins = _problem(B, V, C, h, g, S, N, Wt, seed=len(name) + 7 * S, **extra)
    if (name, prec) not in _small_ref:
        _route_env(monkeypatch, None)
        res, used = _run_kv(ins, h, g, V, prec)
        assert TILE in used and SLAB not in used, sorted(used)
        _small_ref[name, prec] = res
    if (name, "oracle") not in _small_ref and N > 1:
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
        want.backward(torch.randn(want.shape, generator=torch.Generator().manual_seed(77)).double())
        _small_ref[name, "oracle"] = (query.grad, table.grad)
    return ins, _small_ref[name, prec], _small_ref.get((name, "oracle"))


@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(SMALL))
def test_small_grids_in_bands_of_one_and_two_row_blocks(name, prec, blocks, monkeypatch):
    """BEVR_SLAB_ROWS=2 with a band of `blocks` row blocks: every worker arrangement a tall grid has (first block above
    0, idle workers, a ragged last block) at sizes where the whole gradient is compared.  Against the query-tile kernel:
    the forward bit-equal, the key side equal up to its atomics' order, dQ and d(table) within the modes' limits.  bf16
    against the float64 oracle too: no less accurate than the query-tile kernel (1.5 x + 1e-3) and under 1.5e-2.  (One
    key: the softmax weight is 1 and both gradients are identically zero in the oracle, which leaves the relative rule
    nothing to divide by; that case is compared with the query-tile kernel alone, as tests/test_gpu_slab.py has it.)"""
    B, V, C, h, g, S, N, Wt, extra = SMALL[name]
    ins, tile, oracle = _small_reference(name, prec, monkeypatch)
    monkeypatch.setattr(ops, "SLAB_BAND_BLOCKS", blocks)
    bands = ops.slab_bands(S)
    assert len(bands) == -(-(-(-S // 31)) // blocks) and (len(bands) > 1 or S <= 31 * blocks)
    _route_env(monkeypatch, "2")
    assert ops.slab_rows_supported(prec, S, Wt)
    got, used = _run_kv(ins, h, g, V, prec)
    tag = f"rows vs tile {name} {TAG[prec]} blocks={blocks}"
    print(f"\n[{tag}] bands {bands}; slab launches {used.get(SLAB, {}).get('n')}")
    assert SLAB in used and used[SLAB]["n"] == len(bands) and TILE not in used, sorted(used)
    assert torch.equal(got["out"], tile["out"])          # the forward does not depend on the switch
    e_kv, e_p = rel_err(got["dkv"], tile["dkv"]), rel_err(got["dp"], tile["dp"])
    e_q, e_t = rel_err(got["dq"], tile["dq"]), rel_err(got["dt"], tile["dt"])
    print(f"[{tag}] dK|V {e_kv:.2e} d(pos) {e_p:.2e} dQ {e_q:.2e} d(table) {e_t:.2e}")
    assert e_kv < 1e-5 and e_p < 1e-4, (e_kv, e_p)
    assert e_q < AB_LIM[prec] and e_t < AB_LIM[prec], (e_q, e_t)
    assert got["dt"].abs().sum() > 0 or N == 1
    if prec == BF16 and oracle is not None:
        e1 = (rel_err(got["dq"].cpu().double(), oracle[0]), rel_err(got["dt"].cpu().double(), oracle[1]))
        e0 = (rel_err(tile["dq"].cpu().double(), oracle[0]), rel_err(tile["dt"].cpu().double(), oracle[1]))
        print(f"[vs oracle {name} blocks={blocks}] rows dQ {e1[0]:.2e} d(table) {e1[1]:.2e} | tile dQ {e0[0]:.2e} d(table) {e0[1]:.2e}")
        for a, b in zip(e1, e0):
            assert a < 1.5e-2 and a < 1.5 * b + 1e-3, (e1, e0)


# ---- tall grids against the oracle on sampled rows ----------------------------------------------------------------------
def slab_band_rows(S, bands, j0):
    """query indices m = i S + j: the first and last BEV row of every band (columns j0 and S - 1 - j0) and row S - 1"""
    rows = [i * S + j for r0, n in bands for i in (r0, r0 + n - 1) for j in (j0, S - 1 - j0)]
    rows += [(S - 1) * S + j0, (S - 1) * S + S - 1]
    return torch.tensor(sorted(set(rows)))


def _spread(u):
    return (u * 2 - 1) * 0.9


def _far(u):
    """20 % of the keys four times as far out: table rows and columns beyond the table's ends"""
    m = torch.rand(u.shape[:-1] + (1,), generator=torch.Generator().manual_seed(5)) < 0.2
    p = _spread(u)
    return torch.where(m, p * 4.0, p)


_tall_ref = {}


def _tall_reference(S, pos_fn):
    """inputs, sampled rows, their cotangent and the float64 oracle's results: once per (S, key set), for both modes"""
    key = (S, pos_fn.__name__)
    if key not in _tall_ref:
        Cc, h, D, N = 64, 2, 5, 1500
        ins = _problem_kv(1, 1, Cc, h, S, D, N, 900 + S, pos_fn)
        p = dict(query=ins[0], k=ins[1], v=ins[2], pos=ins[3], table=ins[4])
        bands = ops.slab_bands(S, 7)
        must = slab_band_rows(S, bands, 11)
        rows = torch.unique(torch.cat((pick_rows(S, 72, S), must)))
        assert all(int(m) in set(rows.tolist()) for m in must)
        cot = torch.randn(1, len(rows), Cc, generator=torch.Generator().manual_seed(8))
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        want, grads = oracle_rows(p, h, rows, cot)
        _tall_ref[key] = (p, rows, cot, want, grads)
    return _tall_ref[key]


def _run_tall(S, prec, pos_fn, monkeypatch):
    p, rows, cot, want, grads = _tall_reference(S, pos_fn)
    monkeypatch.delenv("BEVR_SLAB", raising=False)
    monkeypatch.setenv("BEVR_SLAB_ROWS", "1")
    bands = ops.slab_bands(S)
    dev = {n: p[n].clone().to(DEV).requires_grad_(True) for n in ("query", "k", "v", "pos", "table")}
    ops.KERNEL_TIMER.start()
    out = ops.attention_core(dev["query"], dev["k"], dev["v"], dev["pos"], dev["table"], heads=2, groups=1, views=1,
                             precision=prec)
    cot_full = torch.zeros_like(out)
    cot_full[:, rows.to(DEV)] = cot.to(DEV)
    out.backward(cot_full)
    used = ops.KERNEL_TIMER.stop()
    print(f"\n[tall S={S} {TAG[prec]} {pos_fn.__name__}] bands {bands}; slab launches {used.get(SLAB, {}).get('n')}")
    assert SLAB in used and used[SLAB]["n"] == len(bands) and TILE not in used, sorted(used)
    assert torch.isfinite(out).all()
    return p, rows, want, grads, out, dev


@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("S", [218, 400, 404, 448])
def test_tall_grids_rows_and_gradients(S, prec, monkeypatch):
    """BEVR_SLAB_ROWS=1, D = 5, 1 500 scattered keys: 218 the smallest side with two bands, 400 config 5's (the 832-row
    pitch), 404 the first side on the 960-row pitch, 448 the limit (three bands).  Forward and every gradient on sampled
    rows -- random ones, the first and last row of every band in two columns, row S - 1 -- against the float64 oracle at
    tests/test_gpu_fullsize.py's LIMITS; the slab kernel ran once per band, the query-tile kernel did not."""
    assert len(ops.slab_bands(S)) == {218: 2, 400: 2, 404: 2, 448: 3}[S]
    p, rows, want, grads, out, dev = _run_tall(S, prec, _spread, monkeypatch)
    lim, tag = LIMITS[prec], f"tall S={S} {TAG[prec]}"
    got_rows = out.detach()[:, rows.to(DEV)].cpu().double()
    per_row = (got_rows - want).abs().amax(-1)[0] / want.abs().max().item()
    print(f"[{tag}] out rel err {per_row.max().item():.3e} (worst row m = {int(rows[per_row.argmax()])})")
    errs = {n: rel_err_rows(dev[n].grad.cpu(), grads[n]) for n in ("query", "k", "v", "table")}
    for n, e in errs.items():
        print(f"[{tag}] grad {n:6s} rel err {e:.3e}  (max |want| {grads[n].abs().max().item():.3e})")
    assert per_row.max().item() < lim["out"], f"{tag}: out {per_row.max().item():.3e}"
    for n, e in errs.items():
        assert e < lim[n], f"{tag}: grad {n}: {e:.3e}"
    check_dpos(dev["pos"].grad, grads["pos"], p["pos"], S, p["table"].shape[-1], lim["pos"], tag,
               cols=(rows % S).tolist(), min_clean=0.3)


@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "f16"])
def test_tall_grid_with_keys_far_outside_the_table(prec, monkeypatch):
    """S = 218 with 20 % of the keys at four times their distance: 32-key halves that take the clamped body in a worker
    whose row block is not the column's first seven.  out, d(query) and d(table) on the sampled rows (the key side is
    the key-side kernel's, which this route does not touch)."""
    S = 218
    p, rows, want, grads, out, dev = _run_tall(S, prec, _far, monkeypatch)
    a = (1.0 - p["pos"][..., 0]) * ((S - 1) / 2.0)
    assert ((a < -10) | (a > S - 1 + 8)).float().mean() > 0.05          # keys outside the window's unclamped rows
    lim, tag = LIMITS[prec], f"tall far S={S} {TAG[prec]}"
    e_out = rel_err_rows(out.detach()[:, rows.to(DEV)].cpu(), want)
    errs = {n: rel_err_rows(dev[n].grad.cpu(), grads[n]) for n in ("query", "table")}
    print(f"[{tag}] out {e_out:.3e} grad query {errs['query']:.3e} grad table {errs['table']:.3e}")
    assert e_out < lim["out"] and errs["query"] < lim["query"] and errs["table"] < lim["table"], (e_out, errs)


# ---- config 5's side against the query-tile kernel -------------------------------------------------------------------
def test_bev400_dense_cotangent_agrees_with_the_query_tile_kernel(monkeypatch):
    """S = 400, fp16, 600 keys, a dense cotangent: every row of both bands, dQ and d(table) against the query-tile route
    within the fp16 A/B limit of tests/test_gpu_slab.py."""
    S, N, h = 400, 600, 2
    ins = _problem(1, 1, 64, h, 1, S, N, 2 * S * 5 - 1, seed=400)
    _route_env(monkeypatch, None)
    tile, used0 = _run_kv(ins, h, 1, 1, F16)
    _route_env(monkeypatch, "1")
    got, used1 = _run_kv(ins, h, 1, 1, F16)
    assert TILE in used0 and SLAB not in used0 and TILE not in used1 and used1[SLAB]["n"] == 2, (sorted(used0), sorted(used1))
    e_q, e_t = rel_err(got["dq"], tile["dq"]), rel_err(got["dt"], tile["dt"])
    print(f"\n[S=400 fp16 rows vs tile] dQ {e_q:.2e} d(table) {e_t:.2e}")
    assert torch.equal(got["out"], tile["out"])
    assert e_q < AB_LIM[F16] and e_t < AB_LIM[F16], (e_q, e_t)
