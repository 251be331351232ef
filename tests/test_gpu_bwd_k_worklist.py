"""The key-side backward entry points with a device work list (bevr_attn_bwd_k_ws, bevr_attn_tap_bwd_k_ws: the main launch
lists the units that miss its LDS window, a fixed grid runs exactly those) against the float64 oracle and against the
entry points without a list (bevr_attn_bwd_k, bevr_attn_tap_bwd_k) on the same operands.

S = 40 (two row blocks, the second ragged), 2 heads.  Region: 800 keys = three blocks of 384, the last one partial (32
live keys and 32 padded ones).  Tap: 600 keys = 19 live tiles in three workgroups of the main grid, the last live tile
partial.  Per kernel: no unit slow (an empty list), every unit slow, one slow unit in the middle, the partial last unit
slow, and every unit slow on TWO workgroups (items outnumber the workgroups many times).  The slow units of every case
are counted on the CPU by a restatement of the kernels' predicates.

Outputs that are stored (dK / dV rows of blocks on the window kernel) or summed by two commutative adds (the position
gradients of units that are never slow: one add per head) must be bit-equal between the two entry points.  Outputs summed
by float atomics over a split of the sweep differ in the order of the sums: they are held against the old entry point's
own spread over three runs as tools/route_trace.py judges a difference (2 x the spread), with a floor for the
reassociation itself -- 1e-5 of the largest entry for dK / dV and 1e-4 for the position gradients, the figures
tests/test_gpu_slab.py holds "equal up to the order of the float atomics" to (the new split is not the old one: even a
bit-stable old sum is reassociated)."""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

from bevrender_amd import _lib, ops
from oracle import bevrender_oracle as O
from test_gpu_fullsize import LIMITS, TAG, check_dpos, rel_err

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, HEADS, CH = 40, 2, 64
WT = 2 * S * 5 - 1
SPREAD_MARGIN = 2.0                  # tools/route_trace.py
FLOOR_KV, FLOOR_POS = 1e-5, 1e-4     # tests/test_gpu_slab.py

#        slow units        max_workgroups
CASES = {"none": ((), 0), "all": ((0, 1, 2), 0), "middle": ((1,), 0), "last": ((2,), 0), "all_two_wgs": ((0, 1, 2), 2)}


def summed_close(new, olds, floor, what):
    """`new` against three runs of the old entry point: inside SPREAD_MARGIN x their spread or the reassociation floor"""
    spread = max((olds[i] - olds[j]).abs().max().item() for i in range(3) for j in range(i))
    d = max((new - t).abs().max().item() for t in olds)
    big = max(t.abs().max().item() for t in olds)
    print(f"[worklist {what}] spread {spread:.3e} diff {d:.3e} largest entry {big:.3e}")
    assert torch.isfinite(new).all(), what
    assert d <= max(SPREAD_MARGIN * spread, floor * big), (what, d, spread, big)


# ---- region kernels ------------------------------------------------------------------------------------------
N_REGION, KEYS_WG = 800, 384


def region_inputs(slow):
    """Keys inside the grid (every block's table slab fits the ring); the blocks in `slow` spread over the whole padded
    table width instead, which no ring holds."""
    gen = torch.Generator().manual_seed(31 + sum(1 << b for b in slow))
    query = torch.randn(1, CH, S, S, generator=gen)
    kv = torch.randn(1, N_REGION, 2 * CH, generator=gen)
    pos = (torch.rand(1, N_REGION, 2, generator=gen) * 2 - 1) * 0.98
    for b in slow:
        n0, n1 = b * KEYS_WG, min(N_REGION, (b + 1) * KEYS_WG)
        pos[0, n0:n1, 1] = torch.linspace(-3.05, 3.05, n1 - n0)[torch.randperm(n1 - n0, generator=gen)]
    table = torch.randn(HEADS, 2 * S - 1, WT, generator=gen) * 0.3
    return query, kv, pos, table


def region_misfit_blocks(ka, kb, prec):
    """csrc/attn_bwd_k.hip (key_clamp, wg_key_box, make_slab) on the CPU: the key blocks the window kernel hands over"""
    Sp, Ht, Np = 32 * ((S + 31) // 32), 2 * S - 1, ka.shape[-1]
    a = ka.float().cpu().reshape(-1, Np).clamp(-(Sp + 1.0), Ht + 1.0)
    b = kb.float().cpu().reshape(-1, Np).clamp(-(WT // 2 + 2.0), WT + 1.0)
    wcap = 30720 if prec in (_lib.PREC_BF16, _lib.PREC_F16) else 26624
    rx_ceil = -(-(WT - 1) // (2 * (S - 1)))
    out = []
    for p in range(a.shape[0]):
        for blk in range(-(-Np // KEYS_WG)):
            n0, n1 = blk * KEYS_WG, min(N_REGION, (blk + 1) * KEYS_WG)
            if n1 <= n0:
                continue
            A, bb = a[p, n0:n1].floor(), b[p, n0:n1]
            rows = int(A.max() - A.min()) + Sp + 1
            pitch = rows + ((7 - rows) & 31)
            need = int(torch.floor(bb.max() - bb.min())) + 4 + rx_ceil + 1
            if wcap // pitch - 1 < need:
                out.append((p, blk))
    return out


@functools.lru_cache(maxsize=None)
def region_oracle(slow):
    ins = region_inputs(slow)
    query, kv, pos, table = (t.clone().double().requires_grad_(True) for t in ins)
    c = CH // HEADS
    q = query[0].reshape(HEADS, c, S * S)
    kk = kv[0, :, :CH].reshape(N_REGION, HEADS, c).permute(1, 2, 0)
    vv = kv[0, :, CH:].reshape(N_REGION, HEADS, c).permute(1, 2, 0)
    want = O.attention_core(q, kk, vv, pos, table, S, S, 1, c ** -0.5).reshape(CH, S * S).t()[None]
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(77)).double()
    want.backward(cot)
    return ins, cot.float(), kv.grad, pos.grad


def region_case(name, prec, monkeypatch):
    slow, max_wg = CASES[name]
    ins, cot, want_kv, want_pos = region_oracle(slow)
    got = {}

    def hook(entry, o):
        """ops' launch of the key-side backward: the operands as ops built them, through both entry points"""
        L = _lib.lib()
        ins_ptr = [ops._ptr(t) for t in (o.Qe, o.Qt, o.Ke, o.Ve, o.ka, o.kb, o.pair, o.dOe, o.dOt, o.LSE, o.delta, o.gscale)]

        def call(sym, outs, *extra):
            rc = getattr(L, sym)(C.byref(o.desc), *ins_ptr, *[ops._ptr(t) for t in outs], *extra, ops._stream())
            _lib.check(rc, sym)
            return outs

        def fresh():        # dK, dV are stored or cleared by the main launch: NaN shows a row nobody wrote
            return (torch.full_like(o.dK, float("nan")), torch.full_like(o.dV, float("nan")),
                    torch.zeros_like(o.da), torch.zeros_like(o.db))
        assert not o.da.any() and not o.db.any()
        got["old"] = [call("bevr_attn_bwd_k", fresh()) for _ in range(3)]
        ws = torch.empty(L.bevr_attn_bwd_k_ws_bytes(C.byref(o.desc)), device=o.dK.device, dtype=torch.uint8)
        got["new"] = [call("bevr_attn_bwd_k_ws", fresh(), ops._ptr(ws), max_wg) for _ in range(2)]     # one workspace, twice
        call("bevr_attn_bwd_k_ws", (o.dK, o.dV, o.da, o.db), ops._ptr(ws), max_wg)                     # the call's own result
        got["misfit"] = region_misfit_blocks(o.ka, o.kb, prec)
        got["Np"] = o.desc.Np
    monkeypatch.setitem(ops._RUN, ops.K.BWD_K, hook)
    query, kv, pos, table = (t.clone().to(DEV).requires_grad_(True) for t in ins)
    out = ops.attention_core(query, None, None, pos, table, heads=HEADS, groups=1, views=1, precision=prec, kv=kv)
    out.backward(cot.to(DEV))
    torch.cuda.synchronize()
    tag = f"region {name} {TAG[prec]}"

    # the case has the slow blocks it claims (one problem, one group: a block is slow for both heads)
    assert got["misfit"] == [(0, b) for b in slow], got["misfit"]
    # the float64 oracle, through ops' unpacking of what the work-list entry point returned
    lim = LIMITS[prec]
    e_k, e_v = rel_err(kv.grad[..., :CH].cpu(), want_kv[..., :CH]), rel_err(kv.grad[..., CH:].cpu(), want_kv[..., CH:])
    print(f"[worklist {tag}] d(k) {e_k:.3e} d(v) {e_v:.3e}")
    assert e_k < lim["k"] and e_v < lim["v"], (e_k, e_v)
    check_dpos(pos.grad, want_pos, ins[2], S, WT, lim["pos"], f"worklist {tag}")
    # the entry point without a list on the same operands
    blocks = [slice(b * KEYS_WG, min(got["Np"], (b + 1) * KEYS_WG)) for b in range(-(-got["Np"] // KEYS_WG))]
    for which, new in enumerate(got["new"]):
        for i, floor in ((0, FLOOR_KV), (1, FLOOR_KV), (2, FLOOR_POS), (3, FLOOR_POS)):
            for b, rows in enumerate(blocks):
                olds = [t[i][..., rows, :] if i < 2 else t[i][..., rows] for t in got["old"]]
                mine = new[i][..., rows, :] if i < 2 else new[i][..., rows]
                if b in slow:
                    summed_close(mine, olds, floor, f"{tag} call {which} {'dK dV da db'.split()[i]} block {b}")
                else:
                    assert all(torch.equal(mine, t) for t in olds), (tag, which, i, b)


@pytest.mark.parametrize("prec", [_lib.PREC_BF16, _lib.PREC_F16])
@pytest.mark.parametrize("name", list(CASES))
def test_region_bwd_k_from_the_work_list(name, prec, monkeypatch):
    region_case(name, prec, monkeypatch)


def test_region_bwd_k_from_the_work_list_in_f32(monkeypatch):
    region_case("middle", _lib.PREC_F32, monkeypatch)


# ---- tap kernels ---------------------------------------------------------------------------------------------
N_TAP, NKW = 600, 7
TAP_SLOW = {0: tuple(range(19)), 1: (9,), 2: (18,)}      # CASES' unit numbers -> tiles: every live tile, one in the middle
#                                                          workgroup, the partial last live tile (keys 576 .. 599)
TAP_LIMITS = {_lib.PREC_BF16: 3e-2, _lib.PREC_F16: 4e-3}  # tests/test_gpu_tap.py


def tap_tiles(units):
    return tuple(range(19)) if len(units) == 3 else tuple(t for u in units for t in TAP_SLOW[u])


def tap_unfit_tiles(ws, geom):
    """csrc/attn_tap_bwd_k.hip (tile_fits) and csrc/attn_tap.h (box_fits) on the CPU, on the boxes bevr_attn_tap_prep
    wrote: the tiles with a column that takes the per-pair gather"""
    nt = geom.Np // 32
    raw = ws[geom.n_prob * geom.Np * 16:][:geom.n_prob * nt * 16].cpu()
    bi, bf = raw.view(torch.int32).reshape(-1, nt, 4), raw.view(torch.float32).reshape(-1, nt, 4)
    rx = torch.tensor(float(geom.Wt - 1)) / torch.tensor(2.0 * (geom.S - 1))
    out = []
    for p in range(bi.shape[0]):
        for w0 in range(0, nt, NKW):
            live = [t for t in range(w0, min(nt, w0 + NKW)) if bi[p, t, 1] >= bi[p, t, 0]]
            a0w = min((int(bi[p, t, 0]) for t in live), default=0)
            bminw = min((bf[p, t, 2] for t in live), default=torch.tensor(0.0))
            for t in live:
                amin, amax, bmin, bmax = int(bi[p, t, 0]), int(bi[p, t, 1]), bf[p, t, 2], bf[p, t, 3]
                for j in range(geom.S):
                    jrx = torch.tensor(float(j)) * rx
                    x0, x1 = int(torch.floor(jrx + bmin)), int(torch.floor(jrx + bmax)) + 1
                    dx, da = x0 - int(torch.floor(jrx + bminw)), amin - a0w
                    if not (0 <= da <= 8 and x1 - x0 < 4 and amax + 1 - amin < 4 and 0 <= dx <= 4):
                        out.append((p, t))
                        break
    return out


@functools.lru_cache(maxsize=None)
def tap_problem(tiles, prec):
    """Keys of one table cell row and under two table columns: every tile's taps fit one chunk of its workgroup's window
    in every column.  The tiles in `tiles` span six table rows instead (from the same first row: the windows' origins
    stay where they are), which no chunk holds.  Returns the operands and the float64 gradients."""
    import tap_check as tc
    f16 = prec == _lib.PREC_F16
    geom, a, b, ys, xs, G, Gb, T = tc.make_case(P=1, h=HEADS, S=S, N=N_TAP, Wt=WT, seed=41, prec=prec,
                                                gscale=2.0 if f16 else 4.0)
    gen = torch.Generator().manual_seed(43 + len(tiles))
    a[:, :N_TAP] = ((S - 1) + 0.1 + 1.8 * torch.rand(1, N_TAP, generator=gen)).to(DEV)
    b[:, :N_TAP] = ((WT - 1) / 2.0 + 0.1 + 1.5 * torch.rand(1, N_TAP, generator=gen)).to(DEV)
    for t in range(N_TAP // 32 + 1):
        a[:, 32 * t] = (S - 1) + 0.1                  # every tile starts in table row S - 1
        if t in tiles:
            a[:, 32 * t + 1:min(N_TAP, 32 * t + 32)] += torch.linspace(0.0, 4.9, min(N_TAP, 32 * t + 32) - 32 * t - 1).to(DEV)
    headroom = 8.0 if f16 else 64.0
    _, _, _, ws, pair = tc.run_fwd(geom, a, b, ys, xs, G, Gb, T, headroom)
    T2 = T.double() * ops.LOG2E
    _, LSE = tc.reference(G.float(), Gb, a, b, ys, xs, T2, S, WT, N_TAP, None)
    gen = torch.Generator(device=DEV).manual_seed(99)
    valid = (torch.arange(geom.Mp, device=DEV) % geom.Sp) < S
    H = torch.zeros(1, HEADS, geom.Mp, 16, device=DEV)
    H[..., :12] = torch.randn(1, HEADS, geom.Mp, 12, device=DEV, generator=gen)
    H = (H * valid[None, None, :, None]).to(G.dtype)
    Hc = (torch.randn(1, HEADS, geom.Mp, device=DEV, generator=gen) * valid).contiguous()
    lse_p = torch.full((1, HEADS, S, geom.Sp), 30000.0 if f16 else 1.0e30, device=DEV, dtype=torch.float64)
    lse_p[:, :, :, :S] = LSE
    Gc = (Gb.double() - lse_p.reshape(1, HEADS, geom.Mp)).float().contiguous()
    want = tc.grad_reference(G.float(), Gb, H.float(), Hc, a, b, ys, xs, T2, S, WT, N_TAP, LSE)[2:]
    Gk, Hk = G.clone(), H.clone()
    tc.set_offset(Gk, Gc)
    tc.set_offset(Hk, Hc)
    return geom, Gk, Hk, ws, ops.pack_table(T.float(), geom).contiguous(), [w.cpu() for w in want]


@pytest.mark.parametrize("prec", [_lib.PREC_BF16, _lib.PREC_F16])
@pytest.mark.parametrize("name", list(CASES))
def test_tap_bwd_k_from_the_work_list(name, prec):
    units, max_wg = CASES[name]
    tiles = tap_tiles(units)
    geom, G, H, ws, Tt, want = tap_problem(tiles, prec)
    assert tap_unfit_tiles(ws, geom) == [(0, t) for t in tiles]
    L = _lib.lib()
    d = geom.desc()

    def call(sym, *extra):
        outs = [torch.zeros(1, geom.Np, device=DEV) for _ in range(4)]
        rc = getattr(L, sym)(C.byref(d), ops._ptr(G), ops._ptr(H), ops._ptr(ws), ops._ptr(Tt), *[ops._ptr(t) for t in outs],
                             *extra, ops._stream())
        _lib.check(rc, sym)
        torch.cuda.synchronize()
        return outs
    olds = [call("bevr_attn_tap_bwd_k") for _ in range(3)]
    lws = torch.empty(L.bevr_attn_tap_bwd_k_ws_bytes(C.byref(d)), device=DEV, dtype=torch.uint8)
    news = [call("bevr_attn_tap_bwd_k_ws", ops._ptr(lws), max_wg) for _ in range(2)]                 # one workspace, twice
    tag = f"tap {name} {TAG[prec]}"
    slow_keys = torch.zeros(geom.Np, dtype=torch.bool, device=DEV)
    for t in tiles:
        slow_keys[32 * t:32 * t + 32] = True
    for which, new in enumerate(news):
        for i, what in enumerate(("da", "db", "dys", "dxs")):
            e = rel_err(new[i][:, :N_TAP].cpu(), want[i])
            print(f"[worklist {tag}] call {which} {what} {e:.3e}")
            assert e < TAP_LIMITS[prec], (what, e)
            # keys of tiles that are never slow: one add per head from the main launch, in either order
            assert all(torch.equal(new[i][:, ~slow_keys], t[i][:, ~slow_keys]) for t in olds), (tag, which, what)
            if tiles:
                summed_close(new[i][:, slow_keys], [t[i][:, slow_keys] for t in olds], FLOOR_POS, f"{tag} call {which} {what}")
