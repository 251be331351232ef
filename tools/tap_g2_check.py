"""Tap kernels for two channel groups (csrc/attn_tap_*_g2.hip) against a float64 restatement of their definition
(include/bevrender_hip.h, "TAP entry points for TWO CHANNEL GROUPS"), and their reduction to the one-group entry points.
    python tools/tap_g2_check.py        small random cases, forward and both backward entry points"""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bevrender_amd import ops, _lib  # noqa: E402
import tap_check as tc  # noqa: E402

dev = "cuda"
NG = 2


def tap_w32(ys, xs, dtype=torch.float64):
    """ys, xs (..., 2, N): both groups' positions -> (..., N, 32) slot weights: block 0 = tap_check.tap_w of group 0
    (slot 15 = 1), block 1 = group 1's 12 taps and zeros."""
    w0 = tc.tap_w(ys[..., 0, :], xs[..., 0, :], dtype)
    w1 = tc.tap_w(ys[..., 1, :], xs[..., 1, :], dtype).clone()
    w1[..., 12:] = 0
    return torch.cat((w0, w1), -1)


TAPS = list(range(12)) + list(range(16, 28))        # the 24 tap slots of a 32-slot row


def reference(G, Gb, a, b, ys, xs, T2, S, Wt, N, mimic=None, with_max=False):
    """float64 definition.  G (P, h, Mp, 32), Gb (P, h, Mp) values; a, b (2P, Np), ys, xs (2P, 2, Np) the rows' arrays.
    Returns Rn (P, h, S(j), S(i), 32) normalised, LSE (P, h, S, S).  Head hd reads row p * 2 + hd // (h / 2).
    with_max: a third value, the rows' largest logit (P, h, S, S)."""
    P, h, Mp, _ = G.shape
    Sp = Mp // S
    hg = h // NG
    Gd = G.double().reshape(P, h, S, Sp, 32)[:, :, :, :S]
    Gbd = Gb.double().reshape(P, h, S, Sp)[:, :, :, :S]
    w = tap_w32(ys[..., :N], xs[..., :N])                      # (2P, N, 32)
    if mimic is not None:
        w = tc._mim(w, mimic)
        T2 = tc._mim(T2, mimic)
    Rn = torch.zeros(P, h, S, S, 32, dtype=torch.float64, device=G.device)
    LSE = torch.zeros(P, h, S, S, dtype=torch.float64, device=G.device)
    MAX = torch.zeros(P, h, S, S, dtype=torch.float64, device=G.device)
    for p in range(P):
        for g in range(NG):
            r, hs = p * NG + g, slice(g * hg, (g + 1) * hg)
            for j in range(S):
                bia = tc.bias_ref(T2[hs], a[r, :N].double(), b[r, :N], S, Wt, j, mimic)                 # (hg, S, N)
                lg = torch.einsum("hit,nt->hin", Gd[p, hs, j][..., TAPS], w[r][:, TAPS]) + Gbd[p, hs, j, :, None] + bia
                m = lg.amax(-1, keepdim=True)
                pr = torch.exp2(lg - m)
                l = pr.sum(-1, keepdim=True)
                LSE[p, hs, j] = (m + torch.log2(l))[..., 0]
                MAX[p, hs, j] = m[..., 0]
                Rn[p, hs, j] = torch.einsum("hin,nt->hit", pr / l, w[r])
    return (Rn, LSE, MAX) if with_max else (Rn, LSE)


def grad_reference(G, Gb, H, Hc, a, b, ys, xs, T2, S, Wt, N, LSE):
    """float64 gradients through autograd of tap_check.grad_reference's pseudo-loss.  Returns dG (P, h, S, S, 32), dT2,
    da, db (2P, N), dys, dxs (2P, 2, N): per row, summed over the heads of the row's group."""
    P, h, Mp, _ = G.shape
    Sp = Mp // S
    hg = h // NG
    Gd = G.double().reshape(P, h, S, Sp, 32)[:, :, :, :S]
    Hd = H.double().reshape(P, h, S, Sp, 32)[:, :, :, :S]
    Gbd = Gb.double().reshape(P, h, S, Sp)[:, :, :, :S]
    Hcd = Hc.double().reshape(P, h, S, Sp)[:, :, :, :S]
    al, bl, yl, xl = (t[..., :N].double().clone().requires_grad_(True) for t in (a, b, ys, xs))
    T2l = T2.clone().requires_grad_(True)
    dG = torch.zeros(P, h, S, S, 32, dtype=torch.float64, device=G.device)
    for p in range(P):
        for g in range(NG):
            r, hs = p * NG + g, slice(g * hg, (g + 1) * hg)
            w = tap_w32(yl[r], xl[r])
            for j in range(S):
                bia = tc.bias_ref(T2l[hs], al[r], bl[r], S, Wt, j)
                lg = torch.einsum("hit,nt->hin", Gd[p, hs, j][..., TAPS], w[:, TAPS]) + Gbd[p, hs, j, :, None] + bia
                Pm = torch.exp2(lg - LSE[p, hs, j, :, None]).detach()
                dpl = torch.einsum("hit,nt->hin", Hd[p, hs, j][..., TAPS], w[:, TAPS])
                dS = (Pm * (dpl + Hcd[p, hs, j, :, None])).detach()
                dG[p, hs, j] = torch.einsum("hin,nk->hik", dS, w.detach())
                ((dS * lg).sum() + (Pm * dpl).sum() * ops.LOG2E).backward(retain_graph=True)
    return dG, T2l.grad, al.grad, bl.grad, yl.grad, xl.grad


def make_case(P, h, S, N, Wt, spread=(5.0, 2.5), gscale=4.0, seed=0, prec=_lib.PREC_BF16, sort=True, host_rng=False,
              row_scale=None, unseen=None):
    """The two groups' positions are drawn independently; every row p * 2 + g is cell-sorted by its own group's table
    coordinates with `sort` (ops.tap_group_order), else all rows keep the drawn order.
    host_rng, row_scale, unseen: as tap_check.make_case (unseen: slot tap_check.UNSEEN_TAP of group 0's block)."""
    gd = "cpu" if host_rng else dev
    gen = torch.Generator(device=gd).manual_seed(seed)
    ed = torch.bfloat16 if prec == _lib.PREC_BF16 else torch.float16
    geom = ops.AttnGeom(n_prob=P, q_div=1, heads=h, groups=NG, S=S, N=N, Wt=Wt, precision=prec)
    per = [tc.draw_keys(P, S, N, Wt, spread, False, gen) for _ in range(NG)]
    a, b, ys, xs = (torch.stack([per[g][k] for g in range(NG)], 1).reshape(P * NG, N).to(dev) for k in range(4))
    if sort:
        _, a, b, ys, xs = ops.tap_group_order(a, b, ys, xs, NG)
    else:
        ys, xs = (t.reshape(P, 1, NG, N).expand(-1, NG, -1, -1).reshape(P * NG, NG, N) for t in (ys, xs))
    pad = geom.Np - N
    a, b, ys, xs = (torch.nn.functional.pad(t, (0, pad)).contiguous() for t in (a, b, ys, xs))
    G = torch.zeros(P, h, geom.Mp, 32, device=dev)
    G[..., TAPS] = torch.randn(P, h, geom.Mp, 24, device=gd, generator=gen).to(dev) \
        * (gscale if row_scale is None else row_scale(geom)[None, None, :, None])
    if unseen is not None:
        G[..., tc.UNSEEN_TAP] = unseen
    valid = (torch.arange(geom.Mp, device=dev) % geom.Sp) < S
    G = G * valid[None, None, :, None]
    G[..., 14] = -1.0e30 if prec == _lib.PREC_BF16 else -60000.0
    Gb = torch.randn(P, h, geom.Mp, device=gd, generator=gen).to(dev) * valid
    T = torch.randn(h, 2 * S - 1, Wt, device=gd, generator=gen).to(dev) * 0.5
    return geom, a, b, ys, xs, G.to(ed), Gb.contiguous(), T


def prep(geom, a, b, ys, xs):
    L = _lib.lib()
    d = geom.desc()
    ws = torch.empty(L.bevr_attn_tap_g2_ws_bytes(C.byref(d)), device=dev, dtype=torch.uint8)
    _lib.check(L.bevr_attn_tap_g2_prep(C.byref(d), ops._ptr(a), ops._ptr(b), ops._ptr(ys), ops._ptr(xs), ops._ptr(ws),
                                       ops._stream()), "tap_g2_prep")
    return ws


def static_reference(geom, G, Gb, T, headroom):
    """tap_check.static_reference for two groups: the bound is a SUM over the groups."""
    tmax = (T.float() * ops.LOG2E).amax((1, 2)).clamp_min(0)
    U = (G[..., :12].float().amax(-1).clamp_min(0) + G[..., 16:28].float().amax(-1).clamp_min(0)) * 1.01 + Gb \
        + tmax[None, :, None] * 1.01 + 0.01
    G = G.clone()
    return G, (Gb - tc.set_offset(G, Gb - (U - headroom))).contiguous()


def run_fwd(geom, a, b, ys, xs, G, Gb, T, headroom=64.0):
    L = _lib.lib()
    d = geom.desc()
    Tt = ops.pack_table(T.float(), geom)
    pair = torch.stack((Tt[..., :-1], Tt[..., 1:]), dim=-1).contiguous()
    ws = prep(geom, a, b, ys, xs)
    G, mref = static_reference(geom, G, Gb, T, headroom)
    R = torch.empty(geom.n_prob, geom.heads, geom.Mp, 32, device=dev, dtype=torch.float32)
    flags = torch.zeros(geom.n_prob * geom.heads, geom.S, device=dev, dtype=torch.int32)
    _lib.check(L.bevr_attn_tap_g2_fwd(C.byref(d), ops._ptr(G), ops._ptr(ws), ops._ptr(pair), ops._ptr(mref), ops._ptr(R),
                                      ops._ptr(flags), ops._stream()), "tap_g2_fwd")
    return R, mref, flags, ws, pair


def _offsets(G, Gc, H, Hc):
    G, H = G.clone(), H.clone()
    tc.set_offset(G, Gc)
    tc.set_offset(H, Hc)
    return G, H


def run_bwd_q(geom, G, Gc, H, Hc, ws, pair):
    L = _lib.lib()
    d = geom.desc()
    G, H = _offsets(G, Gc, H, Hc)
    dG = torch.empty(geom.n_prob, geom.heads, geom.Mp, 32, device=dev, dtype=torch.float32)
    dT = torch.zeros(geom.heads, geom.Wp, geom.Hp + 1, device=dev, dtype=torch.float32)
    _lib.check(L.bevr_attn_tap_g2_bwd_q(C.byref(d), ops._ptr(G), ops._ptr(H), ops._ptr(ws), ops._ptr(pair), ops._ptr(dG),
                                        ops._ptr(dT), ops._stream()), "tap_g2_bwd_q")
    torch.cuda.synchronize()
    return dG, dT


def run_bwd_k(geom, G, Gc, H, Hc, ws, Tt):
    L = _lib.lib()
    d = geom.desc()
    G, H = _offsets(G, Gc, H, Hc)
    R2 = geom.n_prob * NG
    outs = [torch.zeros(R2, geom.Np, device=dev, dtype=torch.float32) for _ in range(2)]
    outs += [torch.zeros(R2, NG, geom.Np, device=dev, dtype=torch.float32) for _ in range(2)]
    _lib.check(L.bevr_attn_tap_g2_bwd_k(C.byref(d), ops._ptr(G), ops._ptr(H), ops._ptr(ws), ops._ptr(Tt),
                                        *[ops._ptr(t) for t in outs], ops._stream()), "tap_g2_bwd_k")
    torch.cuda.synchronize()
    return outs


def relerr(got, want):
    return tc.relerr(got, want)


def draw_cotangent(geom, ed, seed=99):
    gen = torch.Generator(device=dev).manual_seed(seed)
    valid = ((torch.arange(geom.Mp, device=dev) % geom.Sp) < geom.S)
    H = torch.zeros(geom.n_prob, geom.heads, geom.Mp, 32, device=dev)
    H[..., TAPS] = torch.randn(geom.n_prob, geom.heads, geom.Mp, 24, device=dev, generator=gen)
    H = (H * valid[None, None, :, None]).to(ed)
    Hc = (torch.randn(geom.n_prob, geom.heads, geom.Mp, device=dev, generator=gen) * valid).contiguous()
    return H, Hc


def check_case(name, **kw):
    """One case through the four entry points; returns tap_check.check_case's figures: 'exact' / 'mimic' = (Rn, LSE)
    errors against the float64 definition on the given operands / on the operands as the kernels round them, and the
    gradients' relative errors (of the largest entry)."""
    headroom = kw.pop("headroom", 64.0)
    forward_only = kw.pop("forward_only", False)   # the forward's figures alone (flags, per-row slack)
    geom, a, b, ys, xs, G, Gb, T = make_case(**kw)
    R, mref, flags, ws, pair = run_fwd(geom, a, b, ys, xs, G, Gb, T, headroom)
    torch.cuda.synchronize()
    P, h, S, Sp, N = geom.n_prob, geom.heads, geom.S, geom.Sp, geom.N
    Rg = R.double().reshape(P, h, S, Sp, 32)[:, :, :, :S]
    mr = mref.double().reshape(P, h, S, Sp)[:, :, :, :S]
    # (mref as the kernel was GIVEN it: the exact pass has rewritten the flagged columns of `mref`)
    mr0 = static_reference(geom, G, Gb, T, headroom)[1].double().reshape(P, h, S, Sp)[:, :, :, :S]
    l = Rg[..., 15]
    Rn_got = Rg / l[..., None]
    lse_got = mr + torch.log2(l)
    mim = torch.bfloat16 if geom.precision == _lib.PREC_BF16 else torch.float16
    T2 = T.double() * ops.LOG2E
    out = {}
    sel = TAPS + [14, 15, 28, 29, 30, 31]
    for tag, mm in (("exact", None), ("mimic", mim)):
        Rn, LSE, MAX = reference(G.float(), Gb, a, b, ys, xs, T2, S, geom.Wt, N, mm, with_max=True)
        out[tag] = ((Rn_got[..., sel] - Rn[..., sel]).abs().max().item(), (lse_got - LSE).abs().max().item())
        out[tag + "_rows"] = dict(lsum_log2=(LSE - mr0).cpu(), slack=(mr0 + headroom - MAX).cpu(),
                                  lse_err=(lse_got - LSE).abs().cpu())    # tap_check.check_case
        if mm is None:
            LSE_exact = LSE
    out["flags"] = flags.reshape(P, h, S).cpu()
    out["finite_G"] = bool(torch.isfinite(G.float()).all())
    if forward_only:
        out.update(flagged=int(flags.sum()), dead=Rn_got[..., 14].abs().max().item())
        print(f"{name:24s} flagged {out['flagged']}  Rn err mimic {out['mimic'][0]:.2e}  LSE err mimic {out['mimic'][1]:.2e}")
        return out
    print(f"{name:24s} flagged {int(flags.sum())}  Rn err exact {out['exact'][0]:.2e} mimic {out['mimic'][0]:.2e}   "
          f"LSE err exact {out['exact'][1]:.2e} mimic {out['mimic'][1]:.2e}")
    H, Hc = draw_cotangent(geom, G.dtype)
    LSE = LSE_exact
    lse_p = torch.full((P, h, S, Sp), 1.0e30 if geom.precision == _lib.PREC_BF16 else 30000.0, device=dev, dtype=torch.float64)
    lse_p[:, :, :, :S] = LSE
    Gc = (Gb.double() - lse_p.reshape(P, h, geom.Mp)).float().contiguous()
    dG, dT = run_bwd_q(geom, G, Gc, H, Hc, ws, pair)
    wdG, wdT, wda, wdb, wdy, wdx = grad_reference(G.float(), Gb, H.float(), Hc, a, b, ys, xs, T2, S, geom.Wt, N, LSE)
    dGg = dG.double().reshape(P, h, S, Sp, 32)[:, :, :, :S]
    dTg = dT.double()[:, geom.x_off:geom.x_off + geom.Wt, geom.y_off:geom.y_off + geom.Ht].transpose(1, 2)
    Tt = ops.pack_table(T.float(), geom).contiguous()
    da, db, dy, dx = [t.double()[..., :N] for t in run_bwd_k(geom, G, Gc, H, Hc, ws, Tt)]
    out.update(flagged=int(flags.sum()), dG=relerr(dGg[..., TAPS], wdG[..., TAPS]), dGb=relerr(dGg[..., 15], wdG[..., 15]),
               dtable=relerr(dTg, wdT), da=relerr(da, wda), db=relerr(db, wdb), dys=relerr(dy, wdy), dxs=relerr(dx, wdx),
               dead=Rn_got[..., 14].abs().max().item())
    print(f"{'':24s} dG {out['dG']:.2e} dGb {out['dGb']:.2e} dtable {out['dtable']:.2e}  da {out['da']:.2e} db {out['db']:.2e} "
          f"dys {out['dys']:.2e} dxs {out['dxs']:.2e}")
    return out


def reduction_case(P=2, h=4, S=24, N=500, D=3, seed=7):
    """With block 1 of G and H zero the two-group entry points are the one-group ones per (problem, group): for group g
    the one-group problem has the heads of g, the keys of the rows p * 2 + g (positions: plane 0 of the row) and those
    heads' tables.  Returns {name: (largest difference, largest entry)} for R[..., :16], mref, dG[..., :16], dtable,
    dkey_a, dkey_b, dkey_y (plane 0), and `finite`: R / dG slots 16..27 are finite.  Then, with both groups' positions
    equal and G block 1 = block 0: 'twin' = (largest |R[16..27] - R[0..11]|, largest entry)."""
    Wt = 2 * S * D - 1
    geom, a, b, ys, xs, G, Gb, T = make_case(P=P, h=h, S=S, N=N, Wt=Wt, seed=seed)
    hg = h // NG
    G0 = G.clone()
    G0[..., 16:] = 0
    H, Hc = draw_cotangent(geom, G.dtype)
    H[..., 16:] = 0
    R, mref, flags, ws, pair = run_fwd(geom, a, b, ys, xs, G0, Gb, T)
    lse = (mref + torch.log2(R[..., 15].clamp_min(1e-37)))
    valid = ((torch.arange(geom.Mp, device=dev) % geom.Sp) < S)
    Gc = torch.where(valid, Gb - lse, torch.full_like(lse, -1.0e30)).contiguous()
    dG, dT = run_bwd_q(geom, G0, Gc, H, Hc, ws, pair)
    Tt = ops.pack_table(T.float(), geom).contiguous()
    da, db, dy, dx = run_bwd_k(geom, G0, Gc, H, Hc, ws, Tt)
    out = {"finite": bool(torch.isfinite(R[..., 16:28]).all() and torch.isfinite(dG[..., 16:28]).all())}

    def put(name, got, want):
        d_, m_ = (got.double() - want.double()).abs().max().item(), want.double().abs().max().item()
        o = out.get(name, (0.0, 0.0))
        out[name] = (max(o[0], d_), max(o[1], m_))
    for g in range(NG):
        hs = slice(g * hg, (g + 1) * hg)
        g1 = ops.AttnGeom(n_prob=P, q_div=1, heads=hg, groups=1, S=S, N=N, Wt=Wt, precision=geom.precision)
        a1, b1, y1, x1 = a[g::NG].contiguous(), b[g::NG].contiguous(), ys[g::NG, 0].contiguous(), xs[g::NG, 0].contiguous()
        Gg, Gbg, Tg = G0[:, hs, :, :16].contiguous(), Gb[:, hs].contiguous(), T[hs].contiguous()
        R1, mref1, _, ws1, pair1 = tc.run_fwd(g1, a1, b1, y1, x1, Gg, Gbg, Tg)
        put("R", R[:, hs, :, :16], R1)
        put("mref", mref[:, hs], mref1)
        Hg, Hcg, Gcg = H[:, hs, :, :16].contiguous(), Hc[:, hs].contiguous(), Gc[:, hs].contiguous()
        dG1, dT1 = tc.run_bwd_q(g1, Gg, Gcg, Hg, Hcg, ws1, pair1)
        put("dG", dG[:, hs, :, :16] * valid[:, None], dG1 * valid[:, None])
        put("dtable", dT[hs], dT1)
        da1, db1, dy1, dx1 = tc.run_bwd_k(g1, Gg, Gcg, Hg, Hcg, ws1, ops.pack_table(Tg.float(), g1).contiguous())
        put("dkey_a", da[g::NG], da1)
        put("dkey_b", db[g::NG], db1)
        put("dkey_y", dy[g::NG, 0], dy1)
    # both groups at the same positions, the same G rows: group 1's weight sums equal group 0's
    ys2, xs2 = ys.clone(), xs.clone()
    ys2[:, 1], xs2[:, 1] = ys[:, 0], xs[:, 0]
    G2 = G.clone()
    G2[..., 16:28] = G[..., :12]
    R2, *_ = run_fwd(geom, a, b, ys2, xs2, G2, Gb, T)
    R2 = R2 * valid[None, None, :, None]
    out["twin"] = ((R2[..., 16:28] - R2[..., :12]).abs().max().item(), R2[..., :12].abs().max().item())
    return out


# the cases of tests/test_gpu_tap_groups.py (mirroring KERNEL_CASES of tests/test_gpu_tap.py)
CASES = {
    "sorted": dict(P=2, h=2, S=24, N=500, Wt=2 * 24 * 3 - 1),
    "two_heads_per_group": dict(P=2, h=4, S=24, N=500, Wt=2 * 24 * 3 - 1),
    "ragged": dict(P=3, h=2, S=20, N=333, Wt=2 * 20 * 5 - 1, seed=1),
    "unsorted_wide": dict(P=1, h=2, S=18, N=200, Wt=2 * 18 * 5 - 1, spread=(12.0, 30.0), sort=False, seed=2),
    "fp16": dict(P=1, h=2, S=24, N=400, Wt=2 * 24 * 3 - 1, seed=5, prec=_lib.PREC_F16, gscale=2.0, headroom=8.0),
    "two_blocks_per_wave": dict(P=1, h=2, S=120, N=313, Wt=2 * 120 * 2 - 1, spread=(12.0, 30.0), sort=False, seed=8),
    "four_blocks_per_wave": dict(P=1, h=2, S=232, N=313, Wt=2 * 232 * 2 - 1, spread=(12.0, 30.0), sort=False, seed=9),
}


def main():
    for name, kw in CASES.items():
        check_case(name, **dict(kw))
    print(reduction_case())


if __name__ == "__main__":
    main()
