"""Tap dropout kernels (csrc/attn_tap_*_drop.hip) against a float64 restatement of their definition with the host twin of
the keep mask (ops.dropout_keep_mask), and their timing against the plain tap kernels on the same keys.
    python tools/tap_drop_check.py check        small random cases, forward and both backward entry points
    B=2 python tools/tap_drop_check.py time     S=200, 65 984 keys per problem, B samples x 6 views x 2 heads
    python tools/tap_drop_check.py check x3     the same cases in the split-bf16 mode (csrc/attn_tap_*_x3_drop.hip,
    B=2 python tools/tap_drop_check.py time x3  bevr_attn_tap_*_x3_dropout), timed against the plain split-mode tap kernels

The definition (include/bevrender_hip.h, "Attention dropout on the tap entry points"), P = softmax over the segment:
    R[slot][q] / lsum[q] = sum_n keep[q][key0 + n] w_slot(n) P[n][q]            LSE = log2 sum_n 2^S[n][q]   (no mask)
    dS[n][q]             = P[n][q] (keep ? sum_t w_t(n) H[t][q] + H[15][q] : 0  +  Hc[q])
    dG[k][q]             = sum_n A[n][k] dS[n][q];  key side: dS through the logits, keep P H / ln2 through the values"""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bevrender_amd import ops, _lib  # noqa: E402
import tap_check as tc  # noqa: E402

dev = tc.dev
X3 = tc.X3


def _entry(geom, stem):
    """the dropout entry point of the case's operand mode: bevr_attn_tap_<stem>[_x3]_dropout"""
    return getattr(_lib.lib(), f"bevr_attn_tap_{stem}{'_x3' if geom.precision == X3 else ''}_dropout")


def header_split_drop(rows, c, hone, dead=0.0):
    """tap_check.header_split extended by slot 15 as include/bevrender_hip.h words it for bevr_attn_tap_*_x3_dropout: the
    kept mass's cotangent in BOTH planes, hi = bf16(x), lo = bf16(x - hi).  Returns (planes, the offset as the kernels add
    it, slot 15 as they contract it: hi + lo)."""
    pl, c_eff = tc.header_split(rows, c, dead)
    hone = hone.float()
    hi = hone.to(torch.bfloat16)
    pl[0][..., 15] = hi
    pl[1][..., 15] = (hone - hi.float()).to(torch.bfloat16)
    return pl, c_eff, pl[0][..., 15].float() + pl[1][..., 15].float()


def keep_mask(seed, thr, geom, key0):
    """(P, h, S(j), S(i), N) float64 0 / 1: the kernels' mask for the segment's keys, hashed at key index key0 + n."""
    P, h, S, N = geom.n_prob, geom.heads, geom.S, geom.N
    m = ops.dropout_keep_mask(seed, thr, P * h, S, key0 + N, device=dev)[..., key0:]          # (P h, i*S + j, N)
    return m.reshape(P, h, S, S, N).permute(0, 1, 3, 2, 4).double()


def run_fwd(geom, a, b, ys, xs, G, Gb, T, key0, thr, seed, headroom=64.0, timer=None):
    L = _lib.lib()
    d = geom.desc()
    Tt = ops.pack_table(T.float(), geom)
    pair = torch.stack((Tt[..., :-1], Tt[..., 1:]), dim=-1).contiguous()
    ws = torch.empty(L.bevr_attn_tap_ws_bytes(C.byref(d)), device=dev, dtype=torch.uint8)
    _lib.check(L.bevr_attn_tap_prep(C.byref(d), ops._ptr(a), ops._ptr(b), ops._ptr(ys), ops._ptr(xs), ops._ptr(ws),
                                    ops._stream()), "tap_prep")
    tmax = (T.float() * ops.LOG2E).amax((1, 2)).clamp_min(0)
    U = G[..., :12].float().amax(-1).clamp_min(0) * 1.01 + Gb + tmax[None, :, None] * 1.01 + 0.01
    if geom.precision == X3:
        G, c_eff = tc.header_split(G, Gb - (U - headroom), dead=-1.0e30)
        mref = (Gb - c_eff).contiguous()
    else:
        G = G.clone()
        mref = (Gb - tc.set_offset(G, Gb - (U - headroom))).contiguous()
    R = torch.empty(geom.n_prob, geom.heads, geom.Mp, 16, device=dev, dtype=torch.float32)
    lsum = torch.empty(geom.n_prob, geom.heads, geom.Mp, device=dev, dtype=torch.float32)
    flags = torch.zeros(geom.n_prob * geom.heads, geom.S, device=dev, dtype=torch.int32)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(_entry(geom, "fwd")(C.byref(d), ops._ptr(G), ops._ptr(ws), ops._ptr(pair), ops._ptr(mref), ops._ptr(R),
                                   ops._ptr(lsum), ops._ptr(flags), key0, thr, seed, ops._stream()), "tap_fwd_dropout")
    e1.record()
    torch.cuda.synchronize()
    if timer is not None:
        timer.append(e0.elapsed_time(e1))
    return R, lsum, mref, flags, ws, pair


def pack_h(H, Hc, Hone, x3=False):
    """the H operand: the 16-bit pack, or (x3) the split planes of float rows (header_split_drop)"""
    if x3:
        return header_split_drop(H, Hc, Hone)[0]
    H = H.clone()
    tc.set_offset(H, Hc)
    H[..., 15] = Hone.to(H.dtype)
    return H


def run_bwd_q(geom, G, Gc, H, ws, pair, key0, thr, seed, timer=None):
    L = _lib.lib()
    d = geom.desc()
    if geom.precision == X3:       # (H: the planes, pack_h)
        G = tc.header_split(G, Gc, dead=-1.0e30)[0]
    else:
        G = G.clone()
        tc.set_offset(G, Gc)
    dG = torch.empty(geom.n_prob, geom.heads, geom.Mp, 16, device=dev, dtype=torch.float32)
    dT = torch.zeros(geom.heads, geom.Wp, geom.Hp + 1, device=dev, dtype=torch.float32)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(_entry(geom, "bwd_q")(C.byref(d), ops._ptr(G), ops._ptr(H), ops._ptr(ws), ops._ptr(pair), ops._ptr(dG),
                                     ops._ptr(dT), key0, thr, seed, ops._stream()), "tap_bwd_q_dropout")
    e1.record()
    torch.cuda.synchronize()
    if timer is not None:
        timer.append(e0.elapsed_time(e1))
    return dG, dT


def run_bwd_k(geom, G, Gc, H, ws, Tt, key0, thr, seed, timer=None):
    L = _lib.lib()
    d = geom.desc()
    if geom.precision == X3:       # (H: the planes, pack_h)
        G = tc.header_split(G, Gc, dead=-1.0e30)[0]
    else:
        G = G.clone()
        tc.set_offset(G, Gc)
    outs = [torch.zeros(geom.n_prob, geom.Np, device=dev, dtype=torch.float32) for _ in range(4)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(_entry(geom, "bwd_k")(C.byref(d), ops._ptr(G), ops._ptr(H), ops._ptr(ws), ops._ptr(Tt),
                                     *[ops._ptr(t) for t in outs], key0, thr, seed, ops._stream()), "tap_bwd_k_dropout")
    e1.record()
    torch.cuda.synchronize()
    if timer is not None:
        timer.append(e0.elapsed_time(e1))
    return outs


def reference(G, Gb, a, b, ys, xs, T2, S, Wt, N, keep, mimic=None):
    """float64 definition of the forward: Rk (P, h, S(j), S(i), 16) = sum_n keep w P (P normalised over ALL keys), LSE.
    mimic: the tap weights, the table and the bias weights rounded as the operand mode holds them (tap_check.reference)."""
    P, h, Mp, _ = G.shape
    Sp = Mp // S
    Gd = G.double().reshape(P, h, S, Sp, 16)[:, :, :, :S]
    Gbd = Gb.double().reshape(P, h, S, Sp)[:, :, :, :S]
    w = tc.tap_w(ys[:, :N], xs[:, :N])
    if mimic is not None:
        w = tc._mim(w, mimic)
        T2 = tc._mim(T2, mimic)
    Rk = torch.zeros(P, h, S, S, 16, dtype=torch.float64, device=G.device)
    LSE = torch.zeros(P, h, S, S, dtype=torch.float64, device=G.device)
    for p in range(P):
        for j in range(S):
            bia = tc.bias_ref(T2, a[p, :N].double(), b[p, :N], S, Wt, j, mimic)
            lg = torch.einsum("hit,nt->hin", Gd[p, :, j, :, :12], w[p, :, :12]) + Gbd[p, :, j, :, None] + bia
            m = lg.amax(-1, keepdim=True)
            pr = torch.exp2(lg - m)
            l = pr.sum(-1, keepdim=True)
            LSE[p, :, j] = (m + torch.log2(l))[..., 0]
            Rk[p, :, j] = torch.einsum("hin,nt->hit", keep[p, :, j] * pr / l, w[p])
    return Rk, LSE


def grad_reference(G, Gb, H, Hc, Hone, a, b, ys, xs, T2, S, Wt, N, LSE, keep):
    """float64 gradients as tap_check.grad_reference, with dS = P (keep (w . H + Hone) + Hc) and the value path keep P."""
    P, h, Mp, _ = G.shape
    Sp = Mp // S
    cut = lambda t: t.double().reshape(P, h, S, Sp, *t.shape[3:])[:, :, :, :S]       # noqa: E731
    Gd, Hd, Gbd, Hcd, Hod = cut(G), cut(H), cut(Gb), cut(Hc), cut(Hone)
    leaves = [t[:, :N].double().clone().requires_grad_(True) for t in (a, b, ys, xs)]
    al, bl, yl, xl = leaves
    T2l = T2.clone().requires_grad_(True)
    dG = torch.zeros(P, h, S, S, 16, dtype=torch.float64, device=G.device)
    for p in range(P):
        w = tc.tap_w(yl[p], xl[p])
        for j in range(S):
            bia = tc.bias_ref(T2l, al[p], bl[p], S, Wt, j)
            lg = torch.einsum("hit,nt->hin", Gd[p, :, j, :, :12], w[:, :12]) + Gbd[p, :, j, :, None] + bia
            Pm = torch.exp2(lg - LSE[p, :, j, :, None]).detach()
            dpl = torch.einsum("hit,nt->hin", Hd[p, :, j, :, :12], w[:, :12])
            kp = keep[p, :, j]
            dS = (Pm * (kp * (dpl + Hod[p, :, j, :, None]) + Hcd[p, :, j, :, None])).detach()
            dG[p, :, j] = torch.einsum("hin,nk->hik", dS, w.detach())
            ((dS * lg).sum() + (kp * Pm * dpl).sum() * ops.LOG2E).backward(retain_graph=True)
    return dG, T2l.grad, al.grad, bl.grad, yl.grad, xl.grad


def check_case(name, key0=1234, p=0.3, drop_seed=0x5eed0001, **kw):
    """Returns the errors of tap_check.check_case's kind for the dropout entry points (forward: Rk = R / lsum against
    the definition, slots 12, 13 left out as there; LSE in log2 units; gradients relative to the largest reference value).
    prec=BEVR_PREC_BF16X3: the split-mode entry points on operands built by header_split / header_split_drop; besides the
    figures above `mass` (the kept mass, slot 15 of Rk, alone), `mimic` = (Rk, LSE, mass) against the restatement on the
    split operands themselves (tap_check.check_case), and `keys`: the per-key position gradients (got, want) for callers
    that judge them key by key.  h_cols: the BEV columns that carry the backward's cotangent (default: all)."""
    headroom = kw.pop("headroom", 64.0)
    h_cols = kw.pop("h_cols", None)
    thr = int(round(p * 65536))
    geom, a, b, ys, xs, G, Gb, T = tc.make_case(**kw)
    S, Sp, P, h, N = geom.S, geom.Sp, geom.n_prob, geom.heads, geom.N
    keep = keep_mask(drop_seed, thr, geom, key0)
    R, lsum, mref, flags, ws, pair = run_fwd(geom, a, b, ys, xs, G, Gb, T, key0, thr, drop_seed, headroom)
    Rg = R.double().reshape(P, h, S, Sp, 16)[:, :, :, :S]
    lg = lsum.double().reshape(P, h, S, Sp)[:, :, :, :S]
    mr = mref.double().reshape(P, h, S, Sp)[:, :, :, :S]
    T2 = T.double() * ops.LOG2E
    Rk, LSE = reference(G.float(), Gb, a, b, ys, xs, T2, S, geom.Wt, N, keep)
    sel = [t for t in range(16) if t not in (12, 13)]
    out = dict(flagged=int(flags.sum()), Rk=((Rg / lg[..., None])[..., sel] - Rk[..., sel]).abs().max().item(),
               LSE=(mr + torch.log2(lg) - LSE).abs().max().item(), dead=(Rg[..., 14] / lg).abs().max().item(),
               kept=keep.mean().item(), mass=(Rg[..., 15] / lg - Rk[..., 15]).abs().max().item())
    x3 = geom.precision == X3
    if x3:
        Rm, Lm = reference(tc._mim(G.double(), tc.MIMIC_X3).float(), Gb, a, b, ys, xs, T2, S, geom.Wt, N, keep, tc.MIMIC_X3)
        out["mimic"] = (((Rg / lg[..., None])[..., sel] - Rm[..., sel]).abs().max().item(),
                        (mr + torch.log2(lg) - Lm).abs().max().item(), (Rg[..., 15] / lg - Rm[..., 15]).abs().max().item())
    gen = torch.Generator(device=dev).manual_seed(99)
    ed = G.dtype
    valid = ((torch.arange(geom.Mp, device=dev) % Sp) < S)
    H = torch.zeros(P, h, geom.Mp, 16, device=dev)
    H[..., :12] = torch.randn(P, h, geom.Mp, 12, device=dev, generator=gen)
    H = (H * valid[None, None, :, None]).to(ed)
    if h_cols is not None:
        col = torch.zeros(S, dtype=torch.bool, device=dev)
        col[torch.tensor(list(h_cols), device=dev)] = True
        valid = valid & col.repeat_interleave(Sp)
        H = H * valid[None, None, :, None].to(ed)
    Hc = (torch.randn(P, h, geom.Mp, device=dev, generator=gen) * valid).contiguous()
    Hone = (torch.randn(P, h, geom.Mp, device=dev, generator=gen) * valid).to(ed)
    Hk = pack_h(H, Hc, Hone, x3)
    lse_p = torch.full((P, h, S, Sp), 1.0e30 if geom.precision in (_lib.PREC_BF16, X3) else 30000.0, device=dev, dtype=torch.float64)
    lse_p[:, :, :, :S] = LSE
    Gc = (Gb.double() - lse_p.reshape(P, h, geom.Mp)).float().contiguous()
    dG, dT = run_bwd_q(geom, G, Gc, Hk, ws, pair, key0, thr, drop_seed)
    # the constants the kernel sees: hi + lo of Hc (split mode: its four parts, and hi + lo of slot 15)
    if x3:
        _, Hc_seen, Hone_seen = header_split_drop(H, Hc, Hone)
    else:
        Hc_seen, Hone_seen = Hk[..., 12].float() + Hk[..., 13].float(), Hone.float()
    wdG, wdT, wda, wdb, wdy, wdx = grad_reference(G.float(), Gb, H.float(), Hc_seen, Hone_seen, a, b, ys, xs, T2, S, geom.Wt,
                                                  N, LSE, keep)
    dGg = dG.double().reshape(P, h, S, Sp, 16)[:, :, :, :S]
    dTg = dT.double()[:, geom.x_off:geom.x_off + geom.Wt, geom.y_off:geom.y_off + geom.Ht].transpose(1, 2)
    Tt = ops.pack_table(T.float(), geom).contiguous()
    da, db, dy, dx = [t.double()[:, :N] for t in run_bwd_k(geom, G, Gc, Hk, ws, Tt, key0, thr, drop_seed)]
    out.update(dG=tc.relerr(dGg[..., :12], wdG[..., :12]), dGb=tc.relerr(dGg[..., 15], wdG[..., 15]), dtable=tc.relerr(dTg, wdT),
               da=tc.relerr(da, wda), db=tc.relerr(db, wdb), dys=tc.relerr(dy, wdy), dxs=tc.relerr(dx, wdx))
    print(f"{name:24s} " + "  ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in out.items()))
    out["keys"] = dict(geom=geom, a=a[:, :N], b=b[:, :N], ys=ys[:, :N], xs=xs[:, :N],
                       da=(da, wda), db=(db, wdb), dys=(dy, wdy), dxs=(dx, wdx))
    return out


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "check"
    x3 = len(sys.argv) > 2 and sys.argv[2] == "x3"
    if mode == "check" and x3:
        check_case("sorted S=24 N=500 x3", P=2, h=2, S=24, N=500, Wt=2 * 24 * 3 - 1, prec=X3)
        check_case("ragged S=20 N=333 x3", P=3, h=2, S=20, N=333, Wt=2 * 20 * 5 - 1, seed=1, prec=X3)
        check_case("unsorted wide x3", P=1, h=2, S=18, N=200, Wt=2 * 18 * 5 - 1, spread=(12.0, 30.0), sort=False, seed=2, prec=X3)
        check_case("S=40 (3 blocks) N=1000 x3", P=1, h=1, S=40, N=1000, Wt=2 * 40 * 5 - 1, seed=3, prec=X3)
        return
    if mode == "check":
        check_case("sorted S=24 N=500", P=2, h=2, S=24, N=500, Wt=2 * 24 * 3 - 1)
        check_case("ragged S=20 N=333", P=3, h=2, S=20, N=333, Wt=2 * 20 * 5 - 1, seed=1)
        check_case("unsorted wide", P=1, h=2, S=18, N=200, Wt=2 * 18 * 5 - 1, spread=(12.0, 30.0), sort=False, seed=2)
        check_case("S=40 (3 blocks) N=1000", P=1, h=1, S=40, N=1000, Wt=2 * 40 * 5 - 1, seed=3)
        check_case("fp16", P=1, h=2, S=24, N=400, Wt=2 * 24 * 3 - 1, seed=5, prec=_lib.PREC_F16, gscale=2.0, headroom=8.0)
        return
    # ---- timing: plain and dropout entry points on the SAME keys, interleaved, medians (ms) ----
    B = int(os.environ.get("B", "2"))
    iters = int(os.environ.get("ITERS", "7"))
    S, h, D, V = 200, 2, 5, 6
    N = int(os.environ.get("N", "65984"))
    key0, thr, seed = 37000, int(round(0.1 * 65536)), 0x5eed
    geom, a, b, ys, xs, G, Gb, T = tc.make_case(P=B * V, h=h, S=S, N=N, Wt=2 * S * D - 1,
                                                prec=X3 if x3 else _lib.PREC_BF16)
    R, mref, flags, ws, pair = tc.run_fwd(geom, a, b, ys, xs, G, Gb, T)
    lse = (mref + torch.log2(R[..., 15].clamp_min(1e-37)))
    H = (torch.randn_like(G.float()) * (torch.arange(16, device=dev) < 12)).to(G.dtype)
    Hc = torch.randn_like(Gb)
    Hk = pack_h(H, Hc, torch.randn_like(Gb), x3)
    Gc = (Gb - lse).contiguous()
    Tt = ops.pack_table(T.float(), geom).contiguous()
    t = {k: [] for k in ("fwd", "fwd_drop", "bwd_q", "bwd_q_drop", "bwd_k", "bwd_k_drop")}
    for it in range(iters + 1):
        sink = [] if it == 0 else None          # the first round warms up
        tc.run_fwd(geom, a, b, ys, xs, G, Gb, T, timer=sink if it == 0 else t["fwd"])
        run_fwd(geom, a, b, ys, xs, G, Gb, T, key0, thr, seed, timer=sink if it == 0 else t["fwd_drop"])
        tc.run_bwd_q(geom, G, Gc, H, Hc, ws, pair, timer=sink if it == 0 else t["bwd_q"])
        run_bwd_q(geom, G, Gc, Hk, ws, pair, key0, thr, seed, timer=sink if it == 0 else t["bwd_q_drop"])
        tc.run_bwd_k(geom, G, Gc, H, Hc, ws, Tt, timer=sink if it == 0 else t["bwd_k"])
        run_bwd_k(geom, G, Gc, Hk, ws, Tt, key0, thr, seed, timer=sink if it == 0 else t["bwd_k_drop"])
    pairs = B * V * h * S * S * N
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    for k in ("fwd", "bwd_q", "bwd_k"):
        print(f"TAP{' x3' if x3 else ''} {k:6s} plain {med[k]:8.2f} ms ({pairs / med[k] / 1e9:5.2f} T pairs/s, min {min(t[k]):.2f} max {max(t[k]):.2f})   "
              f"dropout {med[k + '_drop']:8.2f} ms ({pairs / med[k + '_drop'] / 1e9:5.2f} T pairs/s, min {min(t[k + '_drop']):.2f} "
              f"max {max(t[k + '_drop']):.2f})   ratio {med[k + '_drop'] / med[k]:.2f}")


if __name__ == "__main__":
    main()
