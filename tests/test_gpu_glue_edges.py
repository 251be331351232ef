"""The glue kernels around the attention core (csrc/sample.hip, layernorm.hip, offset_head.hip, keypos.hip, warp.hip,
merge.hip, attn_bwd_prep.hip) where their small direct tests do not reach: past one sweep of every capped grid (A), against
float64 instead of the float32 stock chain (B), on what padding rows and empty key segments really hold (C), and under
cotangents far from 1 (D).  The reference is always the stock op of the kernel's existing test in float64 on the CPU.

Tolerances carry over UNCHANGED from the existing test of the same kernel (named in each docstring) wherever the
reduction length is the same.  Sums of far more terms into one float than any existing test has (parameter gradients
over 10^4 .. 10^6 rows, the feature gradient of pinned keys, the statistics of bwd_prep) have no derived limit: there
the stock PyTorch op runs in float32 on the device on the same input, its error against float64 is measured, and the
limit is 4 x that error (another, equally valid summation order; not a lost row), never below the carried-over
tolerance.  Both errors are printed per case at the end (profiles/glue_edges.txt is that table)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from bevrender_amd import _lib, ops
from oracle import bevrender_oracle as O
import test_gpu_grad_patterns_glue as glue
from test_gpu_grad_patterns_glue import ratio

pytestmark = pytest.mark.gpu
DEV = "cuda"
TABLE = []      # (case, quantity, kernel error / carried limit, stock float32 error / carried limit, limit / carried limit)


def teardown_module(module):
    print("\n[glue edges] errors against float64 as multiples of the carried-over tolerance")
    print(f"{'case':58s} {'quantity':10s} {'kernel':>9s} {'stock f32':>9s} {'limit':>9s}")
    for case, name, r, rs, lim in TABLE:
        print(f"{case:58s} {name:10s} {r:9.3f} {'-' if rs is None else format(rs, '9.3f'):>9s} {lim:9.3f}")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def check(case, name, tol, got, want, stock=None):
    """got against want (float64) under `tol` (the forms of test_gpu_grad_patterns_glue.ratio); with `stock` (the stock
    op's float32 result on the device) the limit is max(tol, 4 x the stock op's error under the same measure)."""
    r = ratio(tol, got, want)
    rs = None if stock is None else ratio(tol, stock, want)
    lim = 1.0 if stock is None else max(1.0, 4.0 * rs)
    TABLE.append((case, name, r, rs, lim))
    assert r < lim, f"{case}: {name} at {r:.2f} x its tolerance {tol} (limit {lim:.2f} x; the stock op in float32: {rs})"


def run_pair(fn, ins, cot):
    """fn on float64 CPU leaves and on float32 device leaves: (out, grads by name) for each"""
    res = []
    for dev in (False, True):
        leaves = {}
        for n, t in ins.items():
            t = t.clone().to(DEV) if dev else t.clone().double()
            leaves[n] = t.requires_grad_(True)
        out = fn(leaves, dev)
        gs = torch.autograd.grad(out, list(leaves.values()), cot.float().to(DEV) if dev else cot.double())
        res.append((out.detach(), dict(zip(leaves, gs))))
    return res


# =====================================================================================================================
# A. the second sweep of every capped grid
# =====================================================================================================================
@pytest.mark.parametrize("rows,Cc", [(8209, 256), (32808, 64), (524300, 4)])
def test_layer_norm_past_one_sweep(rows, Cc):
    """layernorm_fwd / _bwd with a second, mostly dead iteration at each lane-group width.  Tolerances of
    test_layer_norm_matches_torch (out 2e-5 / 2e-5, dx 2e-5 of max); d(gamma), d(beta) sum 8 000 .. 524 000 rows:
    measured against F.layer_norm in float32."""
    per = 256 // (Cc // 4)
    assert 2048 * per < rows < 2 * 2048 * per       # csrc/layernorm.hip grid_of: 256 * 8 workgroups of LN_THREADS / (C / 4) rows
    assert (rows - 2048 * per) % per                 # the last workgroup of the second sweep is ragged
    gen = _gen(rows + Cc)
    ins = dict(x=torch.randn(rows, Cc, generator=gen) * 2.0 + 0.5, gamma=torch.randn(Cc, generator=gen), beta=torch.randn(Cc, generator=gen))
    cot = torch.randn(rows, Cc, generator=gen)
    (want, gw), (stock, gs) = run_pair(lambda d, dev: F.layer_norm(d["x"], (Cc,), d["gamma"], d["beta"], 1e-5), ins, cot)
    dev = {n: t.clone().to(DEV).requires_grad_(True) for n, t in ins.items()}
    got = ops.layer_norm(dev["x"], dev["gamma"], dev["beta"], 1e-5)
    gg = dict(zip(dev, torch.autograd.grad(got, list(dev.values()), cot.to(DEV))))
    case = f"layer_norm({rows}, {Cc})"
    check(case, "out", ("allclose", 2e-5, 2e-5), got, want)
    check(case, "dx", ("rel", 2e-5), gg["x"], gw["x"])
    check(case, "dgamma", ("rel", 2e-5), gg["gamma"], gw["gamma"], gs["gamma"])
    check(case, "dbeta", ("rel", 2e-5), gg["beta"], gw["beta"], gs["beta"])


def _grid_sample(feat, pos):
    B, Cc = feat.shape[:2]
    N = pos.shape[1]
    return F.grid_sample(feat, pos[:, None, :, (1, 0)], mode="bilinear", padding_mode="zeros",
                         align_corners=True).reshape(B, Cc, N).permute(0, 2, 1)


def _smooth_keys(pos, Hi, Wi, placed):
    """keys whose d(pos) is compared: not placed on a pixel centre deliberately (`placed`), and not within 1e-4 of one by
    chance -- d(pos) is discontinuous there (test_gpu_random_sweep_aux.test_sample_features_random); the chance ones
    must stay below 0.1 % of the keys."""
    px, py = (pos[..., 1].double() + 1) * (Wi - 1) / 2, (pos[..., 0].double() + 1) * (Hi - 1) / 2
    smooth = ((px - px.round()).abs() > 1e-4) & ((py - py.round()).abs() > 1e-4)
    by_chance = (~smooth & ~placed).sum().item()
    assert by_chance < 1e-3 * pos.shape[0] * pos.shape[1], by_chance
    return smooth & ~placed


def test_sample_forward_and_scatter_backward_past_one_sweep():
    """sample_fwd_kernel and sample_bwd_kernel<false> (C too wide for the LDS patch) with a second, partial sweep.
    Tolerances of test_sample_backward_with_most_keys_pinned_to_the_corner, the sampler's existing test against float64
    (out 1e-5 / 5e-5, d(feat) 2e-5 of max, d(pos) 1e-4 / 1e-4 of max; test_sample_features_matches_grid_sample compares
    with float32 grid_sample, which rounds the pixel coordinate as the kernel does); d(feat) sums ~ 900 taps per pixel
    and is measured against F.grid_sample in float32."""
    B, Cc, Hi, Wi, N = 2, 256, 5, 7, 8200
    assert 4096 * 256 < B * N * (Cc // 4) < 2 * 4096 * 256                  # csrc/sample.hip grid_for
    assert Cc * 8 * 32 > 48 * 1024                                           # sample_bwd: patch_ok is false (PCH_WMAX, PCH_BYTES)
    assert 256 * -(-4096 // B) < N * (Cc // 4) < 2 * 256 * -(-4096 // B)     # sample_bwd: gx capped at ceil(256 * 16 / nb)
    gen = _gen(8200)
    feat = torch.randn(B, Cc, Hi, Wi, generator=gen)
    pos = (torch.rand(B, N, 2, generator=gen) * 2 - 1) * 1.2
    placed = torch.zeros(B, N, dtype=torch.bool)
    # the projector's pin and the exact corners, in the first sweep and in the keys only the second sweep reaches
    spots = torch.tensor([[-1., -1.], [1., 1.], [-1., 1.], [0., 0.], [1.5, 0.], [0., -1.5], [3., 3.], [1., -1.]])
    for b, n0 in ((0, 0), (1, N - 8), (1, N - 200)):
        pos[b, n0:n0 + 8] = spots
        placed[b, n0:n0 + 8] = True
    cot = torch.randn(B, N, Cc, generator=gen)
    (want, gw), (stock, gs) = run_pair(lambda d, dev: _grid_sample(d["feat"], d["pos"]), dict(feat=feat, pos=pos), cot)
    fg, pg = feat.clone().to(DEV).requires_grad_(True), pos.clone().to(DEV).requires_grad_(True)
    got = ops.sample_features(fg, pg, 1)
    dfeat, dpos = torch.autograd.grad(got, (fg, pg), cot.to(DEV))
    case = "sample scatter (2, 256, 5, 7) N=8200"
    check(case, "out", ("allclose", 1e-5, 5e-5), got, want)
    check(case, "dfeat", ("rel", 2e-5), dfeat, gw["feat"], gs["feat"])
    keep = _smooth_keys(pos, Hi, Wi, placed)
    check(case, "dpos", ("allclose", 1e-4, 1e-4 * gw["pos"].abs().max().item()), dpos.cpu()[keep], gw["pos"][keep])
    assert torch.isfinite(dpos).all()


@pytest.mark.parametrize("bf16,Wi", [(False, 9), (True, 9), (False, 40)])
def test_sample_patch_backward_with_several_chunks_per_workgroup(bf16, Wi):
    """sample_bwd_patch_kernel with 5 chunks on 3 workgroups per image: a workgroup flushes one LDS window, then builds
    the next behind the same barriers, and its hot-corner registers carry over the chunks (every other key pinned at
    (-1, -1) exactly; the rest anywhere up to +-1.3).  Wi = 40: the chunk's taps span more than the window's PCH_WMAX =
    32 columns, so those beyond it take the direct scatter between the same barriers.  Tolerances of test_sample_backward_with_most_keys_pinned_to_the_corner
    (out 1e-5 / 5e-5, d(feat) 2e-5 of max, d(pos) 1e-4 / 1e-4 of max); d(feat) is measured against F.grid_sample in
    float32; the bf16 map's gradient is stored in bf16: 2^-7 of max (test_sample_features_reads_bf16_features_as_they_are)."""
    B, Cc, Hi, N = 1024, 8, 6, 1100
    n_chunk, want_gx = -(-N // 256), -(-256 * 12 // B)
    assert 256 % (Cc // 4) == 0 and Cc * 8 * 32 <= 48 * 1024         # csrc/sample.hip sample_bwd: patch_ok
    assert n_chunk == 5 and want_gx == 3 and n_chunk > want_gx          # sample_bwd: gx = min(n_chunk, ceil(256 * 12 / nb))
    gen = _gen(1100)
    feat = torch.randn(B, Cc, Hi, Wi, generator=gen)
    if bf16:
        feat = feat.to(torch.bfloat16)
    pos = (torch.rand(B, N, 2, generator=gen) * 2 - 1) * 1.3
    placed = torch.zeros(B, N, dtype=torch.bool)
    pos[:, 0::2] = -1.0
    placed[:, 0::2] = True
    cot = torch.randn(B, N, Cc, generator=gen)
    (want, gw), (stock, gs) = run_pair(lambda d, dev: _grid_sample(d["feat"], d["pos"]), dict(feat=feat.float(), pos=pos), cot)
    fg, pg = feat.clone().to(DEV).requires_grad_(True), pos.clone().to(DEV).requires_grad_(True)
    got = ops.sample_features(fg, pg, 1)
    dfeat, dpos = torch.autograd.grad(got, (fg, pg), cot.to(DEV))
    case = f"sample patch (1024, 8, 6, {Wi}) N=1100{' bf16' if bf16 else ''}"
    check(case, "out", ("allclose", 1e-5, 5e-5), got, want)
    if bf16:
        assert dfeat.dtype == torch.bfloat16
        check(case, "dfeat", ("rel", 2.0 ** -7), dfeat, gw["feat"])
    else:
        check(case, "dfeat", ("rel", 2e-5), dfeat, gw["feat"], gs["feat"])
    keep = _smooth_keys(pos, Hi, Wi, placed)
    scale = gw["pos"].abs().max().item()
    check(case, "dpos", ("allclose", 1e-4, 1e-4 * scale), dpos.cpu()[keep], gw["pos"][keep])
    assert torch.isfinite(dpos).all()


def _offset_head_ref(d, B, H, W, g, cg, mx, K):
    xg = d["x"].reshape(B, H, W, g, cg).permute(0, 3, 1, 2, 4).reshape(B * g, H, W, cg)
    z = xg if "w0" not in d else (xg.unsqueeze(-1) * d["w0"].view(cg, mx) + d["b0"].view(cg, mx)).flatten(-2)
    return F.gelu(F.layer_norm(z, (K,), d["gamma"], d["beta"], 1e-5)) @ d["W3"].t()


@pytest.mark.parametrize("cfg", [(1, 257, 256, 16, 1, 1, 2), (1, 257, 256, 8, 1, 5, 5)])
def test_offset_head_past_the_grid_cap(cfg):
    """offset_head_fwd / _bwd with the grid capped (TSA form and SCA form with Mx = Dout = 5): every wave walks 17 pixels,
    the last step ragged.  Tolerances of test_fused_offset_head_matches_the_stock_op_chain (out 2e-5 / 2e-5, d(x) 2e-5
    of max); the parameter gradients sum 65 792 pixels: measured against the stock chain in float32."""
    B, H, W, Cc, g, mx, dout = cfg
    P = B * H * W
    assert -(-P // (4 * 16)) > 256 * 4 and P % (256 * 4 * 4)          # csrc/offset_head.hip oh_grid: OH_THREADS / 64 = 4 waves x 16 pixels
    cg = Cc // g
    K = cg * mx
    gen = _gen(sum(cfg))
    ins = dict(x=torch.randn(B, H, W, Cc, generator=gen))
    if mx > 1 or dout == mx:
        ins["w0"], ins["b0"] = torch.randn(K, generator=gen) * 0.7, torch.randn(K, generator=gen) * 0.3
    ins["gamma"], ins["beta"] = 1 + 0.2 * torch.randn(K, generator=gen), 0.1 * torch.randn(K, generator=gen)
    ins["W3"] = torch.randn(dout, K, generator=gen) / K ** 0.5
    cot = torch.randn(B * g, H, W, dout, generator=gen)
    (want, gw), (stock, gs) = run_pair(lambda d, dev: _offset_head_ref(d, B, H, W, g, cg, mx, K), ins, cot)
    dev = {n: t.clone().to(DEV).requires_grad_(True) for n, t in ins.items()}
    got = ops.offset_head(dev["x"], dev.get("w0"), dev.get("b0"), dev["gamma"], dev["beta"], dev["W3"], groups=g)
    gg = dict(zip(dev, torch.autograd.grad(got, list(dev.values()), cot.to(DEV))))
    case = f"offset_head{cfg}"
    check(case, "out", ("allclose", 2e-5, 2e-5), got, want)
    check(case, "dx", ("rel", 2e-5), gg["x"], gw["x"])
    for n in ins:
        if n != "x":
            check(case, "d" + n, ("rel", 2e-5), gg[n], gw[n], gs[n])


def _chain(O_r, L_r, O_c, L_c, S, c, views):        # tests/test_gpu_merge.py
    if O_c is not None:
        L_t = torch.logaddexp2(L_r, L_c)
        O_r = torch.exp2(L_r - L_t)[..., None] * O_r + torch.exp2(L_c - L_t)[..., None] * O_c
    return ops.unpack_out_views(O_r, S, c, views)


def _merge_views_inputs(B, V, h, S, c, two, gen):
    Sp = 32 * ((S + 31) // 32)
    Mp = S * Sp
    ins = dict(O_r=torch.randn(B * V, h, Mp, 32, generator=gen))
    if two:
        ins.update(L_r=torch.randn(B * V, h, Mp, generator=gen) * 6.0, O_c=torch.randn(B * V, h, Mp, 32, generator=gen),
                   L_c=torch.randn(B * V, h, Mp, generator=gen) * 6.0)
    return ins, Sp


def _check_merge_views(case, ins, B, V, h, S, c, Sp, gen, pad_exact=True):
    """forward and every gradient of ops.merge_views against the float64 chain at test_merge_views_matches_the_stock_chain's
    limits (out 2e-6, dO 2e-6, dL 2e-5 of max); the padding of the dO's is exactly zero"""
    two = "O_c" in ins
    cot = torch.randn(B, S * S, V * h * c, generator=gen)
    cpu = {n: t.clone().double().requires_grad_(True) for n, t in ins.items()}
    want = _chain(cpu["O_r"], cpu.get("L_r"), cpu.get("O_c"), cpu.get("L_c"), S, c, V)
    gw = dict(zip(cpu, torch.autograd.grad(want, list(cpu.values()), cot.double())))
    dev = {n: t.clone().to(DEV).requires_grad_(True) for n, t in ins.items()}
    got = ops.merge_views(dev["O_r"], S, c, V, *((dev["L_r"], dev["O_c"], dev["L_c"]) if two else ()))
    gg = dict(zip(dev, torch.autograd.grad(got, list(dev.values()), cot.to(DEV))))
    check(case, "out", ("rel", 2e-6), got, want)
    for n in ins:
        check(case, "d" + n, ("rel", 2e-5 if n.startswith("L") else 2e-6), gg[n], gw[n])
        if n.startswith("O") and pad_exact:
            pad = gg[n].reshape(B * V, h, S, Sp, 32)
            assert Sp == S or not pad[:, :, :, S:, :].ne(0).any()
            assert c == 32 or not pad[..., c:].ne(0).any()
    return want.detach(), gw, got.detach(), gg


@pytest.mark.parametrize("c,two", [(32, True), (16, False)])
def test_merge_views_past_one_sweep(c, two):
    """merge_views_fwd / _bwd with a second, partial sweep; Sp = 96 against S = 75, so padding rows fall in both sweeps.
    The reduction (32 channels of a row) is the existing test's: its limits carry over (see _check_merge_views)."""
    B, V, h, S = 2, 3, 4, 75
    ins, Sp = _merge_views_inputs(B, V, h, S, c, two, _gen(S * 7 + c))
    rows = B * V * h * S * Sp
    assert 4096 * 256 // 8 < rows < 2 * 4096 * 256 // 8 and Sp == 96       # csrc/merge.hip merge_grid: 256 * 16 workgroups, 8 threads a row
    _check_merge_views(f"merge_views({B}, {V}, {h}, {S}, {c}) two={two}", ins, B, V, h, S, c, Sp, _gen(1))


def _bwd_prep(dO, Ov, scale, dLSE, LSE0, prec):
    """bevr_attn_bwd_prep through the C ABI, as test_attn_bwd_prep_matches_the_stock_chain calls it"""
    ed = torch.bfloat16 if prec == _lib.PREC_BF16 else torch.float16
    n_prob, h, Mp, _ = dO.shape
    dOe = torch.empty(n_prob, h, Mp, 32, device=DEV, dtype=ed)
    dOt = torch.empty(n_prob, h, 32, Mp, device=DEV, dtype=ed)
    delta = torch.empty(n_prob, h, Mp, device=DEV)
    stats = torch.zeros(2, device=DEV)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = _lib.lib().bevr_attn_bwd_prep(p(dO), p(Ov), p(scale), p(dLSE), p(LSE0) if dLSE is not None else None, p(dOe), p(dOt),
                                       p(delta), p(stats), n_prob * h, Mp, prec, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return dOe, dOt, delta, stats


def _check_bwd_prep(case, n_prob, h, Mp, prec_name, with_lse, inf_rows):
    """dOe, dOt bit-equal to the cast and ops._perm_t; delta against float64 at test_attn_bwd_prep_matches_the_stock_chain's
    2e-6 of max; the two maxima at its 1e-5, or 4 x what its float32 chain on the device misses float64 by"""
    prec = _lib.PREC_BF16 if prec_name == "bf16" else _lib.PREC_F16
    ed = torch.bfloat16 if prec_name == "bf16" else torch.float16
    gen = _gen(11)
    dO = torch.randn(n_prob, h, Mp, 32, generator=gen) * 3.0
    Ov = torch.randn(n_prob, h, Mp, 32, generator=gen)
    sc = 4.0 if prec_name == "f16" else 1.0
    dLSE = torch.randn(n_prob, h, Mp, generator=gen) if with_lse else None
    LSE0 = torch.randn(n_prob, h, Mp, generator=gen)
    LSE0.view(-1)[inf_rows] = float("-inf")                           # a row without finite LSE takes no dLSE
    dOe_w = (dO * sc).to(ed)
    dOt_w = ops._perm_t(dOe_w)
    delta_w = (dOe_w.double() * Ov.double()).sum(-1)
    if with_lse:
        delta_w = delta_w - torch.where(torch.isfinite(LSE0), dLSE, torch.zeros_like(dLSE)).double() * ops.LOG2E * sc
    want_stats = torch.stack((dOe_w.double().pow(2).sum(-1).max(), delta_w.abs().max()))
    g = lambda t: None if t is None else t.to(DEV)
    dOg, Og, dLg, L0g = g(dO), g(Ov), g(dLSE), g(LSE0)
    dOe, dOt, delta, stats = _bwd_prep(dOg, Og, torch.tensor(sc, device=DEV) if sc != 1.0 else None, dLg, L0g, prec)
    assert torch.equal(dOe.cpu(), dOe_w) and torch.equal(dOt.cpu(), dOt_w)
    check(case, "delta", ("rel", 2e-6), delta, delta_w)
    # the stock chain of ops._AttnCore.backward in float32 on the device
    dOr = (dOg * sc).to(ed).float()
    d32 = (dOr * Og).sum(-1)
    if with_lse:
        d32 = d32 - torch.where(torch.isfinite(L0g), dLg, torch.zeros_like(dLg)) * ops.LOG2E * sc
    stock = torch.stack((dOr.pow(2).sum(-1).max(), d32.abs().max()))
    for i, n in enumerate(("stats[0]", "stats[1]")):
        check(case, n, ("allclose", 1e-5, 0.0), stats[i:i + 1], want_stats[i:i + 1], stock[i:i + 1])


@pytest.mark.parametrize("prec_name", ["bf16", "f16"])
def test_attn_bwd_prep_past_one_sweep(prec_name):
    """bevr_attn_bwd_prep with 8 320 row blocks on 8 192 waves: 128 waves take a second block and reuse their LDS tile;
    rows with LSE0 = -inf among those blocks."""
    n_prob, h, Mp = 130, 2, 1024
    n_blk = n_prob * h * (Mp // 32)
    assert 256 * 8 * 4 < n_blk < 2 * 256 * 8 * 4                      # csrc/attn_bwd_prep.hip: 256 * 8 workgroups of BP_WAVES = 4
    inf_rows = torch.tensor([8192 * 32 + r for r in (0, 5, 31, 32 * 7 + 9, 32 * 100 + 17, 32 * 127 + 31)] + [7])
    assert (inf_rows[:-1] // 32 >= 256 * 8 * 4).all() and inf_rows.max() < n_blk * 32
    _check_bwd_prep(f"attn_bwd_prep(260, 1024) {prec_name}", n_prob, h, Mp, prec_name, True, inf_rows)


def _key_positions_ref(off, ref_pts, order, B, V, g, sca_SD, use_tanh, sy, sx):
    """tests/test_gpu_ops.py test_key_positions_sca_ / _tsa_equals_the_stock_op_chain; also returns the unclamped position"""
    N = ref_pts.shape[1]
    scale = torch.tensor([sy, sx], dtype=torch.float64)
    outs = []
    for v in range(V):
        if sca_SD:
            S, D = sca_SD
            o = off[v].reshape(B * g, S // 2, 2, S, D).permute(0, 1, 3, 4, 2).reshape(B, g, N, 2)
        else:
            o = off[v].reshape(B, g, N, 2)
        outs.append((o.tanh() * scale if use_tanh else o) + ref_pts[v].double()[None, None])
    raw = torch.stack(outs, 1)
    p = raw if use_tanh else raw.clamp(-1.0, 1.0)
    if order is not None:
        p = p.gather(3, order[None, :, None, :, None].expand(B, V, g, N, 2))
    return p, raw


@pytest.mark.parametrize("use_tanh", [True, False])
@pytest.mark.parametrize("with_order", [True, False])
@pytest.mark.parametrize("form", ["sca", "tsa"])
def test_key_positions_past_one_sweep(form, with_order, use_tanh):
    """keypos_fwd / _bwd with a second, partial sweep.  Tolerances of test_key_positions_sca_ / _tsa_equals_the_stock_op_chain
    (out 1e-5 / 2e-6, d(off) 1e-4 / 1e-6).  The clamp's derivative jumps at |off + ref| = 1: elements within 1e-6 of it
    (float32 may round them to the other side) are left out, and there must be next to none."""
    if form == "sca":
        V, B, g, S, D = 6, 18, 2, 64, 5
        N = (S // 2) * S * D
        sca_SD, sy, sx = (S, D), 0.7 / (S // 2 - 1.0), 1.3 / (S * D - 1.0)
        gen = _gen(S * D + V)
        off = torch.randn(V, B * g, S, S, D, generator=gen) * 1.5
        ref_pts = torch.rand(V, N, 2, generator=gen) * 2.2 - 1.1
    else:
        V, B, g, Hk, Wk = 1, 47, 2, 150, 150
        N = Hk * Wk
        sca_SD, sy, sx = None, 2.0 / (Hk - 1.0), 2.0 / (Wk - 1.0)
        gen = _gen(5)
        off = torch.randn(V, B * g, N, 2, generator=gen) * (1.0 if use_tanh else 0.3)
        ref_pts = O.normalized_grid(Hk, Wk, torch.float32).reshape(1, N, 2)
    total = V * B * g * N
    assert 8192 * 256 < total < 2 * 8192 * 256                           # csrc/keypos.hip grid_of: 8192 workgroups of 256
    order = torch.stack([torch.randperm(N, generator=gen) for _ in range(V)]) if with_order else None
    cot = torch.randn(B, V, g, N, 2, generator=gen)
    o64 = off.double().requires_grad_(True)
    want, raw = _key_positions_ref(o64, ref_pts, order, B, V, g, sca_SD, use_tanh, sy, sx)
    (dwant,) = torch.autograd.grad(want, o64, cot.double(), retain_graph=True)
    og = off.to(DEV).requires_grad_(True)
    got = ops.key_positions(og, ref_pts.to(DEV), None if order is None else order.to(DEV), B, g, sca_SD=sca_SD, use_tanh=use_tanh,
                            sy=sy, sx=sx)
    (dgot,) = torch.autograd.grad(got, og, cot.to(DEV))
    case = f"key_positions({form}, order={with_order}, tanh={use_tanh})"
    check(case, "out", ("allclose", 1e-5, 2e-6), got, want.detach())
    dgot = dgot.cpu()
    if not use_tanh:
        # raw (B, V, g, N, 2) in the key grid's own order -> the layout of off
        edge = ((raw.detach().abs() - 1.0).abs() < 1e-6)
        (at_edge,) = torch.autograd.grad(raw, o64, edge.double())
        keep = at_edge == 0
        assert (~keep).sum().item() <= 1e-5 * keep.numel(), (~keep).sum().item()
        dgot, dwant = dgot[keep], dwant[keep]
    check(case, "doff", ("allclose", 1e-4, 1e-6), dgot, dwant)


def test_affine_warp_past_one_sweep():
    """affine_warp_kernel, forward and d(img), with a second sweep that is the whole last image -- partly inside, partly
    wholly outside the source (the mask == 0 early exit).  Angles up to 170 degrees and translations up to 2 S as in
    test_history_warp_random, whose limit (1e-4 of max) carries over to both directions: four taps a pixel, as there."""
    B, Cc, S = 33, 1, 256
    assert 8192 * 256 < B * S * S < 2 * 8192 * 256                       # csrc/warp.hip: min(.., 256 * 32) workgroups of 256
    assert (B - 1) * S * S == 8192 * 256                                 # image B - 1 IS the second sweep
    gen = _gen(33)
    img = torch.randn(B, Cc, S, S, generator=gen)
    ang = (torch.rand(B, generator=gen) - 0.5) * 170.0
    tr = (torch.rand(B, 2, generator=gen) - 0.5) * 2.0 * S
    ang[B - 1], tr[B - 1] = 40.0, torch.tensor([0.3 * S, -0.3 * S])
    ang[0], tr[0] = 0.0, torch.tensor([2.0 * S, 0.0])                    # wholly outside
    cot = torch.randn(B, Cc, S, S, generator=gen)
    i64 = img.double().requires_grad_(True)
    want = torch.stack([O.tv_affine(i64[i], float(ang[i]), (float(tr[i, 0]), float(tr[i, 1])), 0.0) for i in range(B)], 0)
    (dwant,) = torch.autograd.grad(want, i64, cot.double())
    with torch.no_grad():
        ones = O.tv_affine(torch.ones(1, S, S, dtype=torch.float64), float(ang[B - 1]), (float(tr[B - 1, 0]), float(tr[B - 1, 1])), 0.0)
    assert 0.2 < (ones == 0).double().mean().item() < 0.8                # the second sweep takes both branches
    assert not want[0].ne(0).any()
    ig = img.to(DEV).requires_grad_(True)
    got = ops.affine_warp(ig, torch.deg2rad(ang).to(DEV), tr.to(DEV))
    (dgot,) = torch.autograd.grad(got, ig, cot.to(DEV))
    check("affine_warp(33, 1, 256, 256)", "out", ("rel", 1e-4), got, want.detach())
    check("affine_warp(33, 1, 256, 256)", "dimg", ("rel", 1e-4), dgot, dwant)


# =====================================================================================================================
# B. float64 references for the kernels tests/test_gpu_merge.py checks against float32
# =====================================================================================================================
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("B,V,h,S,c", [(2, 3, 2, 21, 32), (1, 1, 4, 40, 16), (3, 2, 1, 33, 8), (1, 6, 2, 64, 32)])
def test_merge_views_against_float64(B, V, h, S, c, two):
    """test_merge_views_matches_the_stock_chain's shapes and limits, the chain in float64 on the CPU"""
    ins, Sp = _merge_views_inputs(B, V, h, S, c, two, _gen(S * 7 + c))
    _check_merge_views(f"merge_views({B}, {V}, {h}, {S}, {c}) two={two}", ins, B, V, h, S, c, Sp, _gen(2))


def _merge_tap_inputs(B, V, h, S, c, gen):
    Sp = 32 * ((S + 31) // 32)
    Mp = S * Sp
    ins = dict(O_r=torch.randn(B * V, h, Mp, 32, generator=gen), L_r=torch.randn(B * V, h, Mp, generator=gen) * 5.0,
               Rn=torch.randn(B * V, h, Mp, 12, generator=gen), L_c=torch.randn(B * V, h, Mp, generator=gen) * 5.0,
               Vp=torch.randn(B * V, h, 12, 32, generator=gen), bv=torch.randn(h, 32, generator=gen))
    ins["Vp"][..., c:] = 0.0                 # padded head channels are zero (ops.attention_core pads them)
    ins["bv"][..., c:] = 0.0
    return ins, Sp


def _merge_tap_fn(S, c, V):
    def fn(d, dev):
        return _chain(d["O_r"], d["L_r"], torch.matmul(d["Rn"], d["Vp"]) + d["bv"][None, :, None, :], d["L_c"], S, c, V)
    return fn


def _check_merge_tap(case, ins, B, V, h, S, c, gen):
    """forward and the six gradients of ops.merge_tap against the float64 chain at test_merge_tap_matches_the_stock_chain's
    limits (out 3e-6, gradients 3e-5 of max, dVp / dbv on the head's real channels); dVp and dbv sum every row of a
    (problem, head) / of all problems: measured against the chain in float32 on the device"""
    cot = torch.randn(B, S * S, V * h * c, generator=gen)
    (want, gw), (stock, gs) = run_pair(_merge_tap_fn(S, c, V), ins, cot)
    dev = {n: t.clone().to(DEV).requires_grad_(True) for n, t in ins.items()}
    got = ops.merge_tap(dev["O_r"], dev["L_r"], dev["Rn"], dev["L_c"], dev["Vp"], dev["bv"], S, c, V)
    gg = dict(zip(dev, torch.autograd.grad(got, list(dev.values()), cot.to(DEV))))
    check(case, "out", ("rel", 3e-6), got, want)
    for n in ins:
        if n in ("Vp", "bv"):
            check(case, "d" + n, ("rel", 3e-5), gg[n][..., :c], gw[n][..., :c], gs[n][..., :c])
        else:
            check(case, "d" + n, ("rel", 3e-5), gg[n], gw[n])
    return got.detach(), gg


@pytest.mark.parametrize("B,V,h,S,c", [(2, 3, 2, 21, 32), (1, 2, 4, 40, 16), (1, 6, 2, 64, 32)])
def test_merge_tap_against_float64(B, V, h, S, c):
    """test_merge_tap_matches_the_stock_chain's shapes and limits, the chain in float64 on the CPU"""
    ins, _ = _merge_tap_inputs(B, V, h, S, c, _gen(S + c))
    _check_merge_tap(f"merge_tap({B}, {V}, {h}, {S}, {c})", ins, B, V, h, S, c, _gen(3))


@pytest.mark.parametrize("shape", [(2, 9, 7, 8), (1, 40, 40, 64), (2, 10, 13, 256), (1, 203, 200, 12)])
def test_dwconv_res_gelu_against_float64(shape):
    """test_dwconv_res_gelu_matches_the_stock_chain's shapes and limits (out 2e-6, gradients 2e-5 of max), the chain in
    float64 on the CPU; dw and db sum every pixel: measured against the chain in float32 on the device"""
    B, H, W, Cc = shape
    gen = _gen(H * 3 + Cc)
    ins = dict(x=torch.randn(B, H, W, Cc, generator=gen), w=torch.randn(Cc, 1, 3, 3, generator=gen) * 0.3, b=torch.randn(Cc, generator=gen))
    cot = torch.randn(B, H, W, Cc, generator=gen)

    def fn(d, dev):
        xn = d["x"].permute(0, 3, 1, 2)
        return F.gelu(xn + F.conv2d(xn, d["w"], d["b"], padding=1, groups=Cc)).permute(0, 2, 3, 1)
    (want, gw), (stock, gs) = run_pair(fn, ins, cot)
    dev = {n: t.clone().to(DEV).requires_grad_(True) for n, t in ins.items()}
    got = ops.dwconv_res_gelu(dev["x"], dev["w"], dev["b"])
    gg = dict(zip(dev, torch.autograd.grad(got, list(dev.values()), cot.to(DEV))))
    case = f"dwconv_res_gelu{shape}"
    check(case, "out", ("rel", 2e-6), got, want)
    check(case, "dx", ("rel", 2e-5), gg["x"], gw["x"])
    check(case, "dw", ("rel", 2e-5), gg["w"], gw["w"], gs["w"])
    check(case, "db", ("rel", 2e-5), gg["b"], gw["b"], gs["b"])


@pytest.mark.parametrize("prec_name", ["bf16", "f16"])
@pytest.mark.parametrize("with_lse", [False, True])
def test_attn_bwd_prep_against_float64(prec_name, with_lse):
    """test_attn_bwd_prep_matches_the_stock_chain's shape: delta and the two maxima against float64"""
    inf_rows = torch.tensor([(0 * 2 + 1) * 7 * 32 + 5])
    _check_bwd_prep(f"attn_bwd_prep(6, 224) {prec_name} lse={with_lse}", 3, 2, 7 * 32, prec_name, with_lse, inf_rows)


# =====================================================================================================================
# C. what padding rows and empty segments hold
# =====================================================================================================================
def test_merge_tap_ignores_what_the_padding_rows_hold():
    """test_merge_views_ignores_what_the_padding_rows_hold for merge_tap: rows i >= S of O_r hold NaN and +inf and those of
    L_r hold -inf (what the region kernels leave there); Rn and L_c are 0 on those rows, as _TapAttn guarantees (it
    allocates both zeroed and the tap kernels write live rows only) -- merge_tap_bwd_kernel relies on exactly that when
    it accumulates goc * rn into dVp.  Forward bit-equal to the clean run; all six gradients finite and the clean run's
    (dVp, dbv up to the order of their float atomics: test_merge_tap_matches_the_stock_chain's 3e-5)."""
    B, V, h, S, c = 1, 2, 2, 20, 32
    Sp = 32
    ins, _ = _merge_tap_inputs(B, V, h, S, c, _gen(5))
    rows = lambda t: t.reshape(B * V, h, S, Sp, -1)[:, :, :, S:]
    rows(ins["Rn"]).zero_()
    rows(ins["L_c"]).zero_()
    cot = torch.randn(B, S * S, V * h * c, generator=_gen(6)).to(DEV)
    res = []
    for dirty in (False, True):
        d = {n: t.clone() for n, t in ins.items()}
        if dirty:
            pad = rows(d["O_r"])
            pad[..., 0::2] = float("nan")
            pad[..., 1::2] = float("inf")
            rows(d["L_r"]).fill_(float("-inf"))
        d = {n: t.to(DEV).requires_grad_(True) for n, t in d.items()}
        out = ops.merge_tap(d["O_r"], d["L_r"], d["Rn"], d["L_c"], d["Vp"], d["bv"], S, c, V)
        res.append((out.detach(), dict(zip(d, torch.autograd.grad(out, list(d.values()), cot)))))
    (clean, gc), (out, gd) = res
    assert torch.equal(out, clean)
    for n in ins:
        assert torch.isfinite(gd[n]).all(), n
        if n in ("Vp", "bv"):
            check("merge_tap dirty padding", "d" + n, ("rel", 3e-5), gd[n], gc[n].cpu().double())
        else:
            assert torch.equal(gd[n], gc[n]), n


def _empty_side_rows(L_r, L_c, S, Sp, gen):
    """~5 % of the live rows lose one segment: L_r = -inf on half of them, L_c = -inf on the others; never both"""
    live = (torch.arange(L_r.shape[-1]) % Sp) < S
    pick = (torch.rand(L_r.shape, generator=gen) < 0.05) & live
    side = torch.rand(L_r.shape, generator=gen) < 0.5
    er, ec = pick & side, pick & ~side
    assert er.sum() > 20 and ec.sum() > 20 and not (er & ec).any()
    L_r[er] = float("-inf")
    L_c[ec] = float("-inf")
    return er, ec


def test_merge_views_with_one_segment_empty_on_some_rows():
    """A live row whose first or second key segment is empty (L = -inf, O finite -- the rows attn_bwd_prep treats
    specially): the float64 chain gives the other segment's output unchanged, no gradient to the empty side's O and no
    dL.  Forward and every gradient at test_merge_views_matches_the_stock_chain's limits."""
    B, V, h, S, c = 2, 3, 2, 21, 32
    ins, Sp = _merge_views_inputs(B, V, h, S, c, True, _gen(S * 7 + c))
    er, ec = _empty_side_rows(ins["L_r"], ins["L_c"], S, Sp, _gen(4))
    want, gw, got, gg = _check_merge_views("merge_views one side empty", ins, B, V, h, S, c, Sp, _gen(5))
    # what the float64 chain gives on those rows
    assert not gw["O_r"][er].ne(0).any() and not gw["O_c"][ec].ne(0).any()
    assert not gw["L_r"][er | ec].ne(0).any() and not gw["L_c"][er | ec].ne(0).any()
    one = ops.unpack_out_views(torch.where(er[..., None], ins["O_c"], ins["O_r"]).double(), S, c, V)
    mask = ops.unpack_out_views((er | ec)[..., None].expand(-1, -1, -1, 32).double(), S, c, V) > 0
    assert torch.equal(want[mask], one[mask])
    # and the kernel: exactly so
    for n, m in (("O_r", er), ("O_c", ec), ("L_r", er | ec), ("L_c", er | ec)):
        assert not gg[n].cpu()[m].ne(0).any(), n
    assert torch.equal(got.cpu()[mask], one.float()[mask])


def test_merge_tap_with_one_segment_empty_on_some_rows():
    """The same for merge_tap (O_c = Rn Vp + bv): forward and the six gradients at test_merge_tap_matches_the_stock_chain's
    limits; on the rows with one side empty d(L) is zero, and so is d(O_r) where L_r = -inf and d(Rn) where L_c = -inf."""
    B, V, h, S, c = 2, 3, 2, 21, 32
    ins, Sp = _merge_tap_inputs(B, V, h, S, c, _gen(S + c))
    er, ec = _empty_side_rows(ins["L_r"], ins["L_c"], S, Sp, _gen(7))
    got, gg = _check_merge_tap("merge_tap one side empty", ins, B, V, h, S, c, _gen(8))
    for n, m in (("O_r", er), ("Rn", ec), ("L_r", er | ec), ("L_c", er | ec)):
        assert not gg[n].cpu()[m].ne(0).any(), n


# =====================================================================================================================
# D. cotangent scale
# =====================================================================================================================
SCALES = [2.0 ** -120, 2.0 ** -100, 2.0 ** -60, 1.0, 2.0 ** 60, 2.0 ** 100]
_SAMPLE_REF = {}


def _sample_scale_problem(path):
    """patch path: C = 64, half the keys near the pinned corner (some exactly on it), the rest anywhere; scatter path:
    C = 12 (C / 4 does not divide the workgroup).  The float64 reference at s = 1, computed once."""
    if path not in _SAMPLE_REF:
        B, Cc, Hi, Wi, N = (2, 64, 16, 44, 2000) if path == "patch" else (2, 12, 9, 7, 600)
        gen = _gen(641 if path == "patch" else 12)      # seeds at which at most one key sits on a pixel centre by chance
        feat = torch.randn(B, Cc, Hi, Wi, generator=gen)
        pos = (torch.rand(B, N, 2, generator=gen) * 2 - 1) * 1.2
        placed = torch.zeros(B, N, dtype=torch.bool)
        pos[:, :N // 2] = -1.0 + torch.tanh(torch.randn(B, N // 2, 2, generator=gen)) * torch.tensor([0.2, 0.1])
        pos[:, :N // 8] = -1.0
        placed[:, :N // 8] = True
        pos[0, -3:] = torch.tensor([[1., 1.], [-1., 1.], [0., 0.]])
        placed[0, -3:] = True
        # no entry below 2^-6: s cot is then exact in float32 down to s = 2^-120 (none becomes a subnormal float)
        cot = torch.randn(B, N, Cc, generator=gen)
        cot = torch.where(cot.abs() < 2.0 ** -6, cot + torch.where(cot < 0, -1.0, 1.0) * 2.0 ** -6, cot)
        fc, pc = feat.double().requires_grad_(True), pos.double().requires_grad_(True)
        dfeat, dpos = torch.autograd.grad(_grid_sample(fc, pc), (fc, pc), cot.double())
        _SAMPLE_REF[path] = (feat, pos, cot, dfeat, dpos, _smooth_keys(pos, Hi, Wi, placed))
    return _SAMPLE_REF[path]


@pytest.mark.parametrize("s", SCALES, ids=lambda s: f"2^{int(math.log2(s))}")
@pytest.mark.parametrize("path", ["patch", "scatter"])
def test_sample_backward_under_a_scaled_cotangent(path, s):
    """bevr_sample_bwd is linear in the cotangent: d(feat) / s and d(pos) / s of the cotangent s cot against the float64
    reference at s = 1, for every s at the limits of test_sample_backward_with_most_keys_pinned_to_the_corner (the existing
    test of both paths against float64: d(feat) 2e-5 of max, d(pos) 1e-4 / 1e-4 of max).  The patch kernel's 64-bit
    fixed-point cells are in units of the chunk's largest |dout| * 2^-40, a subnormal float below |dout| ~ 2^-86: such
    chunks take the direct scatter (csrc/sample.hip unit_ok).  Before that, d(feat) of the patch path came back coarsely
    quantised at s = 2^-100 (2.3 x the limit) and as zeros at s = 2^-120."""
    feat, pos, cot, dfeat_w, dpos_w, keep = _sample_scale_problem(path)
    Cc = feat.shape[1]
    assert ((256 % (Cc // 4) == 0) and Cc * 8 * 32 <= 48 * 1024) == (path == "patch")       # csrc/sample.hip sample_bwd: patch_ok
    fg, pg = feat.clone().to(DEV).requires_grad_(True), pos.clone().to(DEV).requires_grad_(True)
    got = ops.sample_features(fg, pg, 1)
    scaled = cot * s
    assert torch.equal(scaled.double() / s, cot.double())                # a power of two: the scaling is exact
    assert not ((scaled != 0) & (scaled.abs() < 2.0 ** -126)).any()
    dfeat, dpos = torch.autograd.grad(got, (fg, pg), scaled.to(DEV))
    case = f"sample bwd {path} s=2^{int(math.log2(s))}"
    dfeat, dpos = dfeat.cpu().double() / s, dpos.cpu().double() / s
    errs = [(n, ratio(t, a, b)) for n, t, a, b in (("dfeat", ("rel", 2e-5), dfeat, dfeat_w),
                                                     ("dpos", ("allclose", 1e-4, 1e-4 * dpos_w.abs().max().item()), dpos[keep], dpos_w[keep]))]
    for n, r in errs:
        TABLE.append((case, n, r, None, 1.0))
    print(f"\n[{case}] " + ", ".join(f"{n} at {r:.3g} x its tolerance" for n, r in errs))
    for n, r in errs:
        assert r < 1.0, f"{case}: {n} at {r:.3g} x its tolerance"


# a case whose gradient is STORED in a 16-bit type may drop an s that leaves that type's range: none does -- sample_bf16
# stores d(feat) in bfloat16, whose exponent range is float32's, so both scales stay.
GLUE_SCALES = [2.0 ** -100, 2.0 ** 100]


@pytest.mark.parametrize("s", GLUE_SCALES, ids=lambda s: f"2^{int(math.log2(s))}")
@pytest.mark.parametrize("cid", list(glue.BUILDERS))
def test_glue_backward_under_a_scaled_cotangent(cid, s):
    """every case of test_gpu_grad_patterns_glue.BUILDERS with its cotangent scaled by s: each gradient / s within the
    case's own grad_tol of its float64 reference (computed once, shared with that module)"""
    c = glue.case(cid)
    want, cot, grads, _ = c.oracle()
    req = set(c.ins)
    gpu = c.leaves(req)
    got = c.dev(gpu)
    scaled = cot.float() * s
    assert torch.equal(scaled.double() / s, cot.float().double())
    got.backward(scaled.to(DEV))
    for n, t in gpu.items():
        assert t.grad is not None and t.grad.dtype == t.dtype
        v = c.view.get(n, lambda x: x)
        r = ratio(c.grad_tol[n], v(t.grad.detach().cpu().double() / s), v(grads[n]))
        TABLE.append((f"{c.name} s=2^{int(math.log2(s))}", "d" + n, r, None, 1.0))
        assert r < 1.0, f"{c.name} s={s}: grad {n} at {r:.3g} x its limit {c.grad_tol[n]}"
