"""The autograd Functions around the attention core under the gradient patterns training uses: every non-empty subset of
the differentiable inputs (ops.py branches on ctx.needs_input_grad: which kernels are launched, which pointers are NULL),
the forward under torch.no_grad(), non-contiguous / stride-0 / all-zero cotangents, and the backward replayed on one graph.

One small shape per op, taken from the op's existing test, whose tolerance carries over UNCHANGED (named at each case);
the reference is that test's stock chain in float64 on the CPU.  The launches are seen through a spy on ops._launch (most
of these entry points are not timed launches, so ops.KERNEL_TIMER does not record them).

Forward kernels without atomics -- bit-equal under no_grad and in grad mode: sample, offset_head, layer_norm, dwconv,
dwconv_res_gelu, merge_views, merge_tap, key_positions, affine_warp, and linear_rows (one rocBLAS call either way).
bevr_corr_fwd accumulates its dot products with float atomics: compared at the existing test's forward tolerance.

_OffsetHead with w0 given and b0 None is not covered: no module builds it (SCADeformableAttention's depthwise 1x1 has a
bias, TSADeformableAttention passes neither)."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from bevrender_amd import ops
from oracle import bevrender_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}


def teardown_module(module):
    print("\n[grad patterns glue] worst error / its limit, per op:", {k: f"{v:.2f}" for k, v in sorted(WORST.items())})


def ratio(tol, a, b):
    """error of a against b as a fraction of the limit `tol`:
    ("allclose", rtol, atol): np.testing.assert_allclose's rule; ("rel", lim): max |a - b| <= lim max |b| (rel_err);
    ("absmax", lim): max |a - b| <= lim max(max |b|, 1)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    d = (a - b).abs()
    if tol[0] == "allclose":
        return (d / (tol[2] + tol[1] * b.abs())).max().item()
    if tol[0] == "rel":
        return d.max().item() / (b.abs().max().item() + 1e-30) / tol[1]
    return d.max().item() / (tol[1] * max(b.abs().max().item(), 1.0))


class Case:
    """ins: the differentiable inputs (CPU); dev(d) the op on device leaves, ref(d) the stock chain on float64 leaves."""

    def __init__(self, name, ins, dev, ref, out_tol, grad_tol, launches=None, subsets=True, exact_fwd=True, stock=None,
                 view=None):
        self.name, self.ins, self.dev, self.ref = name, ins, dev, ref
        self.out_tol, self.grad_tol, self.launches, self.subsets = out_tol, grad_tol, launches, subsets
        self.exact_fwd, self.stock, self.view = exact_fwd, stock, view or {}
        self._oracle = None

    def oracle(self):
        if self._oracle is None:
            cpu = {n: t.clone().double().requires_grad_(True) for n, t in self.ins.items()}
            want = self.ref(cpu)
            cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
            leaves = list(cpu.values())
            g = dict(zip(cpu, torch.autograd.grad(want, leaves, cot, retain_graph=True)))
            gs = dict(zip(cpu, torch.autograd.grad(want, leaves, torch.ones_like(want))))
            self._oracle = (want.detach(), cot, g, gs)
        return self._oracle

    def leaves(self, requires):
        return {n: t.clone().to(DEV).requires_grad_(n in requires) for n, t in self.ins.items()}

    def note(self, r):
        WORST[self.name] = max(WORST.get(self.name, 0.0), r)

    def check_out(self, got, tag):
        r = ratio(self.out_tol, got, self.oracle()[0])
        self.note(r)
        assert r < 1.0, f"{tag}: forward at {r:.2f} x its limit {self.out_tol}"

    def check_grads(self, gpu, requires, ref, tag):
        worst = 0.0
        for n, t in gpu.items():
            if n not in requires:
                assert t.grad is None, f"{tag}: {n} does not require grad and got one"
                continue
            assert t.grad is not None, f"{tag}: no gradient for {n}"
            assert t.grad.dtype == t.dtype and t.grad.shape == t.shape
            v = self.view.get(n, lambda x: x)
            r = ratio(self.grad_tol[n], v(t.grad), v(ref[n]))
            self.note(r)
            worst = max(worst, r)
            assert r < 1.0, f"{tag}: grad {n} at {r:.2f} x its limit {self.grad_tol[n]}"
        return worst


class Spy:
    """records (entry, args) of every ops._launch"""

    def __init__(self, monkeypatch):
        self.calls = []
        orig = ops._launch

        def spy(entry, *args, **kw):
            self.calls.append((entry, args))
            return orig(entry, *args, **kw)
        monkeypatch.setattr(ops, "_launch", spy)

    def take(self):
        calls, self.calls = self.calls, []
        return calls


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def sample_case(bf16):
    """ops.sample_features on a (2, 6, 7, 16) channels-last map, N = 50, positions partly outside the map.  Tolerances of
    test_sample_features_matches_grid_sample (out 1e-5 / 1e-6, d(feat) 1e-4 / 1e-5, d(pos) 1e-4 / 2e-5); the bf16 map's
    gradient is stored in bf16: 2^-7 of the largest entry (test_sample_features_reads_bf16_features_as_they_are)."""
    B, C, Hi, Wi, N = 2, 16, 6, 7, 50
    gen = _gen(5)
    feat = torch.randn(B, C, Hi, Wi, generator=gen)
    pos = (torch.rand(B, N, 2, generator=gen) * 2 - 1) * 1.2
    pos[0, :8] = torch.tensor([[-1., -1.], [1., 1.], [-1., 1.], [0., 0.], [1.5, 0.], [0., -1.5], [.999, .999], [3., 3.]])
    if bf16:
        feat = feat.to(torch.bfloat16)

    def dev(d):
        return ops.sample_features(d["feat"], d["pos"], 1)

    def ref(d):
        return F.grid_sample(d["feat"], d["pos"][:, None, :, (1, 0)], mode="bilinear",
                             align_corners=True).reshape(B, C, N).permute(0, 2, 1)

    def launches(req, calls, backward):
        names = [c[0] for c in calls]
        sfx = "_bf16" if bf16 else ""
        assert names == ["bevr_sample_fwd" + sfx] + (["bevr_sample_bwd" + sfx] if backward else []), names
    return Case("sample_bf16" if bf16 else "sample", dict(feat=feat, pos=pos), dev, ref, ("allclose", 1e-5, 1e-6),
                dict(feat=("rel", 2.0 ** -7) if bf16 else ("allclose", 1e-4, 1e-5), pos=("allclose", 1e-4, 2e-5)), launches)


def offset_head_case(cfg):
    """test_fused_offset_head_matches_the_stock_op_chain's cases and tolerances (out 2e-5 / 2e-5, gradients 2e-5 of max)."""
    B, H, W, Cc, g, mx, dout = cfg
    cg = Cc // g
    K = cg * mx
    gen = _gen(sum(cfg))
    ins = dict(x=torch.randn(B, H, W, Cc, generator=gen))
    if mx > 1 or dout == mx:
        ins["w0"] = torch.randn(K, generator=gen) * 0.7
        ins["b0"] = torch.randn(K, generator=gen) * 0.3
    ins["gamma"], ins["beta"] = 1 + 0.2 * torch.randn(K, generator=gen), 0.1 * torch.randn(K, generator=gen)
    ins["W3"] = torch.randn(dout, K, generator=gen) / K ** 0.5

    def dev(d):
        return ops.offset_head(d["x"], d.get("w0"), d.get("b0"), d["gamma"], d["beta"], d["W3"], groups=g)

    def ref(d):
        xg = d["x"].reshape(B, H, W, g, cg).permute(0, 3, 1, 2, 4).reshape(B * g, H, W, cg)
        z = xg if "w0" not in d else (xg.unsqueeze(-1) * d["w0"].view(cg, mx) + d["b0"].view(cg, mx)).flatten(-2)
        return F.gelu(F.layer_norm(z, (K,), d["gamma"], d["beta"], 1e-5)) @ d["W3"].t()

    def launches(req, calls, backward):
        bwd = [a for e, a in calls if e == "bevr_offset_head_bwd"]
        assert len(bwd) == (g if backward else 0), [c[0] for c in calls]
        for a in bwd:       # argument 7: dx -- NULL when x takes no gradient
            assert (a[7] is None) == ("x" not in req), (sorted(req), a[7])
    return Case(f"offset_head{cfg}", ins, dev, ref, ("allclose", 2e-5, 2e-5), {n: ("rel", 2e-5) for n in ins}, launches)


def layer_norm_case(shape):
    """test_layer_norm_matches_torch's tolerances (out 2e-5 / 2e-5, gradients 2e-5 of max).  (2048 16 + 5, 64): the
    grid-stride loop of csrc/layernorm.hip takes a second, ragged iteration."""
    Cc = shape[-1]
    gen = _gen(sum(shape))
    ins = dict(x=torch.randn(*shape, generator=gen) * 2.0 + 0.5, gamma=torch.randn(Cc, generator=gen),
               beta=torch.randn(Cc, generator=gen))
    return Case(f"layer_norm{shape}", ins, lambda d: ops.layer_norm(d["x"], d["gamma"], d["beta"], 1e-5),
                lambda d: F.layer_norm(d["x"], (Cc,), d["gamma"], d["beta"], 1e-5), ("allclose", 2e-5, 2e-5),
                {n: ("rel", 2e-5) for n in ins})


def dwconv_case(nhwc, bias):
    """test_depthwise_conv_matches_torch's smallest shape and tolerances (out, dx 1e-5 / 1e-5; dw, dbias 2e-4 / 2e-4)."""
    B, Cc, H, W, k = 2, 8, 9, 7, 3
    gen = _gen(B * 100 + Cc + k)
    ins = dict(x=torch.randn(B, Cc, H, W, generator=gen), w=torch.randn(Cc, 1, k, k, generator=gen) * 0.3)
    if bias:
        ins["b"] = torch.randn(Cc, generator=gen)

    def dev(d):
        if nhwc:
            return ops.depthwise_conv(d["x"].permute(0, 2, 3, 1).contiguous(), d["w"], d.get("b"), nhwc=True).permute(0, 3, 1, 2)
        return ops.depthwise_conv(d["x"], d["w"], d.get("b"), nhwc=False)

    def launches(req, calls, backward):
        flips = [a for e, a in calls if e == "bevr_dwconv_fwd" and a[10] == 1]       # argument 10: flip
        bwd_w = [a for e, a in calls if e == "bevr_dwconv_bwd_w"]
        assert len(flips) == int(backward and "x" in req), (sorted(req), [c[0] for c in calls])
        assert len(bwd_w) == int(backward and bool(req & {"w", "b"})), (sorted(req), [c[0] for c in calls])
    return Case(f"dwconv(nhwc={nhwc}, bias={bias})", ins, dev, lambda d: F.conv2d(d["x"], d["w"], d.get("b"), padding=k // 2, groups=Cc),
                ("allclose", 1e-5, 1e-5), dict(x=("allclose", 1e-5, 1e-5), w=("allclose", 2e-4, 2e-4), b=("allclose", 2e-4, 2e-4)),
                launches)


def res_gelu_case(bias):
    """test_dwconv_res_gelu_matches_the_stock_chain's smallest shape and tolerances (out 2e-6, gradients 2e-5 of max)."""
    B, H, W, Cc = 2, 9, 7, 8
    gen = _gen(H * 3 + Cc)
    ins = dict(x=torch.randn(B, H, W, Cc, generator=gen), w=torch.randn(Cc, 1, 3, 3, generator=gen) * 0.3)
    if bias:
        ins["b"] = torch.randn(Cc, generator=gen)

    def ref(d):
        xn = d["x"].permute(0, 3, 1, 2)
        return F.gelu(xn + F.conv2d(xn, d["w"], d.get("b"), padding=1, groups=Cc)).permute(0, 2, 3, 1)

    def launches(req, calls, backward):
        modes = [a[10] for e, a in calls if e == "bevr_dwconv_res_gelu"]                # argument 10: mode
        bwd_w = [a for e, a in calls if e == "bevr_dwconv_bwd_w"]
        assert modes == [1] + ([2] + ([3] if "x" in req else []) if backward else []), (sorted(req), modes)
        assert len(bwd_w) == int(backward and bool(req & {"w", "b"})), (sorted(req), [c[0] for c in calls])
    return Case(f"dwconv_res_gelu(bias={bias})", ins, lambda d: ops.dwconv_res_gelu(d["x"], d["w"], d.get("b")), ref,
                ("rel", 2e-6), {n: ("rel", 2e-5) for n in ins}, launches)


def linear_rows_case(bias):
    """ops.linear_rows just over LINEAR_ROWS_MIN and ragged against its 4 096-row chunk; test_linear_rows_matches_f_linear's
    tolerances: the forward EQUALS F.linear on the device, gradients 1e-5 of max."""
    rows, K, N = 65536 + 37, 8, 12
    assert rows >= ops.LINEAR_ROWS_MIN and rows % ops.LINEAR_ROWS_CHUNK
    gen = _gen(rows + K)
    ins = dict(x=torch.randn(rows, K, generator=gen), w=torch.randn(N, K, generator=gen) * 0.1)
    if bias:
        ins["b"] = torch.randn(N, generator=gen)
    return Case(f"linear_rows(bias={bias})", ins, lambda d: ops.linear_rows(d["x"], d["w"], d.get("b")),
                lambda d: F.linear(d["x"], d["w"], d.get("b")), ("rel", 1e-5), {n: ("rel", 1e-5) for n in ins},
                stock=lambda d: F.linear(d["x"].detach(), d["w"].detach(), None if "b" not in d else d["b"].detach()))


def _chain(O_r, L_r, O_c, L_c, S, c, views):        # tests/test_gpu_merge.py
    if O_c is not None:
        L_t = torch.logaddexp2(L_r, L_c)
        O_r = torch.exp2(L_r - L_t)[..., None] * O_r + torch.exp2(L_c - L_t)[..., None] * O_c
    return ops.unpack_out_views(O_r, S, c, views)


def merge_case(kind):
    """merge_views (one and two segments) and merge_tap at B = 1, V = 2, h = 2, S = 5, c = 8, with the tolerances of
    tests/test_gpu_merge.py: merge_views out 2e-6, dO 2e-6, dL 2e-5; merge_tap out 3e-6, gradients 3e-5 (dVp, dbv on the
    head's real channels)."""
    B, V, h, S, c = 1, 2, 2, 5, 8
    Sp = 32
    Mp = S * Sp
    gen = _gen(S * 7 + c)

    def mk(*shape, scale=1.0):
        return torch.randn(*shape, generator=gen) * scale
    if kind == "tap":
        ins = dict(O_r=mk(B * V, h, Mp, 32), L_r=mk(B * V, h, Mp, scale=5.0), Rn=mk(B * V, h, Mp, 12), L_c=mk(B * V, h, Mp, scale=5.0),
                   Vp=mk(B * V, h, 12, 32), bv=mk(h, 32))
        ins["Vp"][..., c:] = 0.0
        ins["bv"][..., c:] = 0.0
        cut = lambda t: t[..., :c]
        return Case("merge_tap", ins, lambda d: ops.merge_tap(d["O_r"], d["L_r"], d["Rn"], d["L_c"], d["Vp"], d["bv"], S, c, V),
                    lambda d: _chain(d["O_r"], d["L_r"], torch.matmul(d["Rn"], d["Vp"]) + d["bv"][None, :, None, :], d["L_c"], S, c, V),
                    ("rel", 3e-6), {n: ("rel", 3e-5) for n in ins}, view=dict(Vp=cut, bv=cut))
    if kind == "two":
        ins = dict(O_r=mk(B * V, h, Mp, 32), L_r=mk(B * V, h, Mp, scale=6.0), O_c=mk(B * V, h, Mp, 32), L_c=mk(B * V, h, Mp, scale=6.0))
        return Case("merge_views(two)", ins, lambda d: ops.merge_views(d["O_r"], S, c, V, d["L_r"], d["O_c"], d["L_c"]),
                    lambda d: _chain(d["O_r"], d["L_r"], d["O_c"], d["L_c"], S, c, V), ("rel", 2e-6),
                    dict(O_r=("rel", 2e-6), O_c=("rel", 2e-6), L_r=("rel", 2e-5), L_c=("rel", 2e-5)))
    ins = dict(O_r=mk(B * V, h, Mp, 32))
    return Case("merge_views(one)", ins, lambda d: ops.merge_views(d["O_r"], S, c, V),
                lambda d: _chain(d["O_r"], None, None, None, S, c, V), ("rel", 2e-6), dict(O_r=("rel", 2e-6)))


def key_positions_case(sca):
    """test_key_positions_sca_ / _tsa_equals_the_stock_op_chain's smallest case (tanh form) and tolerances (out 1e-5 / 2e-6,
    d(off) 1e-4 / 1e-6).  One differentiable input."""
    if sca:
        B, V, g, S, D = 2, 3, 1, 8, 3
        Hk, Wk = S // 2, S * D
        N = Hk * Wk
        gen = _gen(S * D + V)
        off = torch.randn(V, B * g, S, S, D, generator=gen) * 1.5
        ref_pts = torch.rand(V, N, 2, generator=gen) * 2.2 - 1.1
        order = torch.stack([torch.randperm(N, generator=gen) for _ in range(V)])
        sy, sx = 0.7 / (Hk - 1.0), 1.3 / (Wk - 1.0)

        def ref(d):
            outs = []
            for v in range(V):
                o = d["off"][v].reshape(B * g, Hk, 2, S, D).permute(0, 2, 1, 3, 4).reshape(B * g, 2, Hk, Wk)
                o = o.tanh() * torch.tensor([sy, sx], dtype=torch.float64).reshape(1, 2, 1, 1)
                outs.append(o.permute(0, 2, 3, 1).reshape(B, g, N, 2) + ref_pts[v].double()[None, None])
            return torch.stack(outs, 1).gather(3, order[None, :, None, :, None].expand(B, V, g, N, 2))
        dev = lambda d: ops.key_positions(d["off"], ref_pts.to(DEV), order.to(DEV), B, g, sca_SD=(S, D), use_tanh=True, sy=sy, sx=sx)
    else:
        B, g, Hk, Wk = 2, 2, 7, 9
        N = Hk * Wk
        gen = _gen(5)
        off = torch.randn(1, B * g, N, 2, generator=gen)
        grid = O.normalized_grid(Hk, Wk, torch.float32).reshape(1, N, 2)
        order = torch.randperm(N, generator=gen)[None]
        sy, sx = 2.0 / (Hk - 1.0), 2.0 / (Wk - 1.0)

        def ref(d):
            p = d["off"][0].tanh() * torch.tensor([sy, sx], dtype=torch.float64) + grid.double()
            return p.index_select(1, order[0]).reshape(B, 1, g, N, 2)
        dev = lambda d: ops.key_positions(d["off"], grid.to(DEV), order.to(DEV), B, g, sca_SD=None, use_tanh=True, sy=sy, sx=sx)
    return Case(f"key_positions({'sca' if sca else 'tsa'})", dict(off=off), dev, ref, ("allclose", 1e-5, 2e-6),
                dict(off=("allclose", 1e-4, 1e-6)), subsets=False)


def warp_case():
    """test_warp_backward_matches_autograd_of_the_oracle's case (the history warp as EncoderLayer runs it) with its
    tolerance, 1e-4 / 1e-4, forward (test_project_history_matches_oracle) and gradient.  One differentiable input."""
    from bevrender_amd.model.encoder import EncoderLayer
    B, C, H, W = 2, 3, 10, 13
    gen = _gen(2)
    bev = torch.randn(B, C, H, W, generator=gen)
    pose = torch.randn(B, 2, 3, generator=gen) * torch.tensor([2.0, 2.0, 0.5])
    return Case("affine_warp", dict(bev=bev), lambda d: EncoderLayer.project_history_bev_feat(None, d["bev"], pose.to(DEV)),
                lambda d: O.project_history_bev_feat(d["bev"], pose.double()), ("allclose", 1e-4, 1e-4),
                dict(bev=("allclose", 1e-4, 1e-4)), subsets=False)


def corr_case(normalize):
    """test_pairwise_corr_and_recall's case and tolerances (out 2e-5 max(max |D|, 1), gradients 1e-4 of max); its gradient
    subsets are tests/test_gpu_corr_alias.py's."""
    n, m, E = 8, 8, 64 * 28 * 28
    gen = _gen(9)
    cam = torch.randn(n, E, generator=gen)
    mp = cam + 0.8 * torch.randn(m, E, generator=gen)

    def ref(d):
        a, b = (F.normalize(d["cam"], dim=1), F.normalize(d["map"], dim=1)) if normalize else (d["cam"], d["map"])
        return O.pairwise_corr(a, b)
    return Case(f"pairwise_corr(normalize={normalize})", dict(cam=cam, map=mp), lambda d: ops.pairwise_corr(d["cam"], d["map"], normalize),
                ref, ("absmax", 2e-5), dict(cam=("rel", 1e-4), map=("rel", 1e-4)), subsets=False, exact_fwd=False)


BUILDERS = {
    "sample": lambda: sample_case(False), "sample_bf16": lambda: sample_case(True),
    "offset_head_sca": lambda: offset_head_case((1, 6, 6, 16, 2, 3, 3)), "offset_head_tsa": lambda: offset_head_case((2, 5, 8, 32, 1, 1, 2)),
    "layer_norm_c8": lambda: layer_norm_case((3, 5, 5, 8)), "layer_norm_c256": lambda: layer_norm_case((1, 13, 1, 256)),
    "layer_norm_two_iterations": lambda: layer_norm_case((2048 * 16 + 5, 64)),
    "dwconv_nchw_bias": lambda: dwconv_case(False, True), "dwconv_nchw": lambda: dwconv_case(False, False),
    "dwconv_nhwc_bias": lambda: dwconv_case(True, True), "dwconv_nhwc": lambda: dwconv_case(True, False),
    "res_gelu_bias": lambda: res_gelu_case(True), "res_gelu": lambda: res_gelu_case(False),
    "linear_rows_bias": lambda: linear_rows_case(True), "linear_rows": lambda: linear_rows_case(False),
    "merge_views_one": lambda: merge_case("one"), "merge_views_two": lambda: merge_case("two"), "merge_tap": lambda: merge_case("tap"),
    "key_positions_sca": lambda: key_positions_case(True), "key_positions_tsa": lambda: key_positions_case(False),
    "affine_warp": warp_case, "corr": lambda: corr_case(False), "corr_normalized": lambda: corr_case(True),
}
_CASES = {}


def case(cid):
    if cid not in _CASES:
        _CASES[cid] = BUILDERS[cid]()
    return _CASES[cid]


SUBSET_CASES = [k for k in BUILDERS if not k.startswith(("key_positions", "affine_warp", "corr"))]


@pytest.mark.parametrize("cid", SUBSET_CASES)
def test_every_subset_of_the_inputs_requiring_grad(cid, monkeypatch):
    c = case(cid)
    assert c.subsets
    want, cot, grads, _ = c.oracle()
    spy = Spy(monkeypatch)
    names = list(c.ins)
    worst, count = 0.0, 0
    for k in range(1, len(names) + 1):
        for sub in itertools.combinations(names, k):
            req = set(sub)
            tag = f"{c.name} grads of {sorted(req)}"
            gpu = c.leaves(req)
            got = c.dev(gpu)
            c.check_out(got, tag)
            if c.stock is not None:
                assert torch.equal(got.detach(), c.stock(gpu)), f"{tag}: forward differs from the stock op"
            got.backward(cot.float().to(DEV))
            worst = max(worst, c.check_grads(gpu, req, grads, tag))
            calls = spy.take()
            if c.launches is not None:
                c.launches(req, calls, True)
            count += 1
    print(f"\n[glue {c.name}] {count} subsets, worst gradient error / limit {worst:.2f}")


@pytest.mark.parametrize("cid", list(BUILDERS))
def test_forward_under_no_grad(cid, monkeypatch):
    c = case(cid)
    spy = Spy(monkeypatch)
    gpu = c.leaves(set(c.ins))
    with torch.no_grad():
        quiet = c.dev(gpu)
    calls = spy.take()
    assert not quiet.requires_grad
    assert not [e for e, _ in calls if "_bwd" in e], [e for e, _ in calls]
    if c.launches is not None:
        c.launches(set(c.ins), calls, False)
    c.check_out(quiet, f"{c.name} no_grad")
    loud = c.dev(gpu)
    assert loud.requires_grad
    if c.exact_fwd:
        assert torch.equal(quiet, loud.detach()), f"{c.name}: the no_grad forward differs from the grad-mode forward"
    else:
        r = ratio(c.out_tol, quiet, loud)
        assert r < 1.0, f"{c.name}: no_grad against grad-mode forward at {r:.2f} x the limit"
    # nothing requires grad, grad mode on
    plain = c.dev(c.leaves(set()))
    assert not plain.requires_grad
    c.check_out(plain, f"{c.name} nothing requires grad")


@pytest.mark.parametrize("cid", list(BUILDERS))
def test_cotangent_forms(cid):
    """non-contiguous (a slice of a wider buffer along the last axis), stride 0 (out.sum().backward()), all zero"""
    c = case(cid)
    want, cot, grads, grads_sum = c.oracle()
    req = set(c.ins)
    gpu = c.leaves(req)
    got = c.dev(gpu)
    wide = torch.zeros(*got.shape[:-1], got.shape[-1] + 5, device=DEV)
    view = wide[..., 2:2 + got.shape[-1]]
    view.copy_(cot.float())
    assert not view.is_contiguous()
    got.backward(view)
    w1 = c.check_grads(gpu, req, grads, f"{c.name} sliced cotangent")
    gpu = c.leaves(req)
    c.dev(gpu).sum().backward()
    w2 = c.check_grads(gpu, req, grads_sum, f"{c.name} sum()")
    print(f"\n[glue {c.name}] cotangent forms: sliced {w1:.2f}, stride 0 {w2:.2f} of the limit")
    gpu = c.leaves(req)
    got = c.dev(gpu)
    got.backward(torch.zeros_like(got))
    for n, t in gpu.items():
        assert t.grad is not None and torch.isfinite(t.grad.float()).all(), f"{c.name}: grad {n} under a zero cotangent"
        assert not t.grad.ne(0).any(), f"{c.name}: grad {n} max |.| {t.grad.abs().max().item():.3e} under a zero cotangent"


@pytest.mark.parametrize("cid", list(BUILDERS))
def test_backward_replayed_on_one_graph(cid):
    """backward(retain_graph=True) twice: both replays within the limits of the reference, the second within them of the
    first (float atomics forbid bit equality), and the output untouched."""
    c = case(cid)
    want, cot, grads, _ = c.oracle()
    req = set(c.ins)
    gpu = c.leaves(req)
    got = c.dev(gpu)
    before = got.detach().clone()
    cot = cot.float().to(DEV)
    got.backward(cot, retain_graph=True)
    w1 = c.check_grads(gpu, req, grads, f"{c.name} replay 1")
    first = {n: t.grad.detach().clone() for n, t in gpu.items()}
    for t in gpu.values():
        t.grad = None
    got.backward(cot, retain_graph=True)
    assert torch.equal(got.detach(), before), f"{c.name}: the backward changed the forward's output"
    w2 = c.check_grads(gpu, req, grads, f"{c.name} replay 2")
    w3 = c.check_grads(gpu, req, first, f"{c.name} replay 2 against 1")
    print(f"\n[glue {c.name}] replays: {w1:.2f}, {w2:.2f}; second against first {w3:.2f} of the limit")
