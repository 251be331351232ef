"""attention_core under the gradient patterns a training step really uses, route by route.

The sweeps (tests/test_gpu_random_sweep_routes.py, _dropout.py, test_gpu_tap_x3.py) give requires_grad to every input and
run one backward with a fresh dense cotangent.  In training the history frames run under torch.no_grad() (the forward-only
branch of _AttnCore.forward: no transposed K, NULL outputs of bevr_kv_project / bevr_pack_kv), the one frame with
gradients has a key source that does not require grad (needs_input_grad[7] False: _kv_source_adjoint without the
feature-map gradient), a fine-tuning run freezes the attention parameters, and `.sum().backward()` hands over a stride-0
cotangent.  Here the sweep's configurations (draw(route, prec, seed), seeds 0 and 1; the tap_pix route in the split-bf16
mode; one attention-dropout case per 16-bit mode on the kv_source + tap split) are run once per pattern against ONE
float64 oracle per configuration (every input requiring grad, cached in the module).

No limit is new.  Forward and gradients are held to what run_case (tests/test_gpu_random_sweep_routes.py) applies to the
route and input -- OUT_LIM / TAP_OUT_LIM, GRAD_LIM (tests/test_gpu_ops.py) / TAP_GRAD_LIM, POS_LIM on the keys away from
kinks with its > 0.5 clean-share condition, the per-term bound (gradient_terms, UNIT) for clustered keys, 2^-8 more for a
gradient stored in bf16 -- and, for the split-bf16 tap_pix route, to the limits of
tests/test_gpu_tap_x3.py::test_attention_core_with_tap_pix_matches_the_oracle (2e-4 forward, 5e-4 / 2.5e-4 gradients,
check_keys at 1e-3 for d(pos)).  Every case asserts the kernels that ran (ops.KERNEL_TIMER).

Then, on one configuration per route family (kv_cell, kv_source, tap) in BF16 and F16: the cotangent as a non-contiguous
view and with stride 0, the all-zero cotangent (finite, exactly zero gradients), and backward(retain_graph=True) twice.
Last, _TapAttn with a cotangent on its LSE output alone (dRn None), which attention_core never produces itself."""
import pytest
import torch
import torch.nn.functional as F

from bevrender_amd import _lib, ops
from test_gpu_dropout import _oracle_core_drop, drop_mult
from test_gpu_fullsize import kink_distance
from test_gpu_ops import GRAD_LIM, _oracle_core, rel_err
from test_gpu_random_sweep_routes import (MODE_NAME, OUT_LIM, POS_LIM, ROUTE_MODES, TAP_GRAD_LIM, TAP_OUT_LIM, UNIT, chain_kv,
                                          draw, gradient_terms, make, pixel_kink_distance)
from test_gpu_tap_x3 import check_keys, pos_kink_distance

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, X3, BF16, F16 = _lib.PREC_F32, _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16
DROP_P = 0.3

# every launch that computes attention (the prep kernels run on every route)
ATTN = {"bevr_attn_fwd", "bevr_attn_gather_fwd", "bevr_attn_gather_fwd_rows", "bevr_attn_cell_fwd", "bevr_attn_tap_fwd",
        "bevr_attn_bwd_q", "bevr_attn_slab_bwd_q", "bevr_attn_bwd_k", "bevr_attn_cell_bwd_q", "bevr_attn_cell_bwd_k",
        "bevr_attn_tap_bwd_q", "bevr_attn_tap_bwd_k"}
ATTN |= {k + "_dropout" for k in ("bevr_attn_fwd", "bevr_attn_bwd_q", "bevr_attn_bwd_k", "bevr_attn_tap_fwd",
                                  "bevr_attn_tap_bwd_q", "bevr_attn_tap_bwd_k")}

CASES = {}
for _route, _prec in ROUTE_MODES:
    for _seed in (0, 1):
        CASES[f"{_route}-{MODE_NAME[_prec]}-{_seed}"] = dict(kind="route", route=_route, prec=_prec, seed=_seed)
# the tap_pix route (split-bf16): the bf16 tap draws at seeds 0 and 1 (both leave a region segment, whose projected rows
# the route takes), float feature map as tests/test_gpu_tap_x3.py builds it
for _seed in (0, 1):
    CASES[f"tap_pix-bf16x3-{_seed}"] = dict(kind="tap_pix", route="tap", prec=X3, seed=_seed)
# attention dropout on the kv_source + tap split: the first of seeds 0, 1 whose draw leaves a region segment (with
# dropout the tap split is kept only then: ops.attention_core)
CASES["tap_drop-bf16-0"] = dict(kind="drop", route="tap", prec=BF16, seed=0)
CASES["tap_drop-f16-1"] = dict(kind="drop", route="tap", prec=F16, seed=1)

FUSED = ("query", "feat", "Wkv", "bkv", "pos", "table")
ROWS = ("query", "k", "v", "pos", "table")
NONE, NO_GRAD = "none", "no_grad"          # nothing requires grad (grad mode on); the call under torch.no_grad()
PATTERNS = {
    True: {"all_but_feat": set(FUSED) - {"feat"},           # the last frame: the history carries no gradient
           "query+feat": {"query", "feat"},                   # frozen attention parameters
           **{f"only_{n}": {n} for n in FUSED}, NONE: set(), NO_GRAD: set(FUSED)},
    False: {"query+table": {"query", "table"}, "k+v": {"k", "v"},
            **{f"only_{n}": {n} for n in ROWS}, NONE: set(), NO_GRAD: set(ROWS)},
}
ITEMS = [(cid, pat) for cid, spec in CASES.items() for pat in PATTERNS[spec["route"] in ("kv_source", "tap")]]
# one configuration per route family and 16-bit mode for the cotangent forms, the zero cotangent and the replay
# (kv_cell: both draws have a region and a cell segment; kv_source: all-cell with channel groups and a bf16 map, and
# all-region at S = 40; tap: both merge a region segment with the tap segment)
FAMILY = ["kv_cell-bf16-1", "kv_cell-f16-1", "kv_source-bf16-0", "kv_source-f16-0", "tap-bf16-0", "tap-f16-1"]

_PROBLEMS = {}
WORST = {}


def teardown_module(module):
    print("\n[grad patterns] worst error / its limit, per mode:",
          {k: f"{v:.2f}" for k, v in sorted(WORST.items())})


class Problem:
    """One configuration: CPU inputs, the float64 oracle's output and gradients (every input requiring grad)."""

    def __init__(self, cid):
        spec = CASES[cid]
        self.cid, self.kind, self.route, self.prec = cid, spec["kind"], spec["route"], spec["prec"]
        if self.kind == "tap_pix":
            cfg = dict(draw("tap", BF16, spec["seed"]), prec=X3, feat_bf16=False, cs=1.0)
        else:
            cfg = draw(self.route, self.prec, spec["seed"])
        self.cfg = cfg
        B, V, h, g, S, N = (cfg[k] for k in ("B", "V", "h", "g", "S", "N"))
        self.Wt = 2 * S * cfg["D"] - 1
        seed = 2000 + 97 * spec["seed"] + self.prec              # test_route_random_configuration's data seed
        self.ins = make(cfg, seed)
        self.names = list(self.ins)
        self.fused = "feat" in self.ins
        assert 0 < cfg["split"] < N or self.kind == "route", cfg
        self.keep, self.drop = None, None
        if self.kind == "drop":
            self.drop = (DROP_P, 0x9e000000 + seed)
            self.keep = drop_mult(self.drop[1], DROP_P, B * V * h, S, N)      # one mask over all N keys
        cpu = {n: t.clone().double().requires_grad_(True) for n, t in self.ins.items()}
        if self.fused:
            k64, v64 = chain_kv(cpu["feat"], cpu["Wkv"], cpu["bkv"], cpu["pos"], g)
        else:
            k64, v64 = cpu["k"], cpu["v"]
        if self.keep is None:
            want = _oracle_core(cpu["query"], k64, v64, cpu["pos"], cpu["table"], h, g, V)        # (B V, M, C)
        else:
            want = _oracle_core_drop(cpu["query"], k64, v64, cpu["pos"], cpu["table"], h, g, V, self.keep)
        self.cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64) * cfg["cs"]
        leaves = [cpu[n] for n in self.names]
        family = cid in FAMILY
        self.grads = dict(zip(self.names, torch.autograd.grad(want, leaves, self.cot, retain_graph=family)))
        # the gradients of out.sum(): what a stride-0 cotangent must give
        self.grads_sum = dict(zip(self.names, torch.autograd.grad(want, leaves, torch.ones_like(want)))) if family else None
        self.want = want.detach()
        self.term_ins = [t.detach() for t in (cpu["query"], k64, v64, cpu["pos"], cpu["table"])]
        self._terms = {}
        # run_case's kink mask of d(pos)
        self.clean = kink_distance(self.ins["pos"], S, self.Wt) >= 1e-4
        if self.fused:
            Hi, Wi = self.ins["feat"].shape[1:3]
            self.clean &= pixel_kink_distance(self.ins["pos"], Hi, Wi) >= 1e-4
            self.x3_dist = pos_kink_distance(self.ins["pos"], S, self.Wt, Hi, Wi)

    def terms(self, cot, key):
        if key not in self._terms:
            c = self.cfg
            self._terms[key] = gradient_terms(self.term_ins, cot, c["h"], c["g"], c["V"], keep=self.keep)
        return self._terms[key]

    # ---- the device call, as the route's test makes it ----
    def call(self, gpu):
        c = self.cfg
        kw = dict(heads=c["h"], groups=c["g"], views=c["V"], precision=self.prec, concat_views=c["concat"])
        if self.route in ("kv_cell", "kv_source") and c["split"] < c["N"] or self.route == "tap":
            kw["cell_split"] = c["split"]
        if self.drop:
            kw["attn_drop"] = self.drop
        if self.kind == "tap_pix":      # tests/test_gpu_tap_x3.py run_route: only the scattered keys are sampled and projected
            xs = ops.sample_features(gpu["feat"].permute(0, 3, 1, 2), gpu["pos"][:, :c["split"]].contiguous(), 1)
            got = ops.attention_core(gpu["query"], None, None, gpu["pos"], gpu["table"], kv=F.linear(xs, gpu["Wkv"], gpu["bkv"]),
                                     tap_source=True, tap_pix=(gpu["feat"], gpu["Wkv"], gpu["bkv"]), **kw)
        elif self.fused:
            got = ops.attention_core(gpu["query"], None, None, gpu["pos"], gpu["table"],
                                     kv_source=(gpu["feat"], gpu["Wkv"], gpu["bkv"]), tap_source=self.route == "tap", **kw)
        else:
            got = ops.attention_core(gpu["query"], gpu["k"], gpu["v"], gpu["pos"], gpu["table"], **kw)
        if c["concat"]:       # (B, M, V C) -> (B V, M, C), the oracle's layout
            B, V, C, M = c["B"], c["V"], c["C"], c["S"] ** 2
            assert got.shape == (B, M, V * C)
            return got.reshape(B, M, V, C).permute(0, 2, 1, 3).reshape(B * V, M, C)
        return got

    def leaves(self, requires):
        return {n: t.clone().to(DEV).requires_grad_(n in requires) for n, t in self.ins.items()}

    # ---- the kernels of the route ----
    def kernels(self):
        """(forward, backward) attention launches the route must run, and the operand kernel of its region / cell keys."""
        c = self.cfg
        S, N, split = c["S"], c["N"], c["split"]
        tap = self.route == "tap"
        region, cell = split > 0, split < N and not tap
        sfx = "_dropout" if self.drop else ""
        fwd, bwd = set(), set()
        if tap:
            fwd.add("bevr_attn_tap_fwd" + sfx)
            bwd |= {"bevr_attn_tap_bwd_q" + sfx, "bevr_attn_tap_bwd_k" + sfx}
        if cell:
            fwd.add("bevr_attn_cell_fwd")
            bwd |= {"bevr_attn_cell_bwd_q", "bevr_attn_cell_bwd_k"}
        if region and self.drop:
            fwd.add("bevr_attn_fwd_dropout")
            bwd |= {"bevr_attn_bwd_q_dropout", "bevr_attn_bwd_k_dropout"}
        elif region:
            fwd.add("bevr_attn_gather_fwd" if ops.gather_supported(self.prec, S) else "bevr_attn_fwd")
            bwd |= {"bevr_attn_slab_bwd_q" if ops.slab_supported(self.prec, S, self.Wt) else "bevr_attn_bwd_q", "bevr_attn_bwd_k"}
        # (bevr_pack_kv, the explicit rows' operand kernel, is not a timed launch: the timer does not see it)
        operands = "bevr_kv_project" if (region or cell) and self.fused and self.kind != "tap_pix" else None
        return fwd, bwd, operands

    def check_kernels(self, used, backward, tag, requires=()):
        fwd, bwd, operands = self.kernels()
        if set(requires) == {"bkv"}:
            # the tap kernels see the biases only through Gb, a per-row shift added to their LSE OUTSIDE them (and bv after
            # them): with no other gradient wanted nothing flows into _TapAttn and its backward must not run
            bwd = {k for k in bwd if "_tap_" not in k}
        want = fwd | (bwd if backward else set())
        assert used & ATTN == want, f"{tag}: attention kernels {sorted(used & ATTN)}, the route's are {sorted(want)}"
        assert operands is None or operands in used, f"{tag}: {operands} did not run ({sorted(used)})"
        if not backward:
            back = sorted(k for k in used if "_bwd" in k or k == "bevr_unpack_dkv")
            assert not back, f"{tag}: backward kernels ran in a forward-only call: {back}"

    # ---- numbers ----
    def note(self, what, ratio):
        key = f"{MODE_NAME[self.prec]} {what}"
        WORST[key] = max(WORST.get(key, 0.0), ratio)

    def check_out(self, got, tag):
        e = rel_err(got.detach().cpu().double(), self.want)
        lim = 2e-4 if self.kind == "tap_pix" else (TAP_OUT_LIM if self.route == "tap" else OUT_LIM)[self.prec]
        self.note("out", e / lim)
        assert e < lim, f"{tag}: out {e:.3e} (limit {lim:.1e})"
        return e

    def grad_error(self, n, a, b, cot, cot_key, cs, tag):
        """error / limit of one gradient `a` against `b` under run_case's rule for input n (tap_pix: test_gpu_tap_x3's)."""
        a = a.detach().cpu().double()
        assert torch.isfinite(a).all(), f"{tag}: grad {n} not finite"
        cfg, prec = self.cfg, self.prec
        if self.kind == "tap_pix":
            if n == "pos":
                check_keys(f"{tag} d(pos)", a, b, self.x3_dist, 1e-3)
                return 0.0
            e = (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)
            return e / (2.5e-4 if n == "table" else 5e-4)
        tap = self.route == "tap"
        lim_g = TAP_GRAD_LIM[prec] if tap else GRAD_LIM[prec]
        if n == "pos":
            assert self.clean.float().mean().item() > 0.5, f"{tag}: kink neighbourhood too wide for this case"
            dg, dw = a[self.clean], b[self.clean]
            ep = (dg - dw).norm().item() / max(dw.norm().item(), 2e-2 * cs * max(dw.numel(), 1) ** 0.5)
            return ep / POS_LIM[prec]
        scale = max(b.abs().max().item(), 2e-2 * cs)
        if n in ("table", "query") and (tap or cfg["kind"] == 2) and cot is not None:
            bound = 2.0 * UNIT[prec] * self.terms(cot, cot_key)[n == "query"] + lim_g * scale
            return ((a - b).abs() / bound).max().item()
        e = (a - b).abs().max().item() / scale
        return e / (lim_g + (2.0 ** -8 if n == "feat" and cfg["feat_bf16"] else 0.0))

    def check_grads(self, gpu, requested, tag, ref=None, cot=None, cot_key="cot", cs=None):
        ref = self.grads if ref is None else ref
        cot = self.cot if cot is None else cot
        cs = self.cfg["cs"] if cs is None else cs
        line = []
        for n in self.names:
            g = gpu[n].grad
            if n not in requested:
                assert g is None, f"{tag}: {n} does not require grad and got one"
                continue
            assert g is not None, f"{tag}: no gradient for {n}"
            r = self.grad_error(n, g, ref[n], cot, cot_key, cs, tag)
            self.note(f"grad {n}", r)
            line.append((n, r))
        print(f"[{tag}] error / limit: " + " ".join(f"{n} {r:.2f}" for n, r in line))
        for n, r in line:
            assert r < 1.0, f"{tag}: grad {n} at {r:.2f} x its limit"


def problem(cid):
    if cid not in _PROBLEMS:
        _PROBLEMS[cid] = Problem(cid)
    return _PROBLEMS[cid]


@pytest.mark.parametrize("cid,pattern", ITEMS, ids=[f"{c}-{p}" for c, p in ITEMS])
def test_attention_core_gradient_pattern(cid, pattern, monkeypatch):
    if CASES[cid]["kind"] == "tap_pix":
        monkeypatch.setenv("BEVR_TAP_X3", "1")
    p = problem(cid)
    requires = PATTERNS[p.fused][pattern]
    tag = f"{cid} {pattern}"
    gpu = p.leaves(requires)
    backward = pattern not in (NONE, NO_GRAD)
    ops.KERNEL_TIMER.start()
    try:
        if pattern == NO_GRAD:
            with torch.no_grad():
                got = p.call(gpu)
        else:
            got = p.call(gpu)
        assert got.requires_grad == backward, tag
        if backward:
            got.backward(p.cot.float().to(DEV))
    finally:
        used = set(ops.KERNEL_TIMER.stop())
    p.check_kernels(used, backward, tag, requires)
    e = p.check_out(got, tag)
    print(f"\n[{tag}] out {e:.3e}")
    p.check_grads(gpu, requires if backward else set(), tag)


def _family_run(cid):
    p = problem(cid)
    gpu = p.leaves(set(p.names))
    return p, gpu, p.call(gpu)


@pytest.mark.parametrize("cid", FAMILY)
def test_cotangent_as_a_non_contiguous_view_and_with_stride_zero(cid):
    """Every backward calls .contiguous() on what it is handed: the dense cotangent as a channel slice of a wider buffer
    gives the gradients of the dense one (same limits), and out.sum().backward() (an expanded scalar, stride 0) gives the
    oracle's sum() gradients."""
    p, gpu, got = _family_run(cid)
    wide = torch.zeros(*got.shape[:-1], got.shape[-1] + 5, device=DEV)
    view = wide[..., 2:2 + got.shape[-1]]
    view.copy_(p.cot.float())
    assert not view.is_contiguous()
    got.backward(view)
    p.check_grads(gpu, set(p.names), f"{cid} sliced cotangent")
    p, gpu, got = _family_run(cid)
    got.sum().backward()
    p.check_grads(gpu, set(p.names), f"{cid} sum()", ref=p.grads_sum, cot=torch.ones_like(p.cot), cot_key="ones", cs=1.0)


@pytest.mark.parametrize("cid", FAMILY)
def test_zero_cotangent_gives_finite_exactly_zero_gradients(cid):
    """The backward's scales are log2 of a bound clamped at 1e-30 (fixed-point unit, fp16's power-of-two cotangent
    scale): with an all-zero cotangent nothing may overflow into inf * 0."""
    p, gpu, got = _family_run(cid)
    got.backward(torch.zeros_like(got))
    for n in p.names:
        g = gpu[n].grad
        assert g is not None, f"{cid}: no gradient for {n}"
        assert torch.isfinite(g).all(), f"{cid}: grad {n} not finite under a zero cotangent"
        assert not g.ne(0).any(), f"{cid}: grad {n} max |.| {g.abs().max().item():.3e} under a zero cotangent"


@pytest.mark.parametrize("cid", FAMILY)
def test_backward_replayed_on_one_graph(cid):
    """backward(retain_graph=True) twice: a backward that wrote into what the forward saved (O, LSE, the key workspace,
    the packed operands) would change the second replay or the output.  The float atomics' order forbids bit equality of
    the gradients: both replays meet the oracle's limits and the second meets them against the first."""
    p, gpu, got = _family_run(cid)
    cot = p.cot.float().to(DEV)
    before = got.detach().clone()
    got.backward(cot, retain_graph=True)
    p.check_grads(gpu, set(p.names), f"{cid} replay 1")
    first = {n: gpu[n].grad.detach().cpu().double() for n in p.names}
    for t in gpu.values():
        t.grad = None
    got.backward(cot, retain_graph=True)
    assert torch.equal(got.detach(), before), f"{cid}: the backward changed the forward's output"
    p.check_grads(gpu, set(p.names), f"{cid} replay 2")
    p.check_grads(gpu, set(p.names), f"{cid} replay 2 against 1", ref=first)


# ---------------------------------------------------------------------------------------------------------------------
# _TapAttn with a cotangent on its LSE alone (dRn is None: set_materialize_grads(False))
# ---------------------------------------------------------------------------------------------------------------------
def _tap_segment_lse(p, gpu):
    """The tap segment of attention_core's tap route up to _TapAttn, operands formed as ops.attention_core forms them;
    returns the segment's log2-sum-exp WITHOUT the key bias' share Gb, (B', h, M) in the oracle's row order."""
    c = p.cfg
    S, N, n, h, V, Cc = c["S"], c["N"], c["split"], c["h"], c["V"], c["C"]
    cc = Cc // h
    feat, pos = gpu["feat"], gpu["pos"]
    Bp = feat.shape[0]
    B = Bp // V
    route = ops.attention_route(p.prec, 1, S, p.Wt, N, n, True, False, "kv_source", Cc, h)
    geom = ops.AttnGeom(n_prob=Bp, q_div=V, heads=h, groups=1, S=S, N=N - n, Wt=p.Wt, precision=p.prec)
    Qp = ops.pack_query(gpu["query"].float(), h)
    a, b = ops.key_coords(pos.float(), S, p.Wt, N)
    Tt = ops.pack_table(gpu["table"].float(), geom)
    fpix = feat[:, :ops.TAP_R, :ops.TAP_C, :].float()
    fpix = F.pad(fpix, (0, 0, 0, ops.TAP_C - fpix.shape[2], 0, ops.TAP_R - fpix.shape[1])).reshape(Bp, ops.TAP_N, Cc)
    kp = F.linear(fpix, gpu["Wkv"].float()[:Cc])
    Kp = F.pad(kp.reshape(B, V, ops.TAP_N, h, cc), (0, ops.HEAD_DIM - cc)).permute(0, 3, 4, 1, 2).reshape(B, h, ops.HEAD_DIM, V * ops.TAP_N)
    G = torch.matmul(Qp, Kp).reshape(B, h, geom.Mp, V, ops.TAP_N).permute(0, 3, 1, 2, 4).reshape(Bp, h, geom.Mp, ops.TAP_N)
    key_y = (pos[:, n:, 0].float() + 1.0) * (0.5 * (feat.shape[1] - 1))
    key_x = (pos[:, n:, 1].float() + 1.0) * (0.5 * (feat.shape[2] - 1))
    Rn, LSE = ops._TapAttn.apply(G, a[:, n:], b[:, n:], key_y, key_x, Tt, geom, route.segments[-1], None)
    assert Rn.requires_grad and LSE.requires_grad
    return LSE.reshape(Bp, h, S, geom.Sp)[..., :S].transpose(2, 3).reshape(Bp, h, S * S)


def _tap_segment_lse_oracle(p, cpu):
    """log2 sum_n 2^(log2(e) (c^-0.5 q . (K_n - bk) + bias)) over the tap keys in float64 (gradient_terms' logits)."""
    from oracle import bevrender_oracle as O
    c = p.cfg
    S, n, h, V, Cc = c["S"], c["split"], c["h"], c["V"], c["C"]
    cc, M = Cc // h, S * S
    pos = cpu["pos"][:, n:]
    Nt = pos.shape[1]
    xs = F.grid_sample(cpu["feat"].permute(0, 3, 1, 2), pos[:, None, :, (1, 0)], mode="bilinear", padding_mode="zeros",
                       align_corners=True)[:, :, 0].permute(0, 2, 1)
    kk = F.linear(xs, cpu["Wkv"][:Cc])
    q_grid = O.normalized_grid(S, S, torch.float64).reshape(1, M, 2)
    tab = cpu["table"]
    out = []
    for bp in range(pos.shape[0]):
        q = cpu["query"][bp // V].reshape(h, cc, M)
        kh = kk[bp].reshape(Nt, h, cc).permute(1, 2, 0)
        disp = (q_grid.unsqueeze(2) - pos[bp:bp + 1].reshape(1, 1, Nt, 2)) * 0.5
        bias = F.grid_sample(tab.reshape(1, h, *tab.shape[-2:]), disp[..., (1, 0)], mode="bilinear",
                             align_corners=True).reshape(h, M, Nt)
        out.append(torch.logsumexp(torch.einsum("bcm,bcn->bmn", q, kh) * cc ** -0.5 + bias, 2) * ops.LOG2E)
    return torch.stack(out, 0)


@pytest.mark.parametrize("cid", ["tap-bf16-0", "tap-f16-1"])
def test_tap_segment_with_a_cotangent_on_its_lse_alone(cid):
    """_TapAttn.backward with dRn None: only the LSE carries a cotangent (what the merge hands back where the tap half's
    weight vanishes).  attention_core always sends both, so the Function is called as attention_core calls it.  Forward:
    the LSE limit of tests/test_gpu_tap.py's entry-point test, 10 x (4e-3 bf16, 1e-3 fp16) in log2 units; gradients:
    run_case's rules for the tap route (TAP_GRAD_LIM of the largest entry, floor 2e-2 cs; d(pos) POS_LIM in the 2-norm over
    the tap keys away from kinks; 2^-8 more for a gradient stored in bf16)."""
    p = problem(cid)
    c, prec = p.cfg, p.prec
    n, cs = c["split"], c["cs"]
    names = ["query", "feat", "Wkv", "pos", "table"]
    cpu = {k: p.ins[k].clone().double().requires_grad_(True) for k in names}
    want = _tap_segment_lse_oracle(p, cpu)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(11), dtype=torch.float64) * cs
    ref = dict(zip(names, torch.autograd.grad(want, [cpu[k] for k in names], cot)))
    gpu = {k: p.ins[k].clone().to(DEV).requires_grad_(True) for k in names}
    ops.KERNEL_TIMER.start()
    try:
        got = _tap_segment_lse(p, gpu)
        got.backward(cot.float().to(DEV))
    finally:
        used = set(ops.KERNEL_TIMER.stop())
    assert used & ATTN == {"bevr_attn_tap_fwd", "bevr_attn_tap_bwd_q", "bevr_attn_tap_bwd_k"}, sorted(used)
    e = (got.detach().cpu().double() - want.detach()).abs().max().item()
    lim_f = 10 * (1e-3 if prec == F16 else 4e-3)
    line = [f"LSE {e:.3e} (limit {lim_f:.0e})"]
    assert e < lim_f, line
    for k in names:
        a, b = gpu[k].grad.cpu().double(), ref[k]
        assert torch.isfinite(a).all(), k
        if k == "pos":
            assert not a[:, :n].ne(0).any(), "a key outside the segment got a gradient"
            clean = p.clean[:, n:]
            assert clean.float().mean().item() > 0.5
            dg, dw = a[:, n:][clean], b[:, n:][clean]
            r = (dg - dw).norm().item() / max(dw.norm().item(), 2e-2 * cs * max(dw.numel(), 1) ** 0.5) / POS_LIM[prec]
        else:
            lim = TAP_GRAD_LIM[prec] + (2.0 ** -8 if k == "feat" and c["feat_bf16"] else 0.0)
            r = (a - b).abs().max().item() / max(b.abs().max().item(), 2e-2 * cs) / lim
        p.note(f"grad {k} (LSE alone)", r)
        line.append(f"{k} {r:.2f}")
    print(f"\n[{cid} cotangent on the LSE alone] " + ", gradients error / limit: ".join([line[0], " ".join(line[1:])]))
    assert all(float(s.split()[1]) < 1.0 for s in line[1:]), line
