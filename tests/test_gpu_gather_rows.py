"""The gather forward over row ranges and in fp16 (csrc/attn_gather_fwd.hip, bevr_attn_gather_fwd_rows): BEV sides above
224 as bands of rows, fp16 operands with a softmax reference that works in 5 exponent bits.  Through the C ABI -- on
the operands ops.attention_core packs, picked up at its own gather launch -- and through ops.attention_core, against the
float64 oracle (oracle/bevrender_oracle.py: attention_core, the reference's model/SCA_deform_attn.py:331-413).

Every test prints its figures before it asserts (-s); the recorded run is profiles/r06_gather_rows.txt."""
import ctypes as C
import os

import pytest
import torch

from bevrender_amd import _lib, ops
from test_gpu_fullsize import LIMITS, check_dpos, oracle_rows, pick_rows
from test_gpu_fullsize import rel_err as rel_err_rows
from test_gpu_gather import CASES, LIM_OUT, _problem
from test_gpu_ops import GRAD_LIM, _oracle_core, rel_err
from test_gpu_random_sweep_routes import OUT_LIM

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = _lib.PREC_BF16, _lib.PREC_F16
TAG = {BF16: "bf16", F16: "f16"}
SENT = 12345.0          # what the test writes where a launch must not


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class GatherProbe:
    """Stands in for ops.KERNEL_TIMER.run during ops.attention_core: at the gather launch it hands the launch's operands
    (live device buffers: descriptor, Q, K, V, key workspace, pair table, mref) to `probe`, which calls the C ABI on them
    with outputs of its own; then the launch goes ahead."""

    def __init__(self, probe=None):
        self.probe, self.names = probe, []

    def __call__(self, name, flops, fn, *args, nbytes=0.0, tag=""):
        self.names.append(name)
        if name == "bevr_attn_gather_fwd" and self.probe is not None:
            probe, self.probe = self.probe, None          # the first gather launch of the call
            probe(args[0], args[1:7], args[-1])
        return fn(*args)


class Outputs:
    """O, both LSE planes and the flags of one C-ABI call sequence, sentinel-filled."""

    def __init__(self, d):
        self.d = d
        self.Mp = d.S * d.Sp
        self.O = torch.full((d.n_prob, d.heads, self.Mp, 32), SENT, device=DEV)
        self.LSE = torch.full((2, d.n_prob, d.heads, self.Mp), SENT, device=DEV)
        self.flags = torch.zeros(d.n_prob * d.heads, d.S, device=DEV, dtype=torch.int32)
        self.flagged = torch.zeros_like(self.flags)

    def whole(self, dref, opnds, stream):
        self.flags.zero_()
        _lib.check(_lib.lib().bevr_attn_gather_fwd(dref, *opnds, _ptr(self.O), _ptr(self.LSE), _ptr(self.flags), stream),
                   "bevr_attn_gather_fwd")
        self.flagged |= self.flags
        return self

    def rows(self, dref, opnds, stream, row0, n_rows):
        self.flags.zero_()
        _lib.check(_lib.lib().bevr_attn_gather_fwd_rows(dref, *opnds, _ptr(self.O), _ptr(self.LSE), _ptr(self.flags),
                                                        row0, n_rows, stream), "bevr_attn_gather_fwd_rows")
        self.flagged |= self.flags
        return self

    def by_row(self):
        """O (P, h, j, i, 32) and LSE (2, P, h, j, i): i the BEV row of column j, padding rows included."""
        d = self.d
        return (self.O.reshape(d.n_prob, d.heads, d.S, d.Sp, 32), self.LSE.reshape(2, d.n_prob, d.heads, d.S, d.Sp))

    def out(self, c):
        return ops.unpack_out(self.O, self.d.S, c).cpu().double()


def run_core(ins, h, V, prec, monkeypatch, probe=None, backward_cot=None):
    """ops.attention_core on device copies of `ins` with the probe at the gather launch; returns (out, device inputs,
    names of the kernels that ran)."""
    dev = [t.clone().to(DEV).requires_grad_(backward_cot is not None) for t in ins]
    spy = GatherProbe(probe)
    with monkeypatch.context() as m:
        m.setattr(ops.KERNEL_TIMER, "run", spy)
        out = ops.attention_core(*dev, heads=h, groups=1, views=V, precision=prec)
        if backward_cot is not None:
            out.backward(backward_cot)
        torch.cuda.synchronize()
    return out, dev, spy.names


def tile_permutation(N):
    """keys reversed inside every 32-key tile: the same tiles, the same tap boxes, another summation order"""
    idx = torch.arange(N)
    return torch.cat([idx[t:t + 32].flip(0) for t in range(0, N, 32)])


def kd_sorted(u):
    """4 000 keys on a 399 x 399 table in the k-d order of the modules: a 32-key leaf spans ~25 x 50 table cells, so many
    tiles whose window does not hold 208 BEV rows (per-key strips in the whole column) hold a band's 112 or 88"""
    pos = (u * 2 - 1) * 0.9
    order = torch.from_numpy(ops.kd_key_order(pos[0].double().numpy(), 200, 399))
    return pos[:, order].contiguous()


BAND_CASES = [
    # S, split, problem (B, V, C, h, S, D, N), key positions: the first two are CASES[0] / CASES[1] of test_gpu_gather.py
    (21, 16, CASES[0][1], CASES[0][2]),
    (40, 16, CASES[1][1], CASES[1][2]),
    (200, 112, (1, 1, 64, 2, 200, 5, 1500), lambda u: (u * 2 - 1) * 0.9),
    (200, 112, (1, 1, 64, 2, 200, 1, 4000), kd_sorted),
]


@pytest.mark.parametrize("S,split,cfg,pos_fn", BAND_CASES, ids=["S21", "S40", "S200", "S200-kd-leaves"])
def test_bands_reproduce_the_column(S, split, cfg, pos_fn, monkeypatch):
    """bf16: the row-range entry point over [0, S) -- as one band, and as two bands split at a multiple of 16 -- against
    bevr_attn_gather_fwd on the same operands: O, LSE plane 0 (plane 1 too) and the padding rows; rows outside a band keep
    the sentinel.  A band's windows hold fewer rows, so its `fits` decisions (window or per-key strips) can differ from the
    whole column's: the two may differ by summation order, for which no constant can be derived here.  The yardstick is
    the whole-column entry point against ITSELF with the keys permuted inside their tiles (the parent's kernel); the
    banded result may differ from the whole-column one by at most twice that spread.
    Measured on MI355X (max |dO| / max |O|; max |dLSE0| in binades; printed with -s, profiles/r06_gather_rows.txt):
        case             spread O   spread LSE0   one band O / LSE0   two bands O / LSE0
        S21              2.05e-07   0             0 / 0               0 / 0
        S40              3.80e-07   0             0 / 0               0 / 0
        S200             5.94e-07   3.81e-06      0 / 0               0 / 0
        S200-kd-leaves   5.36e-07   7.63e-06      0 / 0               0 / 0
    i.e. the banded results were bit-identical to the whole column's in all four, inside the allowed 2 x spread.
    Each side on its own meets test_gpu_gather.py's LIM_OUT against the float64 oracle (S = 200: on sampled rows)."""
    B, V, Cc, h, S_, D, N = cfg
    assert S_ == S
    c = Cc // h
    ins = _problem(B, V, Cc, h, S, D, N, 500 + N, pos_fn)
    got = {}

    def probe_all(dref, opnds, stream):
        d = dref._obj
        got["whole"] = Outputs(d).whole(dref, opnds, stream)
        got["one"] = Outputs(d).rows(dref, opnds, stream, 0, S)
        first = Outputs(d).rows(dref, opnds, stream, 0, split)
        got["first"] = (first.O.clone(), first.LSE.clone())
        got["two"] = first.rows(dref, opnds, stream, split, S - split)
        got["second"] = Outputs(d).rows(dref, opnds, stream, split, S - split)

    def probe_perm(dref, opnds, stream):
        got["perm"] = Outputs(dref._obj).whole(dref, opnds, stream)

    run_core(ins, h, V, BF16, monkeypatch, probe_all)
    perm = tile_permutation(N)
    ins_p = (ins[0], ins[1][:, perm], ins[2][:, perm], ins[3][:, perm], ins[4])
    run_core(ins_p, h, V, BF16, monkeypatch, probe_perm)
    assert set(got) == {"whole", "one", "first", "two", "second", "perm"}, "the gather launch was not reached"

    whole = got["whole"]
    Ow, Lw = whole.by_row()
    nblk = (S + 15) // 16
    assert torch.isfinite(Lw).all(), "LSE of the padding rows must be finite"
    assert (Ow[..., nblk * 16:, :] == SENT).all()          # rows no block covers: O untouched
    scale = Ow[..., :S, :].abs().max().item()

    def diff(a, b):
        Oa, La = a.by_row()
        Ob, Lb = b.by_row()
        return ((Oa - Ob).abs().max().item() / scale, (La[0] - Lb[0]).abs().max().item(), (La[1] - Lb[1]).abs().max().item())

    spread = diff(got["perm"], whole)
    print(f"\n[bands S={S}] spread of the whole-column entry point under a key permutation inside tiles: "
          f"O {spread[0]:.3e}  LSE0 {spread[1]:.3e}  LSE1 {spread[2]:.3e}")
    # rows outside a band keep the sentinel: O and both LSE planes, padding rows included
    O1, L1 = (t.reshape(*s) for t, s in zip(got["first"], (Ow.shape, Lw.shape)))
    assert (O1[..., split:, :] == SENT).all() and (L1[..., split:] == SENT).all(), "the first band wrote past its rows"
    assert (O1[..., :split, :] != SENT).any()
    O2, L2 = got["second"].by_row()
    assert (O2[..., :split, :] == SENT).all() and (L2[..., :split] == SENT).all(), "the second band wrote before its rows"
    assert not got["whole"].flagged.any() and not got["two"].flagged.any()
    for name in ("one", "two"):
        e = diff(got[name], whole)
        print(f"[bands S={S}] {name} band(s) against the whole column: O {e[0]:.3e}  LSE0 {e[1]:.3e}  LSE1 {e[2]:.3e}")
        for k, what in enumerate(("O", "LSE plane 0", "LSE plane 1")):
            assert e[k] <= 2.0 * spread[k], f"{name}: {what} differs by {e[k]:.3e}, spread {spread[k]:.3e}"
        # the same rows left untouched (sentinel on both sides compares equal above); and finite everywhere else
        Ob, Lb = got[name].by_row()
        assert torch.isfinite(Lb).all() and ((Ob == SENT) == (Ow == SENT)).all()

    # each side on its own against the float64 oracle
    if S <= 64:
        want = _oracle_core(*[t.double() for t in ins], h, 1, V)
        for name in ("whole", "one", "two"):
            e = rel_err(got[name].out(c), want)
            print(f"[bands S={S}] {name} against the oracle: {e:.3e}")
            assert e < LIM_OUT, f"{name}: {e:.3e}"
    else:
        rows = torch.unique(torch.cat((pick_rows(S, 64, 3), band_rows(S, [(0, split), (split, S - split)], 9))))
        p = dict(query=ins[0], k=ins[1], v=ins[2], pos=ins[3], table=ins[4])
        want, _ = oracle_rows(p, h, rows, None, want_grads=False)
        for name in ("whole", "one", "two"):
            e = rel_err_rows(got[name].out(c)[:, rows], want)
            print(f"[bands S={S}] {name} against the oracle on {len(rows)} rows: {e:.3e}")
            assert e < LIM_OUT, f"{name}: {e:.3e}"


def band_rows(S, bands, j0):
    """query indices m = i S + j: the first and last BEV row of every band (columns j0 and S - 1 - j0), row S - 1, and
    one row of every 16-row block of column j0"""
    rows = [i * S + j for r0, n in bands for i in (r0, r0 + n - 1) for j in (j0, S - 1 - j0)]
    rows += [(S - 1) * S + j0, (S - 1) * S + S - 1]
    rows += [min(16 * b + (5 * b + 3) % 16, S - 1) * S + j0 for b in range((S + 15) // 16)]
    return torch.tensor(sorted(set(rows)))


@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("S", [225, 256, 400, 448])
def test_tall_grids_rows_and_gradients(S, prec, monkeypatch):
    """S above 224 (two bands), D = 5, 1 500 scattered keys, through ops.attention_core: forward and every gradient on
    sampled rows -- the first and last row of every band, row S - 1, a row of every 16-row block of one column, and random
    ones -- against the float64 oracle at tests/test_gpu_fullsize.py's LIMITS; the gather forward ran, the region
    forward did not."""
    monkeypatch.delenv("BEVR_GATHER", raising=False)
    Cc, h, D, N = 64, 2, 5, 1500
    ins = _problem(1, 1, Cc, h, S, D, N, 900 + S, lambda u: (u * 2 - 1) * 0.9)
    p = dict(query=ins[0], k=ins[1], v=ins[2], pos=ins[3], table=ins[4])
    bands = ops.gather_bands(S)
    assert len(bands) == 2
    must = band_rows(S, bands, 11)
    rows = torch.unique(torch.cat((pick_rows(S, 72, S), must)))
    assert all(int(m) in set(rows.tolist()) for m in must)
    cot = torch.randn(1, len(rows), Cc, generator=torch.Generator().manual_seed(8))
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    want, grads = oracle_rows(p, h, rows, cot)

    dev = {n: p[n].clone().to(DEV).requires_grad_(True) for n in ("query", "k", "v", "pos", "table")}
    ops.KERNEL_TIMER.start()
    out = ops.attention_core(dev["query"], dev["k"], dev["v"], dev["pos"], dev["table"], heads=h, groups=1, views=1,
                             precision=prec)
    cot_full = torch.zeros_like(out)
    cot_full[:, rows.to(DEV)] = cot.to(DEV)
    out.backward(cot_full)
    used = ops.KERNEL_TIMER.stop()
    assert "bevr_attn_gather_fwd" in used and "bevr_attn_fwd" not in used, sorted(used)
    assert used["bevr_attn_gather_fwd"]["n"] == len(bands)
    assert torch.isfinite(out).all()
    lim, tag = LIMITS[prec], f"tall S={S} {TAG[prec]}"
    got_rows = out.detach()[:, rows.to(DEV)].cpu().double()
    per_row = (got_rows - want).abs().amax(-1)[0] / want.abs().max().item()          # every sampled row is compared
    print(f"\n[{tag}] out rel err {per_row.max().item():.3e} (worst row m = {int(rows[per_row.argmax()])})")
    assert per_row.max().item() < lim["out"], f"{tag}: out {per_row.max().item():.3e}"
    for n in ("query", "k", "v", "table"):
        e = rel_err_rows(dev[n].grad.cpu(), grads[n])
        print(f"[{tag}] grad {n:6s} rel err {e:.3e}  (max |want| {grads[n].abs().max().item():.3e})")
        assert e < lim[n], f"{tag}: grad {n}: {e:.3e}"
    check_dpos(dev["pos"].grad, grads["pos"], p["pos"], S, p["table"].shape[-1], lim["pos"], tag,
               cols=(rows % S).tolist(), min_clean=0.3)


@pytest.mark.parametrize("name,cfg,pos_fn", CASES, ids=[c[0] for c in CASES])
def test_gather_cases_in_fp16(name, cfg, pos_fn, monkeypatch):
    """tests/test_gpu_gather.py's cases (windows that fit, strips, a table shorter than a window column, clamped taps,
    one key, 31 / 32 / 33 keys) with fp16 operands, against the float64 oracle at the fp16 limits of
    tests/test_gpu_random_sweep_routes.py."""
    monkeypatch.delenv("BEVR_GATHER", raising=False)
    B, V, Cc, h, S, D, N = cfg
    ins = _problem(B, V, Cc, h, S, D, N, 500 + N, pos_fn)
    ins_cpu = [t.clone().double().requires_grad_(True) for t in ins]
    want = _oracle_core(*ins_cpu, h, 1, V)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(3))
    want.backward(cot.double())
    dev = [t.clone().to(DEV).requires_grad_(True) for t in ins]
    ops.KERNEL_TIMER.start()
    got = ops.attention_core(*dev, heads=h, groups=1, views=V, precision=F16)
    got.backward(cot.to(DEV))
    used = set(ops.KERNEL_TIMER.stop())
    assert "bevr_attn_gather_fwd" in used and "bevr_attn_fwd" not in used, sorted(used)
    e = rel_err(got.detach().cpu().double(), want.detach())
    print(f"\n[fp16 {name}] out rel err {e:.3e}")
    assert e < OUT_LIM[F16], f"{name}: out {e:.3e}"
    if N > 1:
        for n, a, b in zip(("query", "k", "v", "table"), (dev[0], dev[1], dev[2], dev[4]),
                           (ins_cpu[0], ins_cpu[1], ins_cpu[2], ins_cpu[4])):
            e = (a.grad.cpu().double() - b.grad).abs().max().item() / max(b.grad.abs().max().item(), 2e-2)
            print(f"[fp16 {name}] grad {n} {e:.3e}")
            assert e < GRAD_LIM[F16], f"{name}: grad {n} {e:.3e}"


# ---- the fp16 softmax reference ------------------------------------------------------------------------------------
def regime_inputs(kind):
    """One head of 32 channels, S = 12, 150 keys.  The static reference is  1.01 (||Q_q|| max ||K_n|| + max |T2|) + 0.01
    minus the headroom 8 (ops.py), in log2 units with Q scaled by c^-0.5 log2(e).
    benign:    small Q and K: the bound is ~4 binades, every logit within a few binades of it.
    subnormal: Q in channels 0..15, K mostly in channels 16..31 (no product) plus a small live part: the bound sits
               ~25 binades over the row maximum, so the weights against the static reference are 2^-17 and less --
               subnormal in fp16, a HEALTHY row sum, a wrong result.  (Zero table in these two: the logits are Q . K.)
    useless:   test_exact_pass_behind_a_useless_static_bound's construction: huge orthogonal Q and K, the bound thousands
               of binades over the logits, every weight zero."""
    B, V, Cc, h, S, D, N = 1, 1, 32, 1, 12, 2, 150
    gen = torch.Generator().manual_seed({"benign": 21, "subnormal": 22, "useless": 9}[kind])
    table = torch.zeros(h, 2 * S - 1, 2 * S * D - 1)
    if kind == "benign":
        query = torch.randn(B, Cc, S, S, generator=gen) * 0.6
        k = torch.randn(B * V, N, Cc, generator=gen) * 0.6
    else:
        query = torch.zeros(B, Cc, S, S)
        query[:, :16] = torch.randn(B, 16, S, S, generator=gen) * 60.0
        k = torch.zeros(B * V, N, Cc)
        k[..., 16:] = torch.randn(B * V, N, 16, generator=gen) * 60.0
        k[..., :16] = torch.randn(B * V, N, 16, generator=gen) * 0.02
        if kind == "subnormal":      # rows of one norm each: the same bound for every query, ~26 binades
            query = query / query.norm(dim=1, keepdim=True) * 10.4
            k[..., 16:] = k[..., 16:] / k[..., 16:].norm(dim=-1, keepdim=True) * 10.4
            k[..., :16] *= 0.3 / 0.02
    v = torch.randn(B * V, N, Cc, generator=gen)
    pos = (torch.rand(B * V, N, 2, generator=gen) * 2 - 1) * 0.9
    if kind == "useless":
        table = torch.randn(h, 2 * S - 1, 2 * S * D - 1, generator=gen) * 0.3
    return (query, k, v, pos, table), (B, V, Cc, h, S, D, N)


def static_reference_model(ins, headroom=8.0):
    """Host model of the STATIC pass alone for a zero table (logits = Q . K): fp16 operands, weights 2^(s - mref) rounded
    to fp16, float sums.  Returns (out (M, C), largest weight per row, row sums, gap = bound - row maximum in binades)."""
    query, k, v, _, table = ins
    assert not table.any()
    Cc, S = query.shape[1], query.shape[-1]
    q = (query[0].reshape(Cc, S * S).t() * (Cc ** -0.5 * ops.LOG2E)).half().double()          # (M, C), m = i S + j
    kk, vv = k[0].half().double(), v[0].half().double()
    s = q @ kk.t()
    ub = 1.01 * (q.norm(dim=-1) * k[0].double().norm(dim=-1).max()) + 0.01
    w = torch.exp2(s - (ub - headroom)[:, None]).half().double()
    l = w.sum(-1)
    return (w @ vv) / l[:, None], w.amax(-1), l, ub - s.amax(-1)


def test_regime_inputs_are_what_they_claim():
    """On the host (no kernel runs): the three regimes' logits against the static bound, and that a static pass which
    only tests the row sum for health would return the subnormal regime wrong by more than the fp16 limit."""
    for kind in ("benign", "subnormal", "useless"):
        ins, (B, V, Cc, h, S, D, N) = regime_inputs(kind)
        want = _oracle_core(*[t.double() for t in ins], h, 1, V)
        assert torch.isfinite(want).all()
        q = ins[0][0].reshape(Cc, S * S).t().double() * (Cc ** -0.5 * ops.LOG2E)
        s = q @ ins[1][0].double().t()
        assert (s.amax(-1) - s.amin(-1)).max() < 900.0          # no row whose weights all vanish in float64 (2^-1000)
        if kind == "useless":
            continue
        out, pmax, l, gap = static_reference_model(ins)
        e = rel_err(out, want[0])
        thr = N * 2.0 ** -14
        print(f"\n[{kind}] bound - row maximum: {gap.min().item():.1f} .. {gap.max().item():.1f} binades; largest weight "
              f"{pmax.min().item():.2e} .. {pmax.max().item():.2e} (threshold {thr:.2e}); static-only error {e:.3e}")
        assert (l > 7.9e-31).all()          # a healthy mass in both regimes
        if kind == "benign":
            assert gap.max() < 8.0 and (pmax >= thr).all() and e < OUT_LIM[F16]
        else:
            assert gap.min() > 19.0 and gap.max() < 29.0 and (pmax < 2.0 ** -14).all()
            assert e > 2.0 * OUT_LIM[F16], "the subnormal regime does not tell the two flag criteria apart"


@pytest.mark.parametrize("kind", ["benign", "subnormal", "useless"])
def test_fp16_reference_regimes(kind, monkeypatch):
    """fp16 through the C ABI (the flags are read back): benign -- no column flagged; largest weight subnormal against the
    static reference -- every column flagged although every row sum is a healthy number; useless bound -- every column
    flagged; the result finite and within the fp16 limit in all three."""
    monkeypatch.delenv("BEVR_GATHER", raising=False)
    ins, (B, V, Cc, h, S, D, N) = regime_inputs(kind)
    want = _oracle_core(*[t.double() for t in ins], h, 1, V)
    got = {}

    def probe(dref, opnds, stream):
        got["abi"] = Outputs(dref._obj).whole(dref, opnds, stream)
        got["rows"] = Outputs(dref._obj).rows(dref, opnds, stream, 0, S)

    out, _, names = run_core(ins, h, V, F16, monkeypatch, probe)
    assert "bevr_attn_gather_fwd" in names and "bevr_attn_fwd" not in names
    for name in ("abi", "rows"):
        o = got[name]
        n_flag, n_col = int(o.flagged.sum()), o.flagged.numel()
        e = rel_err(o.out(Cc // h), want)
        print(f"\n[fp16 {kind}, {name}] {n_flag} of {n_col} columns flagged; out rel err {e:.3e}")
        assert n_flag == (0 if kind == "benign" else n_col), f"{kind}: {n_flag} of {n_col} columns flagged"
        assert torch.isfinite(o.O[o.O != SENT]).all() and torch.isfinite(o.LSE).all()
        assert e < OUT_LIM[F16], f"{kind} ({name}): {e:.3e}"
    e = rel_err(out.detach().cpu().double(), want)
    assert torch.isfinite(out).all() and e < OUT_LIM[F16], f"{kind} (attention_core): {e:.3e}"


def test_region_route_agrees_at_bev400_fp16(monkeypatch):
    """BEVR_GATHER=0 at S = 400 in fp16 takes the region forward and agrees with the gather route within the fp16 limit."""
    Cc, h, S, D, N = 64, 2, 400, 5, 1500
    ins = _problem(1, 1, Cc, h, S, D, N, 1300, lambda u: (u * 2 - 1) * 0.9)
    outs = {}
    for gather in (True, False):
        monkeypatch.setenv("BEVR_GATHER", "1" if gather else "0")
        dev = [t.clone().to(DEV) for t in ins]
        ops.KERNEL_TIMER.start()
        with torch.no_grad():
            outs[gather] = ops.attention_core(*dev, heads=h, groups=1, views=1, precision=F16)
        used = set(ops.KERNEL_TIMER.stop())
        assert ("bevr_attn_gather_fwd" in used) == gather and ("bevr_attn_fwd" in used) == (not gather), sorted(used)
    e = rel_err(outs[True].cpu().double(), outs[False].cpu().double())
    print(f"\n[S=400 fp16] gather route against region route: {e:.3e}")
    assert torch.isfinite(outs[True]).all() and e < OUT_LIM[F16], e
