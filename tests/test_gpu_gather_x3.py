"""The gather forward in the split-bf16 mode (csrc/attn_gather_fwd_x3.hip, bevr_attn_gather_fwd_x3, BEVR_GATHER_X3=1):
scattered keys at the project's f32 limits (tests/test_gpu_fullsize.py: LIMITS[PREC_BF16X3]), against the float64
oracle (oracle/bevrender_oracle.py: attention_core, the reference's model/SCA_deform_attn.py:331-413) and against the
parent's route for that mode, the region forward bevr_attn_fwd (BEVR_GATHER_X3=0), on the same inputs.

One condition for every case: the switch is set through monkeypatch, and WHICH entry point ran is read off a recorder
around ops._launch (the timer's name is the route's and cannot tell the entry points apart); a case in which
bevr_attn_gather_fwd_x3 did not run fails.  Errors are normalised as tests/test_gpu_gather.py normalises them (output:
max |err| / max |want|; gradients: max |err| / max(max |want|, 2e-2)).  Every case prints the new route's and the
parent route's errors before it asserts (-s).  The inputs of the six CASES, of the exact-pass cases and of the
"table" large-logit case are used as they stand; the "q and k" large-logit case is scaled down to where the region forward
passes (see the test)."""
import ctypes as C
import os

import pytest
import torch

from bevrender_amd import _lib, ops
from test_gpu_fullsize import LIMITS, oracle_rows, pick_rows
from test_gpu_fullsize import rel_err as rel_err_rows
from test_gpu_gather import CASES, _problem
from test_gpu_ops import _oracle_core, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
X3 = _lib.PREC_BF16X3
LIM = LIMITS[X3]          # out 2e-4, query / k / v 5e-4, table 2.5e-4
NAME = "bevr_attn_gather_fwd_x3"
REGION = "bevr_attn_fwd"


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class Recorder:
    """Around ops._launch: the entry points in the order they ran.  probe=True: at every bevr_attn_gather_fwd_x3 launch
    the C entry point is also called on the launch's own operands with outputs and flags of the test's, and the flags
    it leaves (the columns its static pass handed to its exact pass) are kept."""

    def __init__(self, probe=False):
        self.names, self.probe, self.flagged, self.n_col = [], probe, 0, 0
        self.orig = ops._launch

    def __call__(self, entry, *a, **kw):
        self.names.append(entry)
        if entry == NAME and self.probe:
            d = a[0]._obj
            Mp = d.S * d.Sp
            O = torch.zeros(d.n_prob, d.heads, Mp, 32, device=DEV)
            LSE = torch.zeros(2, d.n_prob, d.heads, Mp, device=DEV)
            flags = torch.zeros(d.n_prob * d.heads, d.S, device=DEV, dtype=torch.int32)
            _lib.check(_lib.lib().bevr_attn_gather_fwd_x3(a[0], *a[1:7], _ptr(O), _ptr(LSE), _ptr(flags), *a[10:13]), NAME)
            torch.cuda.synchronize()
            self.flagged += int(flags.sum())
            self.n_col += flags.numel()
        return self.orig(entry, *a, **kw)


def run(ins, h, V, monkeypatch, new, cot=None, probe=False, keep=None):
    """ops.attention_core in split mode on device copies of `ins`, on the new route (BEVR_GATHER_X3=1) or the parent's;
    with `cot` a backward too.  keep: a dict that receives the packed O and LSE of the region segment as the forward
    left them.  Returns (out, device inputs, recorder)."""
    rec = Recorder(probe)
    dev = [t.clone().to(DEV).requires_grad_(cot is not None) for t in ins]
    with monkeypatch.context() as m:
        m.setenv("BEVR_GATHER_X3", "1" if new else "0")
        m.delenv("BEVR_GATHER", raising=False)
        m.setattr(ops, "_launch", rec)
        if keep is not None:
            inner = ops._RUN[NAME]

            def keeping(name, o):
                inner(name, o)
                keep.update(O=o.O.clone(), LSE=o.LSE.clone(), g=o.g)
            m.setitem(ops._RUN, NAME, keeping)
        out = ops.attention_core(*dev, heads=h, groups=1, views=V, precision=X3)
        if cot is not None:
            out.backward(cot.to(DEV))
        torch.cuda.synchronize()
    assert (NAME in rec.names) == new and (REGION in rec.names) == (not new), rec.names
    assert "bevr_attn_gather_fwd" not in rec.names and "bevr_attn_gather_fwd_rows" not in rec.names
    return out, dev, rec


def grad_err(a, b):
    return (a.grad.cpu().double() - b.grad).abs().max().item() / max(b.grad.abs().max().item(), 2e-2)


@pytest.mark.parametrize("name,cfg,pos_fn", CASES, ids=[c[0] for c in CASES])
def test_cases_against_the_oracle_and_the_region_forward(name, cfg, pos_fn, monkeypatch):
    """tests/test_gpu_gather.py's six cases (a window that fits with a ragged last emission, strips with two clusters,
    strips over a 1 599-column table, clamped taps, one key, 31 / 32 / 33 keys): forward and the query, k, v and table
    gradients against the float64 oracle; gather against region forward within the sum of the two limits."""
    B, V, Cc, h, S, D, N = cfg
    ins = _problem(B, V, Cc, h, S, D, N, 500 + N, pos_fn)
    ins_cpu = [t.clone().double().requires_grad_(True) for t in ins]
    want = _oracle_core(*ins_cpu, h, 1, V)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(3))
    want.backward(cot.double())
    res = {}
    for new in (True, False):
        out, dev, rec = run(ins, h, V, monkeypatch, new, cot)
        e = dict(out=rel_err(out.detach().cpu().double(), want.detach()))
        if N > 1:
            for n, a, b in zip(("query", "k", "v", "table"), (dev[0], dev[1], dev[2], dev[4]),
                               (ins_cpu[0], ins_cpu[1], ins_cpu[2], ins_cpu[4])):
                e[n] = grad_err(a, b)
        res[new] = (out.detach().cpu().double(), e)
        print(f"\n[x3 {name}] {'gather_x3' if new else 'region   '}: " + "  ".join(f"{k} {v:.3e}" for k, v in e.items()))
        assert rec.names.count(NAME) == (1 if new else 0)
    both = rel_err(res[True][0], res[False][0])
    print(f"[x3 {name}] gather_x3 against region forward: {both:.3e}")
    for k, v in res[False][1].items():
        assert v < LIM[k], f"{name}: the PARENT route misses the limit on these inputs: {k} {v:.3e}"
    assert torch.isfinite(res[True][0]).all()
    for k, v in res[True][1].items():
        assert v < LIM[k], f"{name}: {k} {v:.3e}"
    assert both < 2.0 * LIM["out"], f"{name}: {both:.3e}"


def useless_bound_inputs(live_columns=0):
    """test_gpu_gather.py's test_exact_pass_behind_a_useless_static_bound: huge, mutually orthogonal Q and K, the static
    bound ||Q|| max ||K|| thousands of binades over the logits, every weight of the static pass zero.
    live_columns > 0: the BEV columns j < live_columns get a small Q instead (bound a few binades): they stay unflagged."""
    B, V, Cc, h, S, D, N = 1, 1, 32, 1, 12, 2, 150
    gen = torch.Generator().manual_seed(9)
    query = torch.zeros(B, Cc, S, S)
    query[:, :16] = torch.randn(B, 16, S, S, generator=gen) * 60.0
    k = torch.zeros(B * V, N, Cc)
    k[..., 16:] = torch.randn(B * V, N, 16, generator=gen) * 60.0
    k[..., :16] = torch.randn(B * V, N, 16, generator=gen) * 0.02
    v = torch.randn(B * V, N, Cc, generator=gen)
    pos = (torch.rand(B * V, N, 2, generator=gen) * 2 - 1) * 0.9
    table = torch.randn(h, 2 * S - 1, 2 * S * D - 1, generator=gen) * 0.3
    if live_columns:
        query[..., :live_columns] *= 0.01 / 60.0          # (B, C, i, j): the last axis is the BEV column
    return (query, k, v, pos, table), (B, V, Cc, h, S, D, N)


@pytest.mark.parametrize("live_columns", [0, 5], ids=["every column flagged", "some columns flagged"])
def test_exact_pass_behind_a_useless_static_bound(live_columns, monkeypatch):
    """Finite and within the out limit; the flags the entry point leaves show that its static pass handed every column
    (all but the live ones) to its exact pass -- both launches of the one call did their part: a static pass alone would
    return 0 / 0 on the flagged columns, an exact pass alone is not what the unflagged ones ran."""
    ins, (B, V, Cc, h, S, D, N) = useless_bound_inputs(live_columns)
    want = _oracle_core(*[t.double() for t in ins], h, 1, V)
    got, _, rec = run(ins, h, V, monkeypatch, True, probe=True)
    ref, _, _ = run(ins, h, V, monkeypatch, False)
    e, ep = rel_err(got.detach().cpu().double(), want), rel_err(ref.detach().cpu().double(), want)
    print(f"\n[x3 exact pass, {live_columns} live columns] {rec.flagged} of {rec.n_col} columns flagged; out gather_x3 {e:.3e}"
          f"  region {ep:.3e}")
    assert rec.names.count(NAME) == 1 and rec.n_col == h * S
    assert rec.flagged == h * (S - live_columns)
    assert torch.isfinite(got).all()
    assert ep < LIM["out"], f"the PARENT route misses the limit on these inputs: {ep:.3e}"
    assert e < LIM["out"], e


@pytest.mark.parametrize("what", ["q and k", "table"])
def test_large_logits(what, monkeypatch):
    """The geometry of CASES[0] (a window that fits) with logits of a few hundred log2 units: Q and K scaled by 6 each
    (Q . K c^-0.5 log2 e reaches 163), or the table by 30 (bias of tens of units: a standard deviation of 13, +-51 at the
    table's tails).  Where a dropped lo lo term of the logit product or a one-plane table would show.
    Q and K are scaled DOWN from a first choice of 10 each (|Q . K| up to 803) and then 6 each (289): there the region
    forward itself missed the out limit (MI355X: region 3.36e-4 / 2.50e-4, gather 3.34e-4 / 2.48e-4 against 2e-4 -- the two
    routes alike, both with three-term products), and the limit is asked on inputs where the region forward passes it.
    The table: a bias entry and its weight are carried as hi + lo, each to 2^-18 relative, so the bias of a pair is exact
    to ~2^-17 |bias| where the region forward's f32 interpolation is exact to 2^-24: at "tens of units" that is under
    4e-4 log2 units per logit.  At a table scaled by 100 (|bias| up to 170, beyond what is asked here) the gather forward
    measured 2.3e-4 against the region forward's 1.0e-4 and the 2e-4 limit, with three or with four terms in the bias
    products alike (the representation, not the dropped lo lo term): DESIGN.md records it."""
    name, (B, V, Cc, h, S, D, N), pos_fn = CASES[0]
    query, k, v, pos, table = _problem(B, V, Cc, h, S, D, N, 500 + N, pos_fn)
    if what == "table":
        table = table * 30.0
    else:
        query, k = query * 4.5, k * 4.5          # see the docstring
    ins = (query, k, v, pos, table)
    c = Cc // h
    s = torch.einsum("bhcm,bnhc->bhmn", query.reshape(B, h, c, S * S).repeat_interleave(V, 0), k.reshape(B * V, N, h, c))
    s = s * (c ** -0.5 * ops.LOG2E)
    want = _oracle_core(*[t.double() for t in ins], h, 1, V)
    got, _, rec = run(ins, h, V, monkeypatch, True, probe=True)
    ref, _, _ = run(ins, h, V, monkeypatch, False)
    e, ep = rel_err(got.detach().cpu().double(), want), rel_err(ref.detach().cpu().double(), want)
    print(f"\n[x3 large logits: {what}] max |Q.K| {s.abs().max().item():.0f} log2 units, max |bias| "
          f"{table.abs().max().item() * ops.LOG2E:.0f}; {rec.flagged} of {rec.n_col} columns flagged; out gather_x3 {e:.3e}"
          f"  region {ep:.3e}")
    assert torch.isfinite(got).all()
    assert ep < LIM["out"], f"the PARENT route misses the limit on these inputs: {ep:.3e}"
    assert e < LIM["out"], e


def band_rows(S, bands):
    """query indices m = i S + j: the first and last BEV row of every band (two columns), row S - 1"""
    rows = [i * S + j for r0, n in bands for i in (r0, r0 + n - 1) for j in (3, S - 4)]
    return torch.tensor(sorted(set(rows + [(S - 1) * S + 3, (S - 1) * S + S - 1])))


@pytest.mark.parametrize("S", [232, 400])
def test_bands(S, monkeypatch):
    """S above 224: two bands (S = 232: 128 rows and a ragged 104; S = 400: 208 + 192), 300 scattered keys, one head, one
    view.  The oracle on the first and last row of every band, row S - 1 and 32 random rows; gather against region
    forward on all rows; the padding rows S .. Sp - 1 have a finite LSE; after a backward every gradient is finite."""
    Cc, h, D, N = 32, 1, 3, 300
    bands = ops.gather_bands(S)
    assert len(bands) == 2 and bands[0][1] % 16 == 0 and bands[0][1] <= 224
    ins = _problem(1, 1, Cc, h, S, D, N, 700 + S, lambda u: (u * 2 - 1) * 0.9)
    p = dict(query=ins[0], k=ins[1], v=ins[2], pos=ins[3], table=ins[4])
    rows = torch.unique(torch.cat((pick_rows(S, 32, S), band_rows(S, bands))))
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    want, _ = oracle_rows(p, h, rows, None, want_grads=False)
    cot = torch.randn(1, S * S, Cc, generator=torch.Generator().manual_seed(5))
    keep = {}
    got, dev, rec = run(ins, h, 1, monkeypatch, True, cot, keep=keep)
    ref, _, _ = run(ins, h, 1, monkeypatch, False)
    assert rec.names.count(NAME) == len(bands)
    e = rel_err_rows(got.detach().cpu()[:, rows], want)
    ep = rel_err_rows(ref.detach().cpu()[:, rows], want)
    both = rel_err(got.detach().cpu().double(), ref.detach().cpu().double())
    print(f"\n[x3 bands S={S}] {len(rows)} rows against the oracle: gather_x3 {e:.3e}  region {ep:.3e}; "
          f"gather_x3 against region on all rows {both:.3e}")
    g = keep["g"]
    lse = keep["LSE"].reshape(2, g.n_prob, g.heads, S, g.Sp)
    assert torch.isfinite(lse[0]).all(), "LSE plane 0, padding rows included"
    assert torch.isfinite(lse[1][..., :S]).all()
    assert torch.isfinite(got).all()
    assert ep < LIM["out"], f"the PARENT route misses the limit on these inputs: {ep:.3e}"
    assert e < LIM["out"], e
    assert both < 2.0 * LIM["out"], both
    for n, t in zip(("query", "k", "v", "pos", "table"), dev):
        assert t.grad is not None and torch.isfinite(t.grad).all(), n


def test_benchmark_bev_size_one_view(monkeypatch):
    """S = 200 (13 row blocks, two per wave, the last wave's second block past the column), D = 5, 1 500 keys, one view,
    two heads: the benchmark's launch shape.  Gather against region forward on all rows within the sum of the limits;
    the rows past the grid that no 16-row block covers (208 .. 223 of every column) are never written: zero in O."""
    B, V, Cc, h, S, D, N = 1, 1, 64, 2, 200, 5, 1500
    ins = _problem(B, V, Cc, h, S, D, N, 77, lambda u: (u * 2 - 1) * 0.9)
    keep = {}
    got, _, rec = run(ins, h, V, monkeypatch, True, keep=keep)
    ref, _, _ = run(ins, h, V, monkeypatch, False)
    assert rec.names.count(NAME) == 1
    e = rel_err(got.detach().cpu().double(), ref.detach().cpu().double())
    print(f"\n[x3 S=200, 1500 keys] gather_x3 against region forward: {e:.3e}")
    assert torch.isfinite(got).all()
    assert e < 2.0 * LIM["out"], e
    g = keep["g"]
    O = keep["O"].reshape(g.n_prob, g.heads, S, g.Sp, 32)
    assert torch.isfinite(O).all()
    assert (O[..., 16 * ((S + 15) // 16):, :] == 0).all(), "rows past the grid"
    assert torch.isfinite(keep["LSE"][0]).all()


# ---- the modules ---------------------------------------------------------------------------------------------------
from test_gpu_modules import SCA, TSA, _sca, _tsa, check          # noqa: E402  (the small golden shapes of that file)


@pytest.mark.parametrize("name", TSA)
def test_tsa_module(name, monkeypatch):
    """Split-mode TSADeformableAttention on the golden shapes of tests/test_gpu_modules.py with the switch on: output
    and every gradient at that file's f32 limits (check: the split mode is held to the f32 limits), through the new
    entry point."""
    def build():
        m, z, query, prev = _tsa(name, X3)
        return m, z, query, prev

    def call(m, query, prev):
        return m(prev, query, {"k": 1}, False)[0]

    errs = {}
    for new in (False, True):
        rec = Recorder()
        with monkeypatch.context() as mp:
            mp.setenv("BEVR_GATHER_X3", "1" if new else "0")
            mp.delenv("BEVR_GATHER", raising=False)
            mp.setattr(ops, "_launch", rec)
            m, z, query, prev = build()
            out = call(m, query, prev)
            torch.cuda.synchronize()
            errs[new] = (out.detach().cpu().double() - torch.tensor(z["out"]).double()).abs().max().item()
            assert (NAME in rec.names) == new and (REGION in rec.names) == (not new), rec.names
            if new:
                print(f"\n[x3 TSA {name}] max |out - golden|: gather_x3 {errs[True]:.3e}  region {errs[False]:.3e}")
                check(m, z, out, {"query": query, "prev_bev": prev}, _lib.PREC_F32)


@pytest.mark.parametrize("name", SCA)
def test_sca_module(name, monkeypatch):
    """Split-mode SCADeformableAttention on the golden shapes of tests/test_gpu_modules.py at that file's f32 limits, with
    BEVR_TAP_X3=1 as well.  (At these shapes no call has a tap segment -- 6 x 10 and 8 x 22 feature maps put the learned
    offset range outside the tap grid -- so every key runs on the new entry point; the tap half is the next test's.)"""
    errs = {}
    for new in (False, True):
        rec = Recorder()
        with monkeypatch.context() as mp:
            mp.setenv("BEVR_GATHER_X3", "1" if new else "0")
            mp.setenv("BEVR_TAP_X3", "1")
            mp.delenv("BEVR_GATHER", raising=False)
            mp.setattr(ops, "_launch", rec)
            m, z, query, x, ref = _sca(name, X3)
            out, _ = m(x, query, ref, None, False)
            torch.cuda.synchronize()
            errs[new] = (out.detach().cpu().double() - torch.tensor(z["out"]).double()).abs().max().item()
            assert (NAME in rec.names) == new and (REGION in rec.names) == (not new), rec.names
            if new:
                print(f"\n[x3 SCA {name}] max |out - golden|: gather_x3 {errs[True]:.3e}  region {errs[False]:.3e}")
                check(m, z, out, {"query": query, "x": x}, _lib.PREC_F32)


def test_sca_module_tap_and_gather_halves(monkeypatch):
    """SpatialCrossAttn at the smallest size at which the reference's own float32 error leaves room under the limits
    (tests/test_gpu_tap_x3.py: S = 72, 24 x 64 features, six views, 256 rows against the float64 oracle, out 3e-4,
    gradients 3e-3, offset heads 1.5e-2) with BEVR_TAP_X3=1 and BEVR_GATHER_X3=1: the projector-pinned keys on the tap
    kernels, the scattered keys on the new entry point, merged through (O, LSE).  The parent's route (BEVR_GATHER_X3=0)
    runs on the same inputs first; both print their output error."""
    from test_gpu_fullsize import _sca_module_rows
    for new in (False, True):
        rec = Recorder()
        with monkeypatch.context() as mp:
            mp.setenv("BEVR_GATHER_X3", "1" if new else "0")
            mp.setenv("BEVR_TAP_X3", "1")
            mp.delenv("BEVR_GATHER", raising=False)
            mp.setattr(ops, "_launch", rec)
            print(f"\n[x3 SCA S=72, tap + {'gather_x3' if new else 'region'}]", end="")
            _sca_module_rows(X3, S=72, img_w=256, img_h=96, n_rows=256, max_split=10000)
        assert (NAME in rec.names) == new and (REGION in rec.names) == (not new), rec.names
        for k in ("bevr_attn_tap_fwd", "bevr_attn_tap_bwd_q", "bevr_attn_tap_bwd_k", "bevr_attn_bwd_q", "bevr_attn_bwd_k"):
            assert k in rec.names, rec.names
        assert not any(k.startswith("bevr_attn_cell") for k in rec.names), rec.names
