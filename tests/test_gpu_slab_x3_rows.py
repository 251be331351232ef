"""The split-bf16 slab query-side backward in row bands (csrc/attn_slab_bwd_q_x3_rows.hip, bevr_attn_slab_bwd_q_x3_rows;
BEV sides up to 448) through ops.attention_core, behind BEVR_SLAB_X3=2, against the float64 oracle
(oracle/bevrender_oracle.py: attention_core) at the project's f32 limits (tests/test_gpu_fullsize.py:
LIMITS[PREC_BF16X3]: out 2e-4, query 5e-4, table 2.5e-4, max |err| / max |want| per tensor) and against the parent's
route for these sides, the query-tile kernel bevr_attn_bwd_q (BEVR_SLAB_X3=0), on the same inputs.

WHICH entry points ran is read off a recorder around ops._launch: the new kernel once per band, its prep once, the
query-tile kernel not at all -- and the other way round on the parent's route, which is asserted first with a message of
its own (if it misses a limit the inputs are at fault).  Every case prints its figures before it asserts (-s); the
recorded run is profiles/slab_x3_rows.txt.

  * small grids forced into bands of one and of two row blocks (tests/test_gpu_slab_rows.py's SMALL, every worker
    arrangement a tall grid has), whole gradients;
  * the operand-split and bias-path cases of tests/test_gpu_slab_x3.py through bands of one block;
  * tall grids (two and three bands, both row pitches) on sampled rows with a cotangent that is zero elsewhere, and keys
    far outside the table at S = 218 (the clamped body in a band with row0 > 0);
  * S = 400 with a dense cotangent against the query-tile kernel over every row of both bands;
  * the SCA module on the small golden shapes with every split-mode switch on and the bands forced."""
import pytest
import torch

from bevrender_amd import _lib, ops
from oracle import bevrender_oracle as O
from test_gpu_fullsize import LIMITS, rel_err
from test_gpu_slab import _problem
from test_gpu_slab_rows import SMALL, _far, _spread, _tall_reference
from test_gpu_slab_x3 import Recorder, case, max_logit, oracle_grads
from test_gpu_slab import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
X3 = _lib.PREC_BF16X3
LIM = LIMITS[X3]
NAME, PREP, TILE = "bevr_attn_slab_bwd_q_x3_rows", "bevr_attn_slab_x3_rows_prep", "bevr_attn_bwd_q"
SWITCHES = ("BEVR_SLAB", "BEVR_SLAB_ROWS", "BEVR_SLAB_X3", "BEVR_GATHER_X3", "BEVR_TAP_X3")
FORCED = {"BEVR_SLAB_X3": "2", "BEVR_SLAB_ROWS": "2", "BEVR_SLAB": "2"}      # bands for every side and table width
PARENT = {"BEVR_SLAB_X3": "0"}


def launched(monkeypatch, env, S, fn):
    """fn() -> dict under the switches `env` (every other route switch unset) with the recorder around ops._launch; the
    entry points that ran go into the result ("route") and are asserted by assert_route once the case has printed"""
    rec = Recorder()
    with monkeypatch.context() as m:
        for name in SWITCHES:
            m.delenv(name, raising=False)
        for k, v in env.items():
            m.setenv(k, v)
        m.setattr(ops, "_launch", rec)
        res = fn()
        torch.cuda.synchronize()
        res["route"] = (list(rec.names), env.get("BEVR_SLAB_X3") == "2", len(ops.slab_bands(S)))
    return res


def assert_route(res):
    """the new route: the band kernel once per band of ops.slab_bands(S), one prep, no query-tile kernel; the parent's:
    the query-tile kernel once and no slab entry point"""
    names, new, n_bands = res["route"]
    slab = [n for n in names if n.startswith("bevr_attn_slab")]
    if new:
        assert names.count(NAME) == n_bands and names.count(PREP) == 1, names
        assert TILE not in names and sorted(set(slab)) == sorted((NAME, PREP)), names
    else:
        assert names.count(TILE) == 1 and not slab, f"the PARENT route ran {names}"


def run_kv(ins, h, g, V, S, monkeypatch, env):
    """ops.attention_core on (query, kv, pos, table) in split mode with tests/test_gpu_slab.py's dense cotangent"""
    def go():
        query, kv, pos, table = (t.clone().to(DEV).requires_grad_(True) for t in ins)
        out = ops.attention_core(query, None, None, pos, table, heads=h, groups=g, views=V, precision=X3, kv=kv)
        out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(77)).to(DEV))
        return dict(out=out.detach(), dq=query.grad, dt=table.grad, dkv=kv.grad, dp=pos.grad)
    return launched(monkeypatch, env, S, go)


def one_key_scale(ins, B, V, C, h, S, N):
    """One key: P = 1 and dS = P (dP - delta) = 0 for every pair, the oracle's gradients are zero to the last bit and
    max |want| normalises nothing.  The normalisation of tests/test_gpu_slab_x3.py: the kernels form the DIFFERENCE of
    dP = dO . V and delta = dO . O, each as large as ||dO|| ||V||, so the error is measured against the gradients' size
    before that cancellation (d(table) sums dS over <= 1 tap weight per cell and row, dQ = dS K c^-0.5)."""
    c = C // h
    cot = torch.randn(B * V, S * S, C, generator=torch.Generator().manual_seed(77)).double()
    dp = (cot.reshape(B * V, S * S, h, c).norm(dim=-1).amax(1)
          * ins[1][..., C:].double().reshape(B * V, N, h, c).norm(dim=-1).amax(1)).max().item()
    return dict(query=dp * ins[1][..., :C].abs().max().item() * c ** -0.5, table=dp)


def compare(tag, new, old, want, scale=None):
    """both routes' dQ and d(table) against the oracle's (want), the parent's first; forward and key side between them"""
    if scale is None:
        err = lambda got, w, k: rel_err(got.cpu(), w)          # noqa: E731
    else:
        assert want[0].abs().max().item() < 1e-12 and want[1].abs().max().item() < 1e-12
        err = lambda got, w, k: got.cpu().double().abs().max().item() / scale[k]          # noqa: E731
    e1 = dict(query=err(new["dq"], want[0], "query"), table=err(new["dt"], want[1], "table"))
    e0 = dict(query=err(old["dq"], want[0], "query"), table=err(old["dt"], want[1], "table"))
    e_kv, e_p = rel_err(new["dkv"], old["dkv"]), rel_err(new["dp"], old["dp"])
    print(f"\n[slab x3 rows {tag}] bands: dQ {e1['query']:.3e} d(table) {e1['table']:.3e} | query-tile: dQ {e0['query']:.3e} "
          f"d(table) {e0['table']:.3e} | limits {LIM['query']:.1e} {LIM['table']:.1e} | dK|dV {e_kv:.2e} d(pos) {e_p:.2e} "
          f"between the routes")
    assert_route(old)
    for k in ("query", "table"):
        assert e0[k] < LIM[k], f"{tag}: the PARENT route misses the limit on these inputs: {k} {e0[k]:.3e}"
    assert_route(new)
    assert torch.equal(new["out"], old["out"]), "the forward does not depend on the switch"
    assert e_kv < 1e-5 and e_p < 1e-4, (e_kv, e_p)          # the key side: equal up to its atomics' order
    assert torch.isfinite(new["dq"]).all() and torch.isfinite(new["dt"]).all()
    for k in ("query", "table"):
        assert e1[k] < LIM[k], f"{tag}: {k} {e1[k]:.3e}"
    return e1, e0


# ---- small grids forced into bands ------------------------------------------------------------------------------------
_small = {}


def small_reference(name, monkeypatch):
    """inputs, the oracle's gradients and the parent route's results of a SMALL case: once, left unchanged"""
    if name not in _small:
        B, V, C, h, g, S, N, Wt, extra = SMALL[name]
        ins = _problem(B, V, C, h, g, S, N, Wt, seed=len(name) + 7 * S, **extra)
        want = oracle_grads(ins, B, V, C, h, g, S, N)
        _small[name] = (ins, want, run_kv(ins, h, g, V, S, monkeypatch, PARENT))
    return _small[name]


@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("name", list(SMALL))
def test_small_grids_in_bands_of_one_and_two_row_blocks(name, blocks, monkeypatch):
    """BEVR_SLAB_X3=2 with BEVR_SLAB_ROWS=2 and BEVR_SLAB=2, a band of `blocks` row blocks: a first block above 0, idle
    workers, a ragged last block, far keys over two views, two channel groups, one key -- at sizes where the whole
    gradient is compared with the float64 oracle."""
    B, V, C, h, g, S, N, Wt, extra = SMALL[name]
    ins, want, old = small_reference(name, monkeypatch)
    monkeypatch.setattr(ops, "SLAB_BAND_BLOCKS", blocks)
    bands = ops.slab_bands(S)
    assert len(bands) == -(-(-(-S // 31)) // blocks) and (len(bands) > 1 or S <= 31 * blocks)
    for k, v in FORCED.items():
        monkeypatch.setenv(k, v)
    assert ops.slab_x3_rows_supported(X3, S, Wt)
    new = run_kv(ins, h, g, V, S, monkeypatch, FORCED)
    scale = one_key_scale(ins, B, V, C, h, S, N) if N == 1 else None
    compare(f"{name} blocks={blocks} bands {bands}", new, old, want, scale)
    assert new["dt"].abs().sum() > 0 or N == 1


# ---- operand split and bias path, through bands of one block ----------------------------------------------------------
def _scaled_case(tag, monkeypatch, **scales):
    name = "three_row_blocks"
    B, V, C, h, g, S, N, Wt, extra = CASES[name]
    ins, want = case(name, **scales)
    monkeypatch.setattr(ops, "SLAB_BAND_BLOCKS", 1)
    assert len(ops.slab_bands(S)) == 3
    old = run_kv(ins, h, g, V, S, monkeypatch, PARENT)
    new = run_kv(ins, h, g, V, S, monkeypatch, FORCED)
    compare(tag, new, old, want)
    return ins, (B, V, C, h, N, S)


def test_operand_split_at_large_logits(monkeypatch):
    """Q and K scaled by 3.6 each (tests/test_gpu_slab_x3.py): a product of single bf16 images or a missing lo term is
    three orders of magnitude over the limits"""
    name = "three_row_blocks"
    B, V, C, h, g, S, N, Wt, extra = CASES[name]
    big = max_logit(case(name, q_scale=3.6, k_scale=3.6)[0], B, V, C, h, N, S)
    print(f"\n[slab x3 rows operand split] max |Q.K| {big:.0f} log2 units")
    assert 80.0 < big < 163.0
    _scaled_case("operand split", monkeypatch, q_scale=3.6, k_scale=3.6)


def test_bias_path_at_a_large_table(monkeypatch):
    """the table scaled by 30 (tests/test_gpu_slab_x3.py): a bias path rounded to 16 bits misses the limits by two orders
    of magnitude"""
    _scaled_case("bias path", monkeypatch, t_scale=30.0)


# ---- tall grids against the oracle on sampled rows ----------------------------------------------------------------------
def run_tall(S, pos_fn, monkeypatch, env):
    p, rows, cot, want, grads = _tall_reference(S, pos_fn)

    def go():
        dev = {n: p[n].clone().to(DEV).requires_grad_(True) for n in ("query", "k", "v", "pos", "table")}
        out = ops.attention_core(dev["query"], dev["k"], dev["v"], dev["pos"], dev["table"], heads=2, groups=1, views=1,
                                 precision=X3)
        cot_full = torch.zeros_like(out)          # zero on every other row: a band that wrote dQ outside its rows fails
        cot_full[:, rows.to(DEV)] = cot.to(DEV)
        out.backward(cot_full)
        res = {n: dev[n].grad for n in dev}
        res["out"] = out.detach()
        return res
    return launched(monkeypatch, env, S, go)


# The ONE figure of the parent's route that is not held to its limit: (S, key set, tensor).  With the cotangent on ~80
# sampled rows the query-tile kernel's d(table) at S = 400 measured 4.454e-4 against the 2.5e-4 limit (the band kernel on
# the same inputs: 1.421e-4; with the dense cotangent at S = 400, below, the query-tile kernel is inside: 1.426e-4).  The
# inputs are fixed (tests/test_gpu_slab_rows.py's) and the query-tile kernel is not this file's subject: the figure is
# printed, marked, and recorded in profiles/slab_x3_rows.txt and DESIGN.md section 9 as an open point of that kernel.
PARENT_KNOWN_MISS = {(400, "_spread", "table")}


def tall_errors(tag, S, pos_fn, monkeypatch):
    """both routes on the tall inputs; out, d(query), d(table) of each against the oracle on the sampled rows, printed;
    the key side between the routes.  The parent's route is asserted first -- its kernels, then out, d(query) and
    d(table) at the limits, PARENT_KNOWN_MISS excepted -- then the new route's kernels and the same three limits."""
    p, rows, cot, want, grads = _tall_reference(S, pos_fn)
    old = run_tall(S, pos_fn, monkeypatch, PARENT)
    new = run_tall(S, pos_fn, monkeypatch, {"BEVR_SLAB_X3": "2"})          # the switch alone: S > 211, SCA's table
    errs = []
    for res in (new, old):
        assert torch.isfinite(res["out"]).all()
        e = dict(out=rel_err(res["out"][:, rows.to(DEV)].cpu(), want))
        e.update({n: rel_err(res[n].cpu(), grads[n]) for n in ("query", "table")})
        errs.append(e)
    e1, e0 = errs
    between = {n: rel_err(new[n], old[n]) for n in ("k", "v", "pos")}
    print(f"\n[slab x3 rows {tag}] bands {ops.slab_bands(S)}: out {e1['out']:.3e} dQ {e1['query']:.3e} d(table) "
          f"{e1['table']:.3e} | query-tile: out {e0['out']:.3e} dQ {e0['query']:.3e} d(table) {e0['table']:.3e} | limits "
          f"{LIM['out']:.1e} {LIM['query']:.1e} {LIM['table']:.1e} | between the routes dK {between['k']:.2e} dV "
          f"{between['v']:.2e} d(pos) {between['pos']:.2e}")
    assert_route(old)
    for n in ("out", "query", "table"):
        if (S, pos_fn.__name__, n) in PARENT_KNOWN_MISS:
            print(f"[slab x3 rows {tag}] PARENT_KNOWN_MISS: the query-tile kernel's {n} {e0[n]:.3e} is not held to {LIM[n]:.1e}")
            continue
        assert e0[n] < LIM[n], f"{tag}: the PARENT route misses the limit on these inputs: {n} {e0[n]:.3e}"
    assert_route(new)
    for n in ("out", "query", "table"):
        assert e1[n] < LIM[n], f"{tag}: {n} {e1[n]:.3e}"
    return p, new, old, between


@pytest.mark.parametrize("S", [218, 400, 404, 448])
def test_tall_grids_rows_and_gradients(S, monkeypatch):
    """BEVR_SLAB_X3=2 alone, D = 5, 1 500 scattered keys: 218 the smallest side with two bands, 400 config 5's (the
    832-row pitch, 7 owned columns), 404 the first side on the 960-row pitch (6 columns), 448 the limit (three bands).
    Sampled rows -- random ones, the first and last row of every band in two columns, row S - 1 -- with the inputs and
    the oracle results of tests/test_gpu_slab_rows.py; dK, dV and d(pos) are the key-side kernel's on both routes and
    compared between them (up to the order of the atomics in d(pos))."""
    assert len(ops.slab_bands(S)) == {218: 2, 400: 2, 404: 2, 448: 3}[S]
    p, new, old, between = tall_errors(f"tall S={S}", S, _spread, monkeypatch)
    assert torch.equal(new["out"], old["out"])
    assert between["k"] < 1e-5 and between["v"] < 1e-5 and between["pos"] < 1e-4, between


def test_tall_grid_with_keys_far_outside_the_table(monkeypatch):
    """S = 218 with 20 % of the keys at four times their distance: 32-key halves that take the clamped body in the second
    band (row0 = 124)"""
    S = 218
    p, new, old, between = tall_errors(f"tall far S={S}", S, _far, monkeypatch)
    a = (1.0 - p["pos"][..., 0]) * ((S - 1) / 2.0)
    assert ((a < -10) | (a > S - 1 + 8)).float().mean() > 0.05          # keys outside the window's unclamped rows
    assert ops.slab_bands(S)[1][0] == 124


# ---- config 5's side, a dense cotangent -------------------------------------------------------------------------------
def test_bev400_dense_cotangent_agrees_with_the_query_tile_kernel(monkeypatch):
    """S = 400, 600 keys, a dense cotangent: dQ and d(table) over every row of both bands.  Each route within the limits
    of the float64 oracle (materialised on the device: 160 000 x 600 pairs per head), and the two routes within the
    same 5e-4 / 2.5e-4 of the parent's largest entry of each other -- the single limit, not twice it: the one-band
    kernel's recorded A/B figures are 1.1e-5 / 2.8e-5."""
    S, N, h, C = 400, 600, 2, 64
    ins = _problem(1, 1, C, h, 1, S, N, 2 * S * 5 - 1, seed=400)
    old = run_kv(ins, h, 1, 1, S, monkeypatch, PARENT)
    new = run_kv(ins, h, 1, 1, S, monkeypatch, {"BEVR_SLAB_X3": "2"})
    query, kv, pos, table = (t.clone().double().to(DEV).requires_grad_(True) for t in ins)
    c = C // h
    o = O.attention_core(query[0].reshape(h, c, S * S), kv[0, :, :C].reshape(N, h, c).permute(1, 2, 0),
                         kv[0, :, C:].reshape(N, h, c).permute(1, 2, 0), pos, table, S, S, 1, c ** -0.5)
    want_out = o.reshape(C, S * S).t()[None]
    want_out.backward(torch.randn(want_out.shape, generator=torch.Generator().manual_seed(77)).double().to(DEV))
    want = (query.grad.cpu(), table.grad.cpu())
    e_out = rel_err(new["out"].cpu(), want_out.detach().cpu())
    e_q, e_t = rel_err(new["dq"], old["dq"]), rel_err(new["dt"], old["dt"])
    print(f"\n[slab x3 rows S=400 dense] out vs oracle {e_out:.3e}; bands vs query-tile: dQ {e_q:.2e} d(table) {e_t:.2e}")
    compare("S=400 dense", new, old, want)
    assert e_out < LIM["out"], e_out
    assert e_q < LIM["query"] and e_t < LIM["table"], (e_q, e_t)


# ---- the module ----------------------------------------------------------------------------------------------------
from test_gpu_modules import SCA, _sca, check          # noqa: E402  (the small golden shapes of that file)


@pytest.mark.parametrize("name", SCA)
def test_sca_module(name, monkeypatch):
    """Split-mode SCADeformableAttention on the golden shapes of tests/test_gpu_modules.py with every split-mode switch on
    (BEVR_TAP_X3, BEVR_GATHER_X3, BEVR_SLAB_X3=2) and the bands forced (BEVR_SLAB_ROWS=2, BEVR_SLAB=2: these small tables
    are narrower than SCA's; bands of one row block): output and every gradient at that file's f32 limits, through the
    new entry point -- after the same module with BEVR_SLAB_X3=0, the parent's route, at the same limits."""
    monkeypatch.setattr(ops, "SLAB_BAND_BLOCKS", 1)
    for slab_x3 in ("0", "2"):
        rec = Recorder()
        with monkeypatch.context() as mp:
            for k, v in (("BEVR_TAP_X3", "1"), ("BEVR_GATHER_X3", "1"), ("BEVR_SLAB_X3", slab_x3), ("BEVR_SLAB", "2"),
                         ("BEVR_SLAB_ROWS", "2")):
                mp.setenv(k, v)
            mp.setattr(ops, "_launch", rec)
            m, z, query, x, ref = _sca(name, X3)
            S = int(z["cfg"][4])
            out, _ = m(x, query, ref, None, False)
            torch.cuda.synchronize()
            e = (out.detach().cpu().double() - torch.tensor(z["out"]).double()).abs().max().item()
            print(f"\n[slab x3 rows SCA {name} BEVR_SLAB_X3={slab_x3}] S = {S}, bands {ops.slab_bands(S)}: max |out - golden| {e:.3e}")
            check(m, z, out, {"query": query, "x": x}, _lib.PREC_F32)
        if slab_x3 == "0":
            assert TILE in rec.names and NAME not in rec.names, f"the PARENT route: {rec.names}"
        else:
            assert rec.names.count(NAME) >= len(ops.slab_bands(S, 1)) and PREP in rec.names, rec.names
            assert TILE not in rec.names and "bevr_attn_slab_bwd_q_x3" not in rec.names, rec.names
