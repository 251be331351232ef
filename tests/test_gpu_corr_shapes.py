"""The correlation head (csrc/corr.hip: bevr_corr_fwd, bevr_corr_bwd, bevr_recall_rank) off the square batch, against a
float64 reference written out here: rectangular n != m on every instantiation of the one-pass kernels and on the general
ones, ragged fragment counts, a ragged second grid sweep, one tensor as both sides, zero rows under normalize=True,
misaligned pointers through the C ABI, the 4-wave build of the Gram (BEVR_GRAM_WAVES=4, in a child process), and the rank
vector of bevr_recall_rank compared exactly (ties, NaN, infinities, sizes around the 256-thread block).

Inputs of every shape case: randn rows; the first min(n, m) map rows are cam + 0.8 randn; cam rows are then scaled by
logspace(-3, 3, n), map rows by logspace(2, -2, m); the cotangent is randn(n, m).  With rows six decades apart an error
taken against the largest entry of the matrix sees one row, so the errors here are taken per entry and per row:
  D      |got - want|[i, j] / (2 + 2 a_i b_j), a_i = |cam_i|, b_j = |map_j| on raw rows and 1 on normalised ones (the size
         of the terms before the subtraction), the worst entry;
  dcam, dmap   per row max_e |got - want| / max_e |want|, the worst row.
D is held to 2e-5 and the gradients to 1e-4 (the tolerances of tests/test_gpu_corr_alias.py); a limit is raised to 4 x
the error of the same expression in torch float32 on the CPU, measured here against float64, only where that is larger
(the rule of tests/test_gpu_glue_edges.py).  One line per case is printed (profiles/corr_shapes.txt is that table)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from bevrender_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"D": 2e-5, "dcam": 1e-4, "dmap": 1e-4}
E_ALIGN = -4

# ---- the constants of csrc/corr.hip that place a shape on its path: a changed one fails here, not by moving a case ----
with open(os.path.join(_lib.CSRC, "corr.hip")) as _f:
    _SRC = _f.read()


def _src_int(pattern):
    found = re.findall(pattern, _SRC)
    assert len(found) == 1, (pattern, found)
    return [int(v) for v in (found[0] if isinstance(found[0], tuple) else (found[0],))]


(MAX_ROWS,) = _src_int(r"constexpr int CORR_MAX_ROWS = (\d+);")
(ECHUNK,) = _src_int(r"constexpr int ECHUNK = (\d+);")
(TB,) = _src_int(r"constexpr int TB = (\d+);")
_cap = _src_int(r"want < (\d+) \? \(want < 1 \? 1 : want\) : (\d+)\);")            # the Gram's grid cap
(_waves,) = _src_int(r'atoi\(getenv\("BEVR_GRAM_WAVES"\)\) : (\d+);')               # waves per workgroup by default
(_per_wave,) = _src_int(r"const long long stride = \(long long\)gridDim\.x \* NW \* (\d+);")
(BWD_CHUNK,) = _src_int(r"const int chunks = \(E \+ (\d+)\) / 1024;")
assert MAX_ROWS == 64
assert ECHUNK == 4096
assert TB == 8
assert _cap == [512, 512] and _waves == 8 and _per_wave == 32
SWEEP = _cap[0] * _waves * _per_wave
assert SWEEP == 131072
assert BWD_CHUNK == 1023


def _frags(n):
    return -(-n // 16)


def fwd_path(n, m, E):
    """the dispatch of bevr_corr_fwd"""
    if n <= MAX_ROWS and m <= MAX_ROWS and E % 4 == 0:
        fa, fb = _frags(n), _frags(m)
        return "mfma<1,1>" if fa == 1 and fb == 1 else "mfma<2,2>" if fa <= 2 and fb <= 2 else "mfma<4,4>"
    return "general"


# (n, m, E, the Gram instantiation, what else the shape is there for)
ONE_PASS = [
    (1, 1, 4, "mfma<1,1>", lambda n, m, E: E < _per_wave),                           # waves 1 .. 7 never enter the loop
    (3, 16, 36, "mfma<1,1>", lambda n, m, E: E % 32 == 4 and E > 32),
    (16, 17, 1000, "mfma<2,2>", lambda n, m, E: _frags(n) != _frags(m)),
    (32, 5, 4100, "mfma<2,2>", lambda n, m, E: _frags(n) != _frags(m)),
    (33, 8, 260, "mfma<4,4>", lambda n, m, E: (_frags(n), _frags(m)) == (3, 1)),
    (8, 48, 1028, "mfma<4,4>", lambda n, m, E: (_frags(n), _frags(m)) == (1, 3)),
    (64, 1, 64, "mfma<4,4>", lambda n, m, E: n == MAX_ROWS),
    (64, 64, 128, "mfma<4,4>", lambda n, m, E: n == m == MAX_ROWS),
    (40, 5, 131108, "mfma<4,4>", lambda n, m, E: SWEEP < E < 2 * SWEEP and (E - SWEEP) % 32 != 0),   # ragged second sweep
]
GENERAL = [
    (65, 3, 1024, lambda n, m, E: n == MAX_ROWS + 1 and m <= MAX_ROWS and E % 4 == 0),
    (3, 65, 1024, lambda n, m, E: m == MAX_ROWS + 1 and n <= MAX_ROWS and E % 4 == 0),
    (80, 72, 1028, lambda n, m, E: n % TB == 0 and m % TB == 0 and n // TB != m // TB and E % 4 == 0),
    (5, 40, 1027, lambda n, m, E: E % 4 != 0 and n % TB and n < TB),
    (17, 70, 1029, lambda n, m, E: E % 4 != 0 and n % TB and m % TB),
    (2, 3, 5, lambda n, m, E: E % 4 != 0),
    (1, 1, 1, lambda n, m, E: E % 4 != 0),
    (9, 7, 4099, lambda n, m, E: ECHUNK < E < 2 * ECHUNK and E // 1024 == 4 and E % 4 != 0),
]


def _ids(cases):
    return [f"{c[0]}x{c[1]}x{c[2]}" for c in cases]


# =====================================================================================================================
# inputs, reference, measures
# =====================================================================================================================
def _inputs(n, m, E, seed=None):
    gen = torch.Generator().manual_seed(n * 1000003 + m * 1009 + E if seed is None else seed)
    cam = torch.randn(n, E, generator=gen)
    mp = torch.randn(m, E, generator=gen)
    k = min(n, m)
    mp[:k] = cam[:k] + 0.8 * torch.randn(k, E, generator=gen)
    cam = cam * torch.logspace(-3, 3, n)[:, None]
    mp = mp * torch.logspace(2, -2, m)[:, None]
    cot = torch.randn(n, m, generator=gen)
    return cam, mp, cot


def _expr(cam, mp, cot, normalize, dtype):
    """(D, dcam, dmap) of 2 - 2 a b^T by autograd on the CPU in `dtype`; mp None: one tensor as both sides, (D, dx)"""
    c = cam.detach().cpu().to(dtype).clone().requires_grad_(True)
    p = c if mp is None else mp.detach().cpu().to(dtype).clone().requires_grad_(True)
    a, b = (F.normalize(c, dim=1), F.normalize(p, dim=1)) if normalize else (c, p)
    D = 2 - 2 * a @ b.T
    g = torch.autograd.grad(D, (c,) if mp is None else (c, p), cot.cpu().to(dtype))
    return (D.detach(),) + tuple(g)


def _kernel(cam, mp, cot, normalize):
    c = cam.to(DEV).requires_grad_(True)
    p = c if mp is None else mp.to(DEV).requires_grad_(True)
    D = ops.pairwise_corr(c, p, normalize)
    D.backward(cot.to(DEV))
    torch.cuda.synchronize()
    return (D.detach(), c.grad) + (() if mp is None else (p.grad,))


def _err_D(got, want, cam, mp, normalize):
    n, m = want.shape
    a = torch.ones(n, dtype=torch.float64) if normalize else cam.double().norm(dim=1)
    b = torch.ones(m, dtype=torch.float64) if normalize else (cam if mp is None else mp).double().norm(dim=1)
    return ((got.double().cpu() - want).abs() / (2 + 2 * a[:, None] * b[None, :])).max().item()


def _err_rows(got, want):
    den = want.abs().amax(1)
    assert (den > 0).all(), "a reference gradient row is zero: the row-relative measure needs another input"
    return ((got.double().cpu() - want).abs().amax(1) / den).max().item()


def _errors(res, want, cam, mp, normalize):
    e = {"D": _err_D(res[0], want[0], cam, mp, normalize)}
    for name, g, w in zip(("dcam", "dmap"), res[1:], want[1:]):
        e[name] = _err_rows(g, w)
    return e


def _hold(tag, normalize, got, stock):
    """print the case's line, then hold each error to max(tolerance, 4 x the stock float32 op's error)"""
    fmt = lambda e: " ".join(f"{k} {e[k]:.2e}" if k in e else f"{k} {'-':>8s}" for k in TOL)
    print(f"\n[corr shapes] {tag:34s} normalize={int(normalize)}  kernel: {fmt(got)}  | stock f32: {fmt(stock)}", end="")
    for k, v in got.items():
        lim = max(TOL[k], 4.0 * stock[k])
        assert v < lim, f"{tag} normalize={normalize}: {k} error {v:.3e}, limit {lim:.3e} (stock float32 op {stock[k]:.3e})"


def _case(tag, cam, mp, cot, normalize, res=None):
    want = _expr(cam, mp, cot, normalize, torch.float64)
    stock = _expr(cam, mp, cot, normalize, torch.float32)
    res = _kernel(cam, mp, cot, normalize) if res is None else res
    assert res[0].dtype == torch.float32 and res[0].shape == want[0].shape
    for g, w in zip(res[1:], want[1:]):
        assert g is not None and g.shape == w.shape
    _hold(tag, normalize, _errors(res, want, cam, mp, normalize), _errors(stock, want, cam, mp, normalize))
    return res, want, stock


# =====================================================================================================================
# shapes
# =====================================================================================================================
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("n,m,E,inst,why", ONE_PASS, ids=_ids(ONE_PASS))
def test_corr_one_pass_shapes(n, m, E, inst, why, normalize):
    """gram_mfma_kernel<FA, FB, NW> + finish_dist2_kernel, corr_bwd_slice_kernel<false> (n, m <= 64, E % 4 == 0)"""
    assert fwd_path(n, m, E) == inst and why(n, m, E)
    _case(f"one-pass {inst} ({n}, {m}, {E})", *_inputs(n, m, E), normalize)


# a normalised scalar is +-1 and has no gradient to be relative to: (1, 1, 1) runs on raw rows only
GENERAL_RUNS = [c + (nz,) for c in GENERAL for nz in (False, True) if not (c[:3] == (1, 1, 1) and nz)]


@pytest.mark.parametrize("n,m,E,why,normalize", GENERAL_RUNS, ids=[f"{i}-{c[-1]}" for i, c in zip(_ids(GENERAL_RUNS), GENERAL_RUNS)])
def test_corr_general_shapes(n, m, E, why, normalize):
    """rownorm_kernel, gram_kernel, finish_dist_kernel, corr_bwd_kernel on both sides (n or m > 64, or E % 4 != 0)"""
    assert fwd_path(n, m, E) == "general" and why(n, m, E)
    _case(f"general ({n}, {m}, {E})", *_inputs(n, m, E), normalize)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("n", [17, 40, 63])
def test_corr_one_tensor_as_both_sides_at_ragged_fragment_counts(n, normalize):
    """`same` register sharing in gram_mfma_kernel<2,2> / <4,4> and corr_bwd_slice_kernel<true> with nxp > nx; the
    gradient is the two sides' sum"""
    E = 1028
    assert fwd_path(n, n, E) == ("mfma<2,2>" if n <= 32 else "mfma<4,4>") and n % 16
    assert n % TB or n == 40                    # 17 and 63: the weights' rows in LDS are padded (nxp > nx)
    x, _, cot = _inputs(n, n, E)
    _case(f"one tensor ({n}, {n}, {E})", x, None, cot, normalize)


def test_corr_zero_rows_under_normalize():
    """cam row 3 and map row 7 all zero: F.normalize's eps = 1e-12 is their norm, their distances are exactly 2, their
    gradients are of order 1e12, and every other row holds the gradient of the case without the two rows"""
    n, m, E = 12, 20, 516
    assert fwd_path(n, m, E) == "mfma<2,2>"
    cam, mp, cot = _inputs(n, m, E)
    cam[3] = 0.0
    mp[7] = 0.0
    (D, dcam, dmap), want, stock = _case(f"zero rows ({n}, {m}, {E})", cam, mp, cot, True)
    assert (D[3] == 2.0).all() and (D[:, 7] == 2.0).all()
    assert (want[0][3] == 2.0).all() and (want[0][:, 7] == 2.0).all()
    assert want[1][3].abs().max() > 1e11 and want[2][7].abs().max() > 1e11
    # the same case without the two rows
    kc = [i for i in range(n) if i != 3]
    km = [j for j in range(m) if j != 7]
    sub = lambda r: (r[0][kc][:, km], r[1][kc], r[2][km])
    cam_r, mp_r, cot_r = cam[kc], mp[km], cot[kc][:, km]
    _, want_r, _ = _case(f"  without them ({n - 1}, {m - 1}, {E})", cam_r, mp_r, cot_r, True)
    _hold("  other rows against that case", True, _errors(sub((D, dcam, dmap)), want_r, cam_r, mp_r, True),
          _errors(sub(stock), want_r, cam_r, mp_r, True))


# =====================================================================================================================
# C ABI: pointers off the 16-byte grid
# =====================================================================================================================
GUARD = 12345.0


def _off4(t):
    """a device copy of t, 4 bytes past a 16-byte boundary, with guard values around it"""
    t = t.contiguous()
    buf = torch.full((t.numel() + 8,), GUARD, device=DEV, dtype=torch.float32)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _guards_intact(v):
    buf = v._base
    return buf[0].item() == GUARD and (buf[1 + v.numel():] == GUARD).all().item()


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("normalize", [False, True])
def test_corr_c_abi_every_operand_misaligned(normalize):
    """E % 4 != 0: no alignment contract on either call (the scalar paths with a real offset)"""
    L = _lib.lib()
    n, m, E = 9, 7, 1027
    assert fwd_path(n, m, E) == "general" and E % 4 != 0
    cam, mp, cot = _inputs(n, m, E)
    cg, mg, dD = _off4(cam), _off4(mp), _off4(cot)
    D, inc, inm = _off4(_nan(n, m)), _off4(_nan(n)), _off4(_nan(m))
    dcam, dmap = _off4(_nan(n, E)), _off4(_nan(m, E))
    assert L.bevr_corr_fwd(_p(cg), _p(mg), _p(D), _p(inc), _p(inm), n, m, E, int(normalize), _stream()) == 0
    assert L.bevr_corr_bwd(_p(cg), _p(mg), _p(D), _p(dD), _p(inc), _p(inm), _p(dcam), _p(dmap), n, m, E, int(normalize),
                           _stream()) == 0
    torch.cuda.synchronize()
    _case(f"C ABI all misaligned ({n}, {m}, {E})", cam, mp, cot, normalize, res=(D, dcam, dmap))
    assert all(_guards_intact(t) for t in (cg, mg, dD, D, inc, inm, dcam, dmap))
    assert torch.equal(cg.cpu(), cam) and torch.equal(mg.cpu(), mp)


@pytest.mark.parametrize("normalize", [False, True])
def test_corr_bwd_c_abi_misaligned_gradients_fall_to_the_general_kernels(normalize):
    """one forward, two backwards: all aligned (corr_bwd_slice_kernel) and dcam, dmap off the grid (corr_bwd_kernel twice)"""
    L = _lib.lib()
    n, m, E = 24, 40, 1024
    assert fwd_path(n, m, E) == "mfma<4,4>"
    cam, mp, cot = _inputs(n, m, E)
    cg, mg, dD = cam.to(DEV), mp.to(DEV), cot.to(DEV)
    D, inc, inm = _nan(n, m), _nan(n), _nan(m)
    assert all(t.data_ptr() % 16 == 0 for t in (cg, mg, dD, D, inc, inm))
    assert L.bevr_corr_fwd(_p(cg), _p(mg), _p(D), _p(inc), _p(inm), n, m, E, int(normalize), _stream()) == 0
    for tag, make in (("aligned", lambda *s: _nan(*s)), ("dcam, dmap misaligned", lambda *s: _off4(_nan(*s)))):
        dcam, dmap = make(n, E), make(m, E)
        assert dcam.data_ptr() % 16 == dmap.data_ptr() % 16 == (0 if tag == "aligned" else 4)
        assert L.bevr_corr_bwd(_p(cg), _p(mg), _p(D), _p(dD), _p(inc), _p(inm), _p(dcam), _p(dmap), n, m, E,
                               int(normalize), _stream()) == 0
        torch.cuda.synchronize()
        assert not torch.isnan(dcam).any() and not torch.isnan(dmap).any(), f"{tag}: NaN pre-fill left in a gradient"
        _case(f"C ABI bwd {tag} ({n}, {m}, {E})", cam, mp, cot, normalize, res=(D, dcam, dmap))
        if tag != "aligned":
            assert _guards_intact(dcam) and _guards_intact(dmap)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("n,m", [(24, 40), (65, 3)])
def test_corr_fwd_c_abi_misaligned_rows_of_whole_vectors_are_refused(n, m, normalize):
    L = _lib.lib()
    E = 1024
    cam, mp, _ = _inputs(n, m, E)
    for cg, mg in ((_off4(cam), mp.to(DEV)), (cam.to(DEV), _off4(mp))):
        D, inc, inm = _nan(n, m), _nan(n), _nan(m)
        assert L.bevr_corr_fwd(_p(cg), _p(mg), _p(D), _p(inc), _p(inm), n, m, E, int(normalize), _stream()) == E_ALIGN
        torch.cuda.synchronize()
        assert torch.isnan(D).all() and torch.isnan(inc).all() and torch.isnan(inm).all(), "a refused call wrote"


# =====================================================================================================================
# BEVR_GRAM_WAVES=4: gram_mfma_kernel<.., 4>, read once per process
# =====================================================================================================================
def test_gram_with_four_waves_in_a_child_process():
    env = dict(os.environ, BEVR_GRAM_WAVES="4")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider", __file__,
                        "-k", "test_corr_one_pass_shapes"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    lines = [l.replace("[corr shapes]", "[corr shapes, 4 waves]") for l in r.stdout.splitlines() if "[corr shapes]" in l]
    print("\n" + "\n".join(lines), end="")
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert f"{2 * len(ONE_PASS)} passed" in r.stdout and "failed" not in r.stdout, r.stdout[-1000:]
    assert len(lines) == 2 * len(ONE_PASS)


# =====================================================================================================================
# bevr_recall_rank, exact
# =====================================================================================================================
RANK_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000]


def _rank_ref(D):
    """rank[k] = #{i : D[i, k] < D[k, k]} on a float32 CPU matrix"""
    assert D.dtype == torch.float32 and D.device.type == "cpu"
    return (D < D.diagonal()[None, :]).sum(0).to(torch.int32)


def _rank_matrix(n, content):
    gen = torch.Generator().manual_seed(7919 * n + len(content))
    if content == "randn":
        return torch.randn(n, n, generator=gen)
    if content == "eight levels":
        return torch.randint(0, 8, (n, n), generator=gen).float() * 0.25 - 1.0
    D = torch.randn(n, n, generator=gen)                      # about 2 % NaN, +inf, -inf, some on the diagonal
    u = torch.rand(n, n, generator=gen)
    special = (float("nan"), float("inf"), float("-inf"))
    for k, v in enumerate(special):
        D[(u >= 0.007 * k) & (u < 0.007 * (k + 1))] = v
    for k, v in enumerate(special):
        if k < n:
            D[k, k] = v
        if n > 8:
            D[n - 1 - k, n - 1 - k] = v
    return D


@pytest.mark.parametrize("content", ["randn", "eight levels", "nan and inf"])
@pytest.mark.parametrize("n", RANK_SIZES)
def test_recall_rank_is_exact(n, content):
    D = _rank_matrix(n, content)
    ref = _rank_ref(D)
    if n >= 64:
        assert (ref >= 10).any(), "no rank beyond recall@10 in this input"
    if content == "eight levels" and n >= 64:
        ties = (D == D.diagonal()[None, :]).sum(0) - 1          # other entries of the column equal to its diagonal
        assert (ties > 0).any()
    if content == "nan and inf":
        d = D.diagonal()
        assert torch.isnan(d).any() and (n < 2 or torch.isinf(d).any())
        assert (ref[torch.isnan(d)] == 0).all()                 # a NaN compares false on both sides
    got = ops.recall_rank(D.to(DEV))
    assert got.dtype == torch.int32 and got.shape == (n,)
    assert torch.equal(got.cpu(), ref), (got.cpu() - ref).nonzero().flatten()[:10]


@pytest.mark.parametrize("n", [2, 65, 257])
def test_recall_rank_of_a_transposed_view(n):
    D = _rank_matrix(n, "randn").to(DEV)
    Dt = D.t()
    assert not Dt.is_contiguous() or n == 1
    ref = _rank_ref(D.cpu().t().contiguous())
    if n > 64:
        assert not torch.equal(ref, _rank_ref(D.cpu()))        # the buffer's own ranks are another answer
    assert torch.equal(ops.recall_rank(Dt).cpu(), ref)


@pytest.mark.parametrize("n", [64, 257])
def test_recall_rank_of_a_float64_matrix_is_that_of_its_float32_cast(n):
    gen = torch.Generator().manual_seed(n)
    # distinct in float64, many ties once cast to float32
    D64 = torch.randint(0, 8, (n, n), generator=gen).double() * 0.25 + 1e-10 * torch.randn(n, n, generator=gen, dtype=torch.float64)
    D32 = D64.float()
    ref = _rank_ref(D32)
    ref64 = (D64 < D64.diagonal()[None, :]).sum(0).to(torch.int32)
    assert not torch.equal(ref, ref64)
    got = ops.recall_rank(D64.to(DEV))
    assert got.dtype == torch.int32 and got.shape == (n,)
    assert torch.equal(got.cpu(), ref)
