"""The split-bf16 mode (BEVR_PREC_BF16X3) on the tap entry points, the parts that need no GPU: the library's exports, the
routing switch, the host-side operand builder against the header's words in float64, and a census of the d(pos) kinks
of every key set the GPU tests (tests/test_gpu_tap_x3.py) judge with the kink rule."""
import ctypes as C
import os
import sys

import pytest
import torch

from bevrender_amd import _lib, ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

X3 = _lib.PREC_BF16X3
P = C.c_void_p(0x10000)          # a 16-byte aligned, never dereferenced "device pointer"

# the key sets of tests/test_gpu_tap_x3.py (imported there): tap_check.make_case arguments, drawn with host_rng=True so
# that the census below sees the same keys without a GPU.  nb4: S > 224, the NB = 4 instantiations
from test_gpu_tap import KERNEL_CASES, TAP_CFGS, _tap_problem  # noqa: E402  (nothing there touches the GPU on import)

X3_KERNEL_CASES = {k: KERNEL_CASES[k] for k in ("sorted", "ragged", "unsorted_wide", "three_row_blocks")}
# 15 row blocks per column: 4 per wave.  The cotangent lives on every tenth BEV column (h_cols): with all 232 compared
# columns nearly every key would be within 2e-3 of SOME column's kink and the d(pos) comparison would be vacuous
X3_KERNEL_CASES["nb4"] = dict(P=1, h=1, S=232, N=96, Wt=2 * 232 * 2 - 1, seed=6, h_cols=list(range(3, 232, 10)))
KINK = 2e-3          # the neighbourhood of a kink (tests/test_gpu_fullsize.py:check_dpos)
CAP = 0.02           # at most this share of the keys may miss the limit, all of them inside the neighbourhood


def test_library_exports_what_the_binding_binds():
    L = _lib.lib()
    for name in _lib.SYMBOLS:
        assert hasattr(L, name), name
    assert L.bevr_abi_version() == _lib.ABI_VERSION == 6


def _desc(**over):
    d = ops.AttnGeom(n_prob=2, q_div=1, heads=2, groups=1, S=12, N=100, Wt=71, precision=X3).desc()
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_refusals_stay_and_prep_does_not_look_at_the_precision():
    """Nothing is launched here (fake pointers, the checks come first): the dropout tap entry points refuse the split mode,
    the plain ones keep refusing BEVR_PREC_F32 (BEVR_E_PRECISION = -3); bevr_attn_tap_ws_bytes gives one size for every
    precision and bevr_attn_tap_prep reaches its NULL check with the split-mode descriptor."""
    L = _lib.lib()
    r = C.byref(_desc())
    assert L.bevr_attn_tap_fwd_dropout(r, P, P, P, P, P, P, P, 0, 100, 1, None) == -3
    assert L.bevr_attn_tap_bwd_q_dropout(r, P, P, P, P, P, P, 0, 100, 1, None) == -3
    assert L.bevr_attn_tap_bwd_k_dropout(r, P, P, P, P, P, P, P, P, 0, 100, 1, None) == -3
    f32 = C.byref(_desc(precision=_lib.PREC_F32))
    assert L.bevr_attn_tap_fwd(f32, P, P, P, P, P, P, None) == -3
    assert L.bevr_attn_tap_bwd_q(f32, P, P, P, P, P, P, None) == -3
    assert L.bevr_attn_tap_bwd_k(f32, P, P, P, P, P, P, P, P, None) == -3
    sizes = {p: L.bevr_attn_tap_ws_bytes(C.byref(_desc(precision=p))) for p in (_lib.PREC_F32, _lib.PREC_BF16, _lib.PREC_F16, X3)}
    assert len(set(sizes.values())) == 1 and sizes[X3] > 0
    assert L.bevr_attn_tap_prep(r, P, P, P, P, None, None) == -1          # NULL workspace, whatever the precision


def test_tap_supported_and_its_switch(monkeypatch):
    monkeypatch.delenv("BEVR_TAP", raising=False)
    monkeypatch.delenv("BEVR_TAP_X3", raising=False)
    assert ops.tap_supported(X3, 1) == (ops.TAP_X3_DEFAULT != "0")      # unset: the default the measurement decided
    monkeypatch.setenv("BEVR_TAP_X3", "1")
    assert ops.tap_supported(X3, 1)
    assert not ops.tap_supported(X3, 2)
    assert not ops.tap_supported(X3, 1, dropout=True)          # the tap dropout kernels are 16-bit only
    assert ops.tap_supported(_lib.PREC_BF16, 1, dropout=True)
    assert not ops.tap_supported(_lib.PREC_F32, 1)
    monkeypatch.setenv("BEVR_TAP_X3", "0")
    assert not ops.tap_supported(X3, 1)
    assert ops.tap_supported(_lib.PREC_BF16, 1) and ops.tap_supported(_lib.PREC_F16, 1)      # the 16-bit routes stay
    monkeypatch.setenv("BEVR_TAP_X3", "1")
    monkeypatch.setenv("BEVR_TAP", "0")
    assert not ops.tap_supported(X3, 1)


def _parts64(x):
    """The header's words in float64 arithmetic on bf16-rounded values: successive bf16 parts of x."""
    r, out = x.double(), []
    for _ in range(4):
        p = r.float().to(torch.bfloat16).double()
        out.append(p)
        r = r - p
    return out


@pytest.mark.parametrize("scale", [1e-6, 1.0, 37.5, 3.0e4])
def test_operand_builder_follows_the_header(scale):
    """ops.tap_split_rows against include/bevrender_hip.h ("TAP entry points in BEVR_PREC_BF16X3"): slots 0..11 hi =
    bf16(x), lo = bf16(x - hi) and hi + lo = x to 2^-16 relative; the offset in four parts over slots 12, 13, their sum
    the float itself; slot 14 (dead, 0); slot 15 zero."""
    import tap_check
    gen = torch.Generator().manual_seed(int(scale * 7) % 1000 + 1)
    rows = torch.randn(3, 2, 40, 12, generator=gen) * scale
    c = torch.randn(3, 2, 40, generator=gen) * scale * 10 - 64.0
    planes, c_eff = ops.tap_split_rows(rows, c, dead=-1.0e30)
    assert planes.shape == (2, 3, 2, 40, 16) and planes.dtype == torch.bfloat16 and planes.is_contiguous()
    p = _parts64(rows)
    assert torch.equal(planes[0][..., :12].double(), p[0]) and torch.equal(planes[1][..., :12].double(), p[1])
    got = planes[0][..., :12].double() + planes[1][..., :12].double()
    assert ((got - rows.double()).abs() <= 2.0 ** -16 * rows.double().abs()).all()
    q = _parts64(c)
    for (pl, slot), want in zip(((0, 12), (1, 12), (0, 13), (1, 13)), q):
        assert torch.equal(planes[pl][..., slot].double(), want), (pl, slot)
    total = sum(planes[pl][..., s].double() for pl in (0, 1) for s in (12, 13))
    assert torch.equal(total, c.double())                      # four bf16 parts hold the float exactly
    assert torch.equal(c_eff.double(), c.double())
    assert (planes[0][..., 14].float() == torch.tensor(-1.0e30).to(torch.bfloat16).float()).all()
    assert (planes[1][..., 14] == 0).all() and (planes[..., 15] == 0).all()
    # the tool's builder, written from the header alone, gives the same bits
    r16 = torch.zeros(3, 2, 40, 16)
    r16[..., :12] = rows
    hp, hc = tap_check.header_split(r16, c, dead=-1.0e30)
    assert torch.equal(hp.view(torch.int16), planes.view(torch.int16)) and torch.equal(hc, c_eff)
    # a padding row's offset (-1e30) survives as a finite number
    _, ce = ops.tap_split_rows(rows[:1, :1, :1], torch.full((1, 1, 1), -1.0e30), 0.0)
    assert torch.isfinite(ce).all() and ce.item() < -9e29


def kink_shares(a, b, ys, xs, S, Wt, cols=None):
    """Per key set, in float64: (share of keys within KINK of a kink that does not depend on the BEV column -- an integer
    crossing of a_n or of the sampling position ys / xs --, share within KINK of ANY kink including j rx + b_n over the
    compared columns, per-key distance to the nearest kink)."""
    a, b, ys, xs = (t.double() for t in (a, b, ys, xs))
    rx = (Wt - 1) / (2.0 * (S - 1))
    fixed = torch.minimum((a - a.round()).abs(), torch.minimum((ys - ys.round()).abs(), (xs - xs.round()).abs()))
    dist = fixed.clone()
    for j in (range(S) if cols is None else sorted(set(int(c) for c in cols))):
        t = b + j * rx
        dist = torch.minimum(dist, (t - t.round()).abs())
    return (fixed < KINK).double().mean().item(), (dist < KINK).double().mean().item(), dist


def test_kink_census_of_the_gpu_tests_key_sets():
    """The GPU tests excuse a key that misses the d(pos) limit only if it lies within 2e-3 of a kink, and at most 2 % of
    the keys.  What can be checked without a GPU is that this rule has teeth on the key sets used: computed in float64
    from the same inputs (host_rng draws),
      * the keys near a kink of their OWN coordinates (a_n, ys, xs: the same for every BEV column) are under the 2 % cap,
      * the keys away from every kink, the compared columns' j rx + b_n included, are at least 30 % (check_dpos's
        min_clean): the limit binds on them without exception.
    The share within 2e-3 of a kink of SOME compared column cannot itself be under 2 %: every compared column j adds its
    own 4e-3-wide band of b_n (S columns: ~0.4 S % of the keys, 8-15 % at S = 18..40; the sampled-row tests of
    tests/test_gpu_fullsize.py meet the same with min_clean).  It is printed."""
    import tap_check
    for name, kw in X3_KERNEL_CASES.items():
        gen = torch.Generator().manual_seed(kw.get("seed", 0))
        a, b, ys, xs = tap_check.draw_keys(kw["P"], kw["S"], kw["N"], kw["Wt"], kw.get("spread", (5.0, 2.5)),
                                           kw.get("sort", True), gen)
        own, anyk, dist = kink_shares(a, b, ys, xs, kw["S"], kw["Wt"], kw.get("h_cols"))
        print(f"[census {name}] own-coordinate kinks {own:.4f}, any compared column {anyk:.4f}")
        assert own < CAP, (name, own)
        assert 1.0 - anyk >= 0.3, (name, anyk)
    for cfg in TAP_CFGS:
        B, V, Cc, h, S, D, Hi, Wi, n_pin = cfg
        pos, split = _tap_problem(*cfg, seed=sum(cfg))[4:7:2]
        pin = pos[:, split:].double()
        Wt = 2 * S * D - 1
        a = (1 - pin[..., 0]) * (S - 1) / 2
        b = (1 - pin[..., 1]) * (Wt - 1) / 4
        ys, xs = (pin[..., 0] + 1) * 0.5 * (Hi - 1), (pin[..., 1] + 1) * 0.5 * (Wi - 1)
        own, anyk, _ = kink_shares(a, b, ys, xs, S, Wt)
        print(f"[census cfg {cfg}] own-coordinate kinks {own:.4f}, any compared column {anyk:.4f}")
        assert own < CAP, (cfg, own)
        assert 1.0 - anyk >= 0.3, (cfg, anyk)
