"""Tap forward (csrc/attn_tap_fwd.hip, one and two channel groups): the EXACT pass -- the recompute of flagged columns with
an online maximum -- in every instantiation, the flags themselves against a float64 prediction, and fp16 rows whose static
bound is loose enough that every weight is an fp16 subnormal.  The reference is the float64 restatement of
tools/tap_check.py / tools/tap_g2_check.py on the operands as the kernels round them (`mimic`); the limits are those of
tests/test_gpu_tap.py::test_tap_forward_recomputes_rows_whose_weights_underflow_the_static_reference: Rn 2e-3, LSE 1e-2 in
log2 units.  The backward entry points take the LSE as an operand and never see the flags: their tests are the
float64-definition tests of tests/test_gpu_tap.py and tests/test_gpu_tap_groups.py.
All draws come from a host generator (host_rng): the conditions on the reference hold on any machine."""
import math
import os
import sys

import pytest
import torch

from bevrender_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu
BF16, F16 = _lib.PREC_BF16, _lib.PREC_F16
LIM_RN, LIM_LSE = 2e-3, 1e-2
FLAG_LOG2 = math.log2(7.9e-31)          # the forward flags a column that holds a row whose sum is under 7.9e-31


def _check(groups, name, **kw):
    import tap_check
    import tap_g2_check
    return (tap_g2_check if groups == 2 else tap_check).check_case(name, forward_only=True, host_rng=True, **kw)


def _quartiles(x):
    q = torch.quantile(x.flatten().double(), torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0], dtype=torch.float64))
    return [round(v, 1) for v in q.tolist()]


# ---- A1. every column flagged: the EXACT instantiation of NB = 1, 2, 4 in both 16-bit modes -------------------------
# S = 16 / 120 / 232: 1 / 8 / 15 row blocks per column = NB 1 / 2 / 4 (csrc/attn_tap_fwd.hip, launch)
A1_SIZES = {"nb1": (16, 3, 4), "nb2": (120, 2, 8), "nb4": (232, 2, 9)}        # S, D, seed


@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("size", list(A1_SIZES))
@pytest.mark.parametrize("groups", [1, 2])
def test_exact_pass_of_every_instantiation_with_all_columns_flagged(groups, size, prec):
    """bf16: logit scale 200 (the one-group NB = 1 case of tests/test_gpu_tap.py, here for every NB and for two groups,
    where the recompute rescales a second accumulator).  fp16 at headroom 8: a logit scale alone cannot push EVERY row's
    weights under fp16's range -- a row whose 12 taps are all negative has a bound of ~0 and keys of weight 0 whose logit is
    ~0 (one row in 4096) -- so the bound is set by a logit no key has: G's slot of pixel (3, 2) = 128 at logit scale 8
    (tap_check.UNSEEN_TAP; the mechanism of test_tap_path_with_a_loose_logit_bound_takes_the_exact_pass).  The float64
    reference then puts every row's largest weight under 2^-30 (asserted), fp16 holds nothing under 2^-25, every row sum
    is 0 and every column is flagged."""
    S, D, seed = A1_SIZES[size]
    h = groups                  # one head per group (one group: h = 1, as KERNEL_CASES' multi-block cases)
    kw = dict(P=1, h=h, S=S, N=313, Wt=2 * S * D - 1, spread=(12.0, 30.0), sort=False, seed=seed)
    if prec == F16:
        kw.update(prec=F16, headroom=8.0, gscale=8.0, unseen=128.0)
    else:
        kw.update(gscale=200.0)
    r = _check(groups, f"A1 g{groups} {size} prec{prec}", **kw)
    rows = r["mimic_rows"]
    if prec == F16:
        assert r["finite_G"]
        top = (8.0 - rows["slack"]).max().item()        # log2 of the largest weight of any row against mref
        print(f"fp16: largest weight of any row 2^{top:.1f}")
        assert top < -30.0
    else:
        # (the reference's own statement that the case is what it claims: every column holds an underflowed row)
        assert bool((rows["lsum_log2"] < FLAG_LOG2 - 2).any(-1).all())
    print(f"A1 groups {groups} {size} prec {prec}: flagged {r['flagged']} of {h * S}  Rn {r['mimic'][0]:.2e}  LSE {r['mimic'][1]:.2e}  "
          f"slack quartiles {_quartiles(rows['slack'])}")
    assert r["flagged"] == 1 * h * S
    assert r["dead"] == 0.0
    assert r["mimic"][0] < LIM_RN and r["mimic"][1] < LIM_LSE, r["mimic"]


# ---- A2. some columns flagged, healthy and underflowed rows inside one column --------------------------------------
@pytest.mark.parametrize("groups", [1, 2])
def test_flags_equal_the_float64_prediction_and_unflagged_columns_stay(groups):
    """Logit scale 200 on the rows i = 0 and 12 of every odd BEV column, 4 elsewhere (tap_check.mixed_rows).  The float64
    reference says which columns hold a row whose sum against mref is under 7.9e-31; a column whose verdict hangs on a row
    within 2 binades of that threshold is left out (the kernel's weights are bf16, its sum float).  The flags equal the
    prediction, and EVERY row -- recomputed or not, beside a recomputed one or not -- meets the limits: the EXACT launch
    rewrites R and mref of the flagged columns alone."""
    import tap_check
    h = 2 * groups
    r = _check(groups, f"A2 g{groups}", P=1, h=h, S=24, N=500, Wt=2 * 24 * 3 - 1, seed=11,
               row_scale=tap_check.mixed_rows(200.0, 4.0, every=12))
    ls = r["mimic_rows"]["lsum_log2"]                                  # (P, h, j, i)
    yes = (ls < FLAG_LOG2 - 2).any(-1)
    no = (ls > FLAG_LOG2 + 2).all(-1)
    undecided = ~yes & ~no
    flags = r["flags"].bool()
    print(f"A2 groups {groups}: columns {yes.numel()}  predicted flagged {int(yes.sum())} clear {int(no.sum())} "
          f"undecided {int(undecided.sum())}  kernel flagged {int(flags.sum())}  Rn {r['mimic'][0]:.2e}  LSE {r['mimic'][1]:.2e}")
    assert yes.any() and no.any()
    assert undecided.float().mean().item() <= 0.10
    assert torch.equal(flags[yes | no], yes[yes | no]), (flags & no).nonzero().tolist() + (~flags & yes).nonzero().tolist()
    assert r["dead"] == 0.0
    assert r["mimic"][0] < LIM_RN and r["mimic"][1] < LIM_LSE, r["mimic"]


# ---- A3. fp16 rows between healthy and flagged ----------------------------------------------------------------------
A3_SCALES = (2.0, 4.0, 8.0, 16.0, 20.0, 32.0, 64.0)       # (20: the one-group case's scale with a quarter of the rows in the gap)
_a3 = {}


def _a3_case(groups, gscale):
    key = (groups, gscale)
    if key not in _a3:
        _a3[key] = _check(groups, f"A3 g{groups} x{gscale:g}", P=1, h=2, S=24, N=400, Wt=2 * 24 * 3 - 1, seed=5, prec=F16,
                          gscale=gscale, headroom=8.0)
    return _a3[key]


@pytest.mark.parametrize("gscale", A3_SCALES)
@pytest.mark.parametrize("groups", [1, 2])
def test_fp16_rows_whose_weights_are_all_subnormal(groups, gscale):
    """fp16 at headroom 8: a row whose bound is 22 .. 33 binades loose (slack = mref + headroom - the row's largest logit,
    from the reference) has its largest weight at 2^-14 .. 2^-25: fp16 subnormals of 10 .. 0 significant bits, and a row
    sum far above the 7.9e-31 that flags a column.  Whatever the kernel flags, every row meets the limits the bf16 flagged
    test holds with coarser operands."""
    r = _a3_case(groups, gscale)
    sl = r["mimic_rows"]["slack"]
    gap = ((sl >= 22) & (sl <= 33)).float().mean().item()
    print(f"A3 groups {groups} scale {gscale:g}: slack quartiles {_quartiles(sl)}  rows at slack 22..33 {gap:.3f}  "
          f"flagged {r['flagged']} of {r['flags'].numel()}  Rn {r['mimic'][0]:.2e}  LSE {r['mimic'][1]:.2e}  dead {r['dead']:.1e}")
    assert r["finite_G"]
    assert r["dead"] == 0.0
    assert r["mimic"][0] < LIM_RN and r["mimic"][1] < LIM_LSE, r["mimic"]


@pytest.mark.parametrize("groups", [1, 2])
def test_fp16_gap_cases_reach_the_gap(groups):
    """a condition on the reference alone: at one scale at least a quarter of the rows sits at slack 22 .. 33"""
    best = max(((_a3_case(groups, s)["mimic_rows"]["slack"] >= 22) & (_a3_case(groups, s)["mimic_rows"]["slack"] <= 33))
               .float().mean().item() for s in A3_SCALES)
    assert best >= 0.25, best
