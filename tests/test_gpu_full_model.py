"""G5: the full drop-in `BEVRender` (backbone -> history frame -> TSA/SCA encoder -> render decoder) on the HIP
kernels against the reference's own full model (tests/golden/full_bevrender.npz, made by make_golden_full.py).

The weights are not in the fixture (8 MB): both sides build them as this repo's model under the fixture's seed on
the CPU; the generator loaded them into the reference model with strict=True (452 identical state-dict entries).
"""
import importlib.util
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _gen():
    spec = importlib.util.spec_from_file_location("mgf", os.path.join(HERE, "golden", "make_golden_full.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_full_bevrender_matches_reference_forward_and_backward():
    from bevrender_amd.model.bevrender import BEVRender
    g = _gen()
    z = np.load(os.path.join(HERE, "golden", "full_bevrender.npz"))
    cfg = g.full_config()
    cfg["PRECISION"] = "f32"
    torch.manual_seed(int(z["seed"]))
    model = BEVRender(cfg, logging.getLogger("t"), "train")
    assert len(model.state_dict()) == int(z["n_state"])
    model = model.to("cuda")
    img, pose, vtype = g.full_inputs()
    out, _ = model(img.cuda(), pose.cuda(), vtype.cuda(), {}, False)
    assert tuple(out.shape) == tuple(z["out_shape"])
    out.sum().backward()
    torch.cuda.synchronize()
    got = out.detach().flatten().cpu()[torch.tensor(z["out_idx"])].numpy()
    # f32 kernels + MIOpen convolutions vs the reference's CPU convolutions: small float noise only
    np.testing.assert_allclose(got, z["out_val"], rtol=2e-3, atol=2e-3 * np.abs(z["out_val"]).max())
    assert abs(out.double().sum().item() - float(z["out_sum"])) <= 2e-3 * float(z["out_abs_sum"])
    ge = model.bev_embedding.weight.grad.flatten().cpu()[torch.tensor(z["gemb_idx"])].numpy()
    scale = np.abs(z["gemb_val"]).max()
    np.testing.assert_allclose(ge, z["gemb_val"], rtol=2e-2, atol=2e-2 * scale)


def test_full_bevrender_bf16_product_path_forward_and_backward():
    """The same golden on the BENCHED mode: bf16 operands (gather forward, slab and key-side backward), float backbone
    features and, second run, bf16-staged ones.  This fixture's rig pins 839 of SCA's 1960 keys, fewer than MIN_CELL_KEYS:
    there is no second key segment and NO tap kernel runs here (test_full_bevrender_conditioned below covers them).
    The reference is float32; the limits are the bf16 mode's (an untrained render CNN follows the encoder and amplifies the operands' 2^-9 rounding:
    compared in the 2-norm over the sampled entries, as tests/test_staging.py does)."""
    from bevrender_amd.model.bevrender import BEVRender
    g = _gen()
    z = np.load(os.path.join(HERE, "golden", "full_bevrender.npz"))
    for stage in (None, "bf16"):
        cfg = g.full_config()
        cfg["PRECISION"] = "bf16"
        cfg["STAGE_DTYPE"] = stage
        torch.manual_seed(int(z["seed"]))
        model = BEVRender(cfg, logging.getLogger("t"), "train").to("cuda")
        img, pose, vtype = g.full_inputs()
        out, _ = model(img.cuda(), pose.cuda(), vtype.cuda(), {}, False)
        out.float().sum().backward()
        torch.cuda.synchronize()
        got = out.detach().float().flatten().cpu()[torch.tensor(z["out_idx"])].numpy()
        ge = model.bev_embedding.weight.grad.float().flatten().cpu()[torch.tensor(z["gemb_idx"])].numpy()
        e_out = np.linalg.norm(got - z["out_val"]) / np.linalg.norm(z["out_val"])
        e_g = np.linalg.norm(ge - z["gemb_val"]) / np.linalg.norm(z["gemb_val"])
        e_sum = abs(out.double().sum().item() - float(z["out_sum"])) / float(z["out_abs_sum"])
        print(f"full model bf16 (stage {stage}): out {e_out:.3e} sum {e_sum:.3e} grad(embedding) {e_g:.3e}")
        assert np.isfinite(got).all() and np.isfinite(ge).all()
        assert e_out < OUT_LIMIT[stage] and e_sum < 2e-2 and e_g < GRAD_LIMIT[stage], (stage, e_out, e_sum, e_g)
        bad = [n for n, p in model.named_parameters() if p.grad is not None and not torch.isfinite(p.grad).all()]
        assert not bad, bad


# relative 2-norm limits of the bf16 product path against the float32 reference (written next to the test so that a
# reader sees what "bf16 limits" means here).  Output: ~2.5x the errors observed on MI355X (0.021-0.024).  Gradient of the
# embedding: this untrained model's keys have norms up to 160, its softmax rows are decided by near ties, and the error
# of the gradient -- not of the output -- depends on the ROUNDING REALISATION: scaling the static softmax reference's key
# bound (bevrender_amd/ops.py, `ub`; any value is a valid reference) over 0.8 ... 1.05 moved it between 0.105 and 0.289 with
# no trend (0.105, 0.163, 0.136, 0.244, 0.170, 0.127, 0.128), so a limit of 0.15 held only for one realisation
OUT_LIMIT = {None: 0.10, "bf16": 0.25}
GRAD_LIMIT = {None: 0.45, "bf16": 0.45}


# ---- the conditioned fixture: every mode, every gradient, limits from the reference's own rounding sensitivity ----
X3_ON = {"BEVR_GATHER_X3": "1", "BEVR_SLAB_X3": "1", "BEVR_TAP_X3": "1"}
REGION_16 = {"bevr_attn_gather_fwd", "bevr_attn_slab_bwd_q", "bevr_attn_bwd_k"}
TAP = {"bevr_attn_tap_fwd", "bevr_attn_tap_bwd_q", "bevr_attn_tap_bwd_k"}
CELL = {"bevr_attn_cell_fwd", "bevr_attn_cell_bwd_q", "bevr_attn_cell_bwd_k"}
X3_ENTRIES = {"bevr_attn_gather_fwd_x3", "bevr_attn_slab_bwd_q_x3"}
TILE_F32 = {"bevr_attn_fwd", "bevr_attn_bwd_q", "bevr_attn_bwd_k"}
# mode: (PRECISION, STAGE_DTYPE, switches, the yardstick's operand type, launches it must make, launches it must not make)
# -- timer names and C entry points, written out: what each mode is there to exercise
COND_MODES = {
    # the float modes: query-tile kernels for the scattered keys, cell kernels for the pinned ones
    "f32": ("f32", None, {}, "f32", TILE_F32 | CELL, TAP | X3_ENTRIES | {"bevr_attn_gather_fwd", "bevr_attn_slab_bwd_q"}),
    "bf16x3": ("bf16x3", None, {}, "f32", TILE_F32 | CELL, TAP | X3_ENTRIES | {"bevr_attn_gather_fwd", "bevr_attn_slab_bwd_q"}),
    # the split-bf16 kernel families behind their switches (the tap entry points take the mode from the descriptor)
    "bf16x3-split": ("bf16x3", None, X3_ON, "f32", X3_ENTRIES | {"bevr_attn_bwd_k"} | TAP, CELL),
    # the 16-bit modes: gather forward, slab and key-side backward, tap kernels for the pinned keys
    "bf16": ("bf16", None, {}, "bf16", REGION_16 | TAP, CELL | X3_ENTRIES),
    "bf16-stage": ("bf16", "bf16", {}, "bf16s", REGION_16 | TAP, CELL | X3_ENTRIES),
    "f16": ("f16", None, {}, "f16", REGION_16 | TAP, CELL | X3_ENTRIES),
}
_COND = []


def _cond_fixture():
    if not _COND:
        _COND.append(_gen().load_cond())
    return _COND[0]


@pytest.mark.parametrize("mode", list(COND_MODES))
def test_full_bevrender_conditioned(mode, monkeypatch):
    """The whole model against the reference's on the conditioned fixture (make_golden_full.py, gen_cond: BEV bound 50/50
    -- 1332 pinned keys, a second key segment --, weights conditioned by condition_, loss (out * cot).sum()): the output
    and EVERY parameter gradient, in every operand mode.  The limits come from the fixture, none from a GPU result: s_dt
    is how far the reference's own float32 result moves when what the kernels round and a module boundary exposes (K, V,
    Q, dO, the operands of the K | V GEMM; `bf16s`: also what STAGE_DTYPE stages) is rounded to dt, the largest over four
    realisations of that rounding; a mode may depart 3 s (the kernels round about twice as many operands: 2x;
    realisations beyond the four sampled: 1.5x), or the float32 test's own limits where those are larger (DESIGN.md
    section 3.1 has the measured figures).  A parameter whose gradient float32 rounding alone moves by 10 %
    (softmax-invariant proj_k biases, convolution
    biases in front of a train-mode batch norm) is `null`: only its size is bounded.  The step's launches are recorded and
    compared with the names written out in COND_MODES, so that the fixture cannot fall off the routes it is there for."""
    from bevrender_amd import ops
    from bevrender_amd.model.bevrender import BEVRender
    g, z = _gen(), _cond_fixture()
    prec, stage, env, dt, must, must_not = COND_MODES[mode]
    for k in X3_ON:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    launched = set()

    def recorder(name, flops, fn, *args, nbytes=0.0, tag=""):
        launched.update((name, getattr(fn, "__name__", repr(fn))))
        return fn(*args)
    monkeypatch.setattr(ops.KERNEL_TIMER, "run", recorder)

    cfg = g.cond_config()
    cfg["PRECISION"], cfg["STAGE_DTYPE"] = prec, stage
    torch.manual_seed(int(z["seed"]))
    model = BEVRender(cfg, logging.getLogger("t"), "train")
    g.condition_(model.state_dict())
    assert len(model.state_dict()) == int(z["n_state"])
    model = model.to("cuda")
    img, pose, vtype = g.full_inputs()
    out, _ = model(img.cuda(), pose.cuda(), vtype.cuda(), {}, False)
    assert tuple(out.shape) == tuple(z["out_shape"])
    (out.float() * g.cond_cotangent(out.shape).cuda()).sum().backward()
    torch.cuda.synchronize()
    got = out.detach().float().flatten().cpu()[torch.tensor(z["out_idx"])].numpy()
    e_out = g.rel2(got, z["out_val"])
    lim_out = 2e-3 if dt == "f32" else max(2e-3, 3.0 * float(z["s_out_" + dt]))
    params = dict(model.named_parameters())
    missing = [n for n in z["names"] if n not in params or params[n].grad is None]
    assert not missing, missing
    rows = []
    for i, n in enumerate(z["names"]):           # the fixture's order is the backward's: the first to depart localises
        v = params[n].grad.detach().float().flatten().cpu()[torch.tensor(z["idx"][i])].numpy()
        if z["null"][i]:
            err, lim, what = float(np.linalg.norm(v.astype(np.float64))), 10.0 * float(z["null_bound"][i]), "null |g|"
        else:
            err, lim, what = g.rel2(v, z["val"][i]), max(2e-2, 3.0 * float(z["s_" + dt][i])), "rel"
        line = f"  {i:3d} {n:90s} {what:8s} {err:.3e} limit {lim:.3e}{'' if err <= lim else '  FAIL'}"
        rows.append((err <= lim, line, err, lim))
    emb = rows[z["names"].index("bev_embedding.weight")]
    print(f"[{mode}] launched: {sorted(launched)}")
    print(f"[{mode}] per-parameter gradient errors in backward order:")
    print("\n".join(r[1] for r in rows))
    print(f"[{mode}] summary: out {e_out:.3e} limit {lim_out:.3e}; grad(embedding) {emb[2]:.3e} limit {emb[3]:.3e}; "
          f"{int(z['null'].sum())} of {len(rows)} parameters null")

    assert must <= launched, sorted(must - launched)
    assert not (must_not & launched), sorted(must_not & launched)
    assert np.isfinite(got).all()
    if dt == "f32":
        np.testing.assert_allclose(got, z["out_val"], rtol=2e-3, atol=2e-3 * np.abs(z["out_val"]).max())
    else:
        assert e_out <= lim_out, (mode, e_out, lim_out)
    nonfinite = [n for n, p in params.items() if p.grad is not None and not torch.isfinite(p.grad).all()]
    assert not nonfinite, nonfinite
    assert emb[3] <= 0.18                        # the point of the fixture: 0.45 on the unconditioned one
    bad = [r[1] for r in rows if not r[0]]
    assert not bad, f"{mode}: {len(bad)} gradients beyond their limit, in backward order:\n" + "\n".join(bad)
