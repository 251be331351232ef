"""The conditioned whole-model fixture without the representable-weights edit (tests/golden/full_bevrender_cond_w.npz,
made by make_golden_full_w.py) is what tests/test_gpu_kv_wsplit.py takes the whole-model limits of the split-weight
K | V source from.  Checked here, without a GPU, as tests/test_full_model_fixture_cpu.py checks the first fixture: it
belongs to this repository's model and rig, its proj_k / proj_v weights are NOT on the bf16 grid, and the reference's own
rounding sensitivities stored in it meet the generator's conditions."""
import importlib.util
import logging
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "full_bevrender_cond_w.npz")


def _load(name, fname):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", fname))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def gen():
    return _load("mgfw", "make_golden_full_w.py")


@pytest.fixture(scope="module")
def fix(gen):
    return gen.load_cond_w(PATH)


@pytest.fixture(scope="module")
def model(gen, fix):
    from bevrender_amd.model.bevrender import BEVRender
    torch.manual_seed(int(fix["seed"]))
    m = BEVRender(gen.mgf.cond_config(), logging.getLogger("t"), "train")
    before = {k: v.clone() for k, v in m.state_dict().items()}
    gen.condition_w_(m.state_dict())
    return m, before


def test_state_dict_and_conditioning(gen, fix, model):
    m, before = model
    sd = m.state_dict()
    base = _load("mgf0", "make_golden_full.py")          # the first fixture's generator, untouched by this one's flag
    assert base.COND_ROUND_W is True and gen.mgf.COND_ROUND_W is False
    assert len(sd) == int(fix["n_state"]) and not bool(fix["round_w"])
    assert float(fix["cond_scale"]) == base.COND_SCALE and int(fix["cot_seed"]) == base.COT_SEED
    assert float(fix["cond_out_scale"]) == base.COND_OUT_SCALE and int(fix["seed"]) == base.SEED
    # edits 1 and 3 of condition_, and nothing else: the proj_k / proj_v weights keep their low bits
    want, touched, off_grid = {}, [], 0
    for k, v in before.items():
        w = v.clone()
        if k.endswith(".proj_k.weight") or k.endswith(".proj_k.bias"):
            w = w * base.COND_SCALE
        if k.endswith("_deform_attn.proj_out.weight") or k.endswith("_deform_attn.proj_out.bias"):
            w = w * base.COND_OUT_SCALE
        if k.endswith(".proj_k.weight") or k.endswith(".proj_v.weight"):
            assert not torch.equal(sd[k].to(torch.bfloat16).float(), sd[k]), k
            # most of a seeded weight's entries are off the bf16 grid (8 of 24 significand bits)
            assert (sd[k].to(torch.bfloat16).float() != sd[k]).float().mean().item() > 0.9, k
            off_grid += 1
        want[k] = w
        if not torch.equal(w, v):
            touched.append(k)
    assert off_grid == 4
    assert all(torch.equal(sd[k], want[k]) for k in sd)
    assert len(touched) == 4 and all("_deform_attn.proj_" in k and k.endswith(".weight") for k in touched), touched
    assert all(torch.equal(p, sd[n]) for n, p in m.named_parameters())
    # the same model as the first fixture's up to that edit: its conditioning moves these weights by at most half a bf16 ulp
    m0 = {k: v.clone() for k, v in before.items()}
    base.condition_(m0)
    for k in sd:
        if k.endswith(".proj_k.weight") or k.endswith(".proj_v.weight"):
            assert ((m0[k] - sd[k]).abs() <= 2.0 ** -8 * sd[k].abs()).all()     # 8 significand bits
        else:
            assert torch.equal(m0[k], sd[k]), k


def test_same_rig_as_the_first_fixture(gen, fix):
    from bevrender_amd.model.SCA import MIN_CELL_KEYS
    first = gen.mgf.load_cond()
    pinned = gen.mgf.pinned_keys(gen.mgf.cond_config())
    assert pinned == [int(p) for p in fix["pinned"]] == [int(p) for p in first["pinned"]]
    assert min(pinned) >= MIN_CELL_KEYS
    assert fix["names"] == first["names"] and tuple(fix["out_shape"]) == tuple(first["out_shape"])
    assert (fix["out_idx"] == first["out_idx"]).all() and all((a == b).all() for a, b in zip(fix["idx"], first["idx"]))
    # another model all the same: the weights differ in their low bits, so do the reference's results -- a little
    assert not np.array_equal(fix["out_val"], first["out_val"])
    assert gen.mgf.rel2(fix["out_val"], first["out_val"]) < 1e-2


def test_yardstick_conditions(gen, fix):
    emb, med, n_null, loud = gen.cond_w_conditions(fix)
    print(f"s_bf16: embedding {emb:.3e} median {med:.3e}; {n_null} null; {len(loud)} parameters with 3 s > {gen.W_REPORT_3S}:")
    for n, s in loud:
        print(f"  {n} s_bf16 {s:.3e}")
    assert emb <= gen.W_LIMIT_EMB == 0.06
    assert med <= gen.W_LIMIT_MEDIAN == 0.06
    assert n_null <= gen.W_MAX_NULL == 25
    assert (fix["null"] == (fix["s_f32"] > gen.mgf.NULL_S_F32)).all() and gen.mgf.NULL_S_F32 == 0.1
    for k in ("s_f32", "s_bf16", "s_f16", "null_bound", "norm"):
        assert np.isfinite(fix[k]).all() and (fix[k] >= 0).all(), k
    for k in ("s_out_f32", "s_out_bf16", "s_out_f16"):
        assert 0 < float(fix[k]) < 1e-2, k
    # the output's limit in the GPU test is max(2e-3, 3 s_out): the floor decides in both 16-bit modes, which is what
    # makes the switch-off run (rounded weights: 2.8e-3 with the same rounding hooked into the reference) miss it
    assert 3.0 * float(fix["s_out_bf16"]) < 2e-3 and 3.0 * float(fix["s_out_f16"]) < 2e-3
    i = fix["names"].index("bev_embedding.weight")
    assert not fix["null"][i]
    assert max(3.0 * float(fix[k][i]) for k in ("s_f32", "s_bf16", "s_f16")) <= 0.18
    # the worst parameters are not capped, but they are known: SCA's offset head, whose gradient passes through the
    # sampling positions of every key
    assert all(".spatial_deform_attn.conv_offset_m0." in n for n, _ in loud), loud
    assert not [n for n, s, nul in zip(fix["names"], fix["s_f16"], fix["null"]) if not nul and 3.0 * s > gen.W_REPORT_3S]


def test_every_parameter_is_in_the_fixture_or_has_no_gradient(fix, model):
    m, _ = model
    params = dict(m.named_parameters())
    names = fix["names"]
    assert len(set(names)) == len(names) and set(names) <= set(params)
    assert sorted(set(params) - set(names)) == sorted(str(n) for n in fix["no_grad_names"])
    assert "bev_embedding.weight" in names and any(".rpe_table" in n for n in names)
    for i, n in enumerate(names):
        numel = params[n].numel()
        idx = fix["idx"][i]
        assert len(idx) == min(numel, 64) == len(fix["val"][i]) and len(set(idx.tolist())) == len(idx)
        assert 0 <= idx.min() and idx.max() < numel
        assert np.linalg.norm(fix["val"][i].astype(np.float64)) <= float(fix["norm"][i]) * (1 + 1e-6)


def test_file_size(gen):
    assert os.path.getsize(PATH) <= gen.mgf.COND_MAX_BYTES == 400 * 1000
