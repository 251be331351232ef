"""The conditioned whole-model fixture (tests/golden/full_bevrender_cond.npz, made by make_golden_full.py: gen_cond) is
what tests/test_gpu_full_model.py takes every limit from.  Checked here, without a GPU: it still belongs to this
repository's model and rig, it still puts the pinned keys on a second key segment, and the reference's own rounding
sensitivities stored in it still meet the conditions that make those limits tight."""
import importlib.util
import logging
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "full_bevrender_cond.npz")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("mgf", os.path.join(HERE, "golden", "make_golden_full.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def fix(gen):
    return gen.load_cond(PATH)


@pytest.fixture(scope="module")
def model(gen, fix):
    from bevrender_amd.model.bevrender import BEVRender
    torch.manual_seed(int(fix["seed"]))
    m = BEVRender(gen.cond_config(), logging.getLogger("t"), "train")
    before = {k: v.clone() for k, v in m.state_dict().items()}
    gen.condition_(m.state_dict())
    return m, before


def test_state_dict_and_conditioning(gen, fix, model):
    m, before = model
    sd = m.state_dict()
    assert len(sd) == int(fix["n_state"])
    assert float(fix["cond_scale"]) == gen.COND_SCALE and int(fix["cot_seed"]) == gen.COT_SEED
    assert float(fix["cond_out_scale"]) == gen.COND_OUT_SCALE
    # in place, on the model's own tensors (the biases start at 0): TSA's and SCA's key projection x COND_SCALE, their
    # output projection x COND_OUT_SCALE, the proj_k / proj_v weights then on bf16-representable values; nothing else
    want, touched = {}, []
    for k, v in before.items():
        w = v.clone()
        if k.endswith(".proj_k.weight") or k.endswith(".proj_k.bias"):
            w = w * gen.COND_SCALE
        if k.endswith("_deform_attn.proj_out.weight") or k.endswith("_deform_attn.proj_out.bias"):
            w = w * gen.COND_OUT_SCALE
        if k.endswith(".proj_k.weight") or k.endswith(".proj_v.weight"):
            w = w.to(torch.bfloat16).float()
            assert torch.equal(sd[k].to(torch.bfloat16).float(), sd[k])
        want[k] = w
        if not torch.equal(w, v):
            touched.append(k)
    assert all(torch.equal(sd[k], want[k]) for k in sd)
    assert len(touched) == 6 and all("_deform_attn.proj_" in k and k.endswith(".weight") for k in touched), touched
    assert all(torch.equal(p, sd[n]) for n, p in m.named_parameters())


def test_pinned_keys_form_a_second_segment(gen, fix):
    from bevrender_amd.model.SCA import MIN_CELL_KEYS
    pinned = gen.pinned_keys(gen.cond_config())
    assert pinned == [int(p) for p in fix["pinned"]]
    assert min(pinned) >= MIN_CELL_KEYS
    # and the unconditioned fixture's rig does not: why this fixture exists
    assert max(gen.pinned_keys(gen.full_config())) < MIN_CELL_KEYS


def test_yardstick_conditions(gen, fix):
    emb, med, n_null, worst3 = gen.cond_conditions(fix)
    print(f"s_bf16: embedding {emb:.3e} median {med:.3e}; {n_null} null; 3 x worst {worst3:.3e}")
    assert emb <= gen.COND_LIMIT_EMB == 0.06
    assert med <= gen.COND_LIMIT_MEDIAN == 0.06
    assert n_null <= gen.COND_MAX_NULL == 25
    assert worst3 <= gen.COND_LIMIT_WORST3 == 0.45
    assert (fix["null"] == (fix["s_f32"] > gen.NULL_S_F32)).all() and gen.NULL_S_F32 == 0.1
    # every stored sensitivity is a finite number, and the 16-bit ones are no smaller than float32's floor allows
    for k in ("s_f32", "s_bf16", "s_f16", "s_bf16s", "null_bound", "norm"):
        assert np.isfinite(fix[k]).all() and (fix[k] >= 0).all(), k
    for k in ("s_out_f32", "s_out_bf16", "s_out_f16", "s_out_bf16s"):
        assert 0 < float(fix[k]) < 1e-2, k
    # the GPU test's embedding-gradient limit in every mode: 3 s, at most 0.18 (0.45 on the unconditioned fixture)
    i = fix["names"].index("bev_embedding.weight")
    assert not fix["null"][i]
    assert max(3.0 * float(fix[k][i]) for k in ("s_f32", "s_bf16", "s_f16", "s_bf16s")) <= 0.18


def test_every_parameter_is_in_the_fixture_or_has_no_gradient(fix, model):
    m, _ = model
    params = dict(m.named_parameters())
    names = fix["names"]
    assert len(set(names)) == len(names) and set(names) <= set(params)
    # the rest: parameters the reference's backward never reached (modules its forward does not use, kept for
    # state-dict parity), recorded by name
    assert sorted(set(params) - set(names)) == sorted(str(n) for n in fix["no_grad_names"])
    assert "bev_embedding.weight" in names and any(".rpe_table" in n for n in names)
    for i, n in enumerate(names):
        numel = params[n].numel()
        idx = fix["idx"][i]
        assert len(idx) == min(numel, 64) == len(fix["val"][i]) and len(set(idx.tolist())) == len(idx)
        assert 0 <= idx.min() and idx.max() < numel
        assert np.linalg.norm(fix["val"][i].astype(np.float64)) <= float(fix["norm"][i]) * (1 + 1e-6)


def test_file_size(gen):
    assert os.path.getsize(PATH) <= gen.COND_MAX_BYTES == 400 * 1000
