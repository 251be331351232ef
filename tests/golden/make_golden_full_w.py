#!/usr/bin/env python3
"""G5w: the conditioned whole-model fixture WITHOUT the representable-weights edit (full_bevrender_cond_w.npz).

make_golden_full.py's conditioned fixture moves the proj_k / proj_v weights onto bf16-representable values (condition_,
edit 2), because the fused K | V kernel rounds its GEMM's weights and that error, common to all keys, would swamp the
test.  With BEVR_KV_WSPLIT=1 the kernel takes the weights as hi + lo planes (bevr_kv_project_w2) and the edit is not
needed: this fixture keeps the seeded weights' low bits (edits 1 and 3 only) and its yardstick rounds what the
split-weight kernel rounds -- Q and dO (yardstick_hooks' sites "q" and "o"), the K | V GEMM's feature operand (forward
only) and the K / V outputs with their cotangents -- with the weights left exact.

Run ONLY where the reference model's checkout is, with its directory as the argument:
    python tests/golden/make_golden_full_w.py <reference checkout>
Everything else -- rig, seeds, inputs, cotangent, the rounding realisations, the stored format (load_cond) -- is
make_golden_full.py's, loaded by path; that generator and its fixture stay as they are.
"""
import importlib.util
import logging
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH_W = os.path.join(HERE, "full_bevrender_cond_w.npz")
# the yardsticks of this fixture: the 16-bit modes the split-weight kernel has, and float32 (which decides `null`)
W_YARDSTICKS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
# the conditions the fixture must meet (asserted here and by tests/test_full_model_fixture_w_cpu.py); the worst
# parameter is NOT capped: every parameter with 3 s_bf16 > W_REPORT_3S is printed and recorded in DESIGN.md 3.1
W_LIMIT_EMB, W_LIMIT_MEDIAN, W_MAX_NULL, W_REPORT_3S = 0.06, 0.06, 25, 0.45


def _load(name, fname):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, fname))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


mgf = _load("mgf_w", "make_golden_full.py")     # a private instance: its COND_ROUND_W is this file's to set
mgf.COND_ROUND_W = False


def condition_w_(state_dict):
    """make_golden_full.condition_ with COND_ROUND_W false: the key projection times COND_SCALE, the output projection
    times COND_OUT_SCALE, and the proj_k / proj_v weights NOT moved onto bf16-representable values.  In place."""
    assert mgf.COND_ROUND_W is False
    return mgf.condition_(state_dict)


def load_cond_w(path=None):
    return mgf.load_cond(path or PATH_W)


def cond_w_conditions(d):
    """(embedding, median over non-null parameters, n_null) of s_bf16, and the parameters with 3 s_bf16 > W_REPORT_3S
    as (name, s_bf16) in backward order."""
    live = ~d["null"]
    emb = float(d["s_bf16"][d["names"].index("bev_embedding.weight")])
    loud = [(n, float(s)) for n, s, ok in zip(d["names"], d["s_bf16"], live) if ok and 3.0 * s > W_REPORT_3S]
    return emb, float(np.median(d["s_bf16"][live])), int(d["null"].sum()), loud


def projection_hooks(ref, u, dt):
    """What the split-weight K | V kernel rounds at proj_k / proj_v: the GEMM's feature operand, forward only (the
    backward is the unfused float chain), and the K / V outputs with their cotangents; the weights stay exact."""
    handles = []
    for att in [m for m in ref.modules() if hasattr(m, "proj_k") and hasattr(m, "proj_out")]:
        assert att.n_groups == 1
        for proj in (att.proj_q, att.proj_k, att.proj_v):
            def at_projection(mod, inp, out):
                out = mod._conv_forward(mgf._RoundForward.apply(inp[0], u, dt), mod.weight, mod.bias)
                return mgf._Round.apply(out, u, dt)
            handles.append(proj.register_forward_hook(at_projection))
    assert handles
    return handles


def gen_cond_w(reference_dir):
    """gen_cond's procedure (make_golden_full.py) on the weights of condition_w_ with the yardstick above."""
    mg = _load("mg_w", "make_golden.py")
    mg.install_import_stubs()
    log = logging.getLogger("golden")
    cfg = mgf.cond_config()
    pinned = mgf.pinned_keys(cfg)
    assert min(pinned) >= mgf.min_cell_keys(), (pinned, mgf.min_cell_keys())

    sys.path.insert(0, ROOT)
    from bevrender_amd.model.bevrender import BEVRender as Mine
    torch.manual_seed(mgf.SEED)
    mine = Mine(mgf.cond_config(), log, "train")
    sd = condition_w_({k: v.clone() for k, v in mine.state_dict().items()})
    sys.path.remove(ROOT)
    off_grid = [k for k in sd if k.endswith(".proj_k.weight") or k.endswith(".proj_v.weight")]
    assert off_grid and all(not torch.equal(sd[k].to(torch.bfloat16).float(), sd[k]) for k in off_grid)

    sys.path.insert(0, reference_dir)
    from model.bevrender import BEVRender as Ref
    sys.path.remove(reference_dir)
    torch.manual_seed(0)
    ref = Ref(mgf.cond_config(), log, "train")
    ref.load_state_dict(sd, strict=True)
    img, pose, vtype = mgf.full_inputs()
    params = dict(ref.named_parameters())
    arrival = []
    for n, p in params.items():
        p.register_hook(lambda g, n=n: arrival.append(n))

    def run(u=None, dt=None):
        handles = [] if dt is None else mgf.yardstick_hooks(ref, u, dt, sites=("q", "o")) + projection_hooks(ref, u, dt)
        # every run from the same state (the batch norms' running statistics, which a train-mode forward updates)
        ref.load_state_dict(sd, strict=True)
        ref.zero_grad(set_to_none=True)
        del arrival[:]
        out, _ = ref(img, pose, vtype, {}, False)
        (out * mgf.cond_cotangent(out.shape)).sum().backward()
        for hd in handles:
            hd.remove()
        return out.detach().clone(), {n: p.grad.detach().clone() for n, p in params.items() if p.grad is not None}

    out0, g0 = run()
    names = list(dict.fromkeys(n for n in arrival if n in g0))          # backward order, every parameter once
    assert set(names) == set(g0)
    oi = mgf.sample_index(out0.numel(), 256, 7)
    idx = [mgf.sample_index(g0[n].numel(), mgf.COND_SAMPLES, 100 + i) for i, n in enumerate(names)]
    take = lambda g: [g[n].flatten()[ix].numpy() for n, ix in zip(names, idx)]   # noqa: E731
    base_out, base = out0.flatten()[oi].numpy(), take(g0)
    s_out = {}
    s = {k: np.zeros(len(names)) for k in W_YARDSTICKS}
    bound = np.array([np.linalg.norm(v.astype(np.float64)) for v in base])
    for key, dt in W_YARDSTICKS.items():
        s_out[key] = 0.0
        for u in mgf.COND_U:
            if dt == torch.float32 and u == 1.0:
                continue
            o, g = run(u, dt)
            assert set(g) == set(g0)
            s_out[key] = max(s_out[key], mgf.rel2(o.flatten()[oi].numpy(), base_out))
            for i, v in enumerate(take(g)):
                s[key][i] = max(s[key][i], mgf.rel2(v, base[i]))
                bound[i] = max(bound[i], np.linalg.norm(v.astype(np.float64)))
    null = s["f32"] > mgf.NULL_S_F32
    off = np.cumsum([0] + [len(ix) for ix in idx])
    np.savez_compressed(
        PATH_W, seed=mgf.SEED, in_seed=mgf.IN_SEED, cot_seed=mgf.COT_SEED, cond_scale=mgf.COND_SCALE,
        cond_out_scale=mgf.COND_OUT_SCALE, round_w=False, n_state=len(sd),
        pinned=np.array(pinned), out_shape=np.array(out0.shape), out_idx=oi.numpy(), out_val=base_out,
        g_names=np.array(names), no_grad_names=np.array(sorted(set(params) - set(names))), g_off=off,
        g_idx=torch.cat(idx).numpy().astype(np.int32), g_val=np.concatenate(base),
        norm=np.array([float(g0[n].double().norm()) for n in names]), null=null, null_bound=bound,
        **{"s_out_" + k: v for k, v in s_out.items()}, **{"s_" + k: v for k, v in s.items()})
    d = load_cond_w()
    emb, med, n_null, loud = cond_w_conditions(d)
    print(f"wrote {os.path.basename(PATH_W)}: {os.path.getsize(PATH_W)} bytes, pinned {pinned}, {len(names)} gradients, "
          f"{n_null} null; s(out) " + " ".join(f"{k} {v:.3e}" for k, v in s_out.items()))
    for k in W_YARDSTICKS:
        live = s[k][~null]
        print(f"  s_{k}: embedding {s[k][names.index('bev_embedding.weight')]:.3e} median {np.median(live):.3e} "
              f"worst {live.max():.3e} ({names[int(np.flatnonzero(~null)[live.argmax()])]})")
    print(f"  {len(loud)} parameters with 3 s_bf16 > {W_REPORT_3S} (not capped):")
    for n, v in loud:
        print(f"    {n:90s} s_bf16 {v:.3e} s_f16 {float(d['s_f16'][d['names'].index(n)]):.3e}")
    assert os.path.getsize(PATH_W) <= mgf.COND_MAX_BYTES
    assert emb <= W_LIMIT_EMB and med <= W_LIMIT_MEDIAN and n_null <= W_MAX_NULL, (emb, med, n_null)
    return d


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit(__doc__)
    gen_cond_w(os.path.abspath(sys.argv[1]))
