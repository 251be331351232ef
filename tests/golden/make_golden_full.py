#!/usr/bin/env python3
"""G5: golden output of the reference's full `BEVRender` (model/bevrender.py:14-221) on a synthetic 2-frame window.

Run ONLY in the build container (needs /root/reference and this repo):
    python tests/golden/make_golden_full.py [full] [decoder] [cond]        (no argument: all three)
full -> full_bevrender.npz, decoder -> decoder.npz, cond -> full_bevrender_cond.npz (G5c below: conditioned weights,
every parameter's gradient, and the reference's own rounding sensitivity as the yardstick of the GPU test's limits).

The model has 2.0 M parameters (8 MB): too large to commit.  Instead the weights are *this repo's* `BEVRender`
constructed under `torch.manual_seed(SEED)` on the CPU (deterministic for a given torch build); they are loaded
into the reference model with `strict=True` -- which also pins that both models expose the same 452 state-dict
entries with the same shapes -- and only inputs' seed and sampled outputs are stored.  The test rebuilds the same
weights from the same seed on the GPU box.  Import stubs for timm / torchvision: see make_golden.py.
"""
import importlib.util
import logging
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SEED, IN_SEED = 1234, 99


def full_config():
    R0 = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], dtype=np.float64)
    T = np.eye(4)
    T[:3, :3] = R0
    T[:3, 3] = (0, 0, 1.5)
    K = np.array([[100, 0, 64, 0], [0, 100, 64, 0], [0, 0, 1, 0]], dtype=np.float64)
    return dict(
        BATCH_SIZE=2, DATA_TYPE=torch.float32, DAT_BEV_SHAPE=[28, 28], DAT_EMBED_DIMS=[64, 64], DAT_NUM_STAGES=1,
        DAT_VIT_DEPTHS=[1], DAT_NUM_HEADS=[2], DAT_NUM_GROUPS=[1], DAT_STRIDES=[1], DAT_K_SIZES=[3], DAT_EXPANSION=4,
        DAT_BEV_DEPTH_DIM=5, SAMPLE_Z_SHIFT=-1.0, BEV_BOUND={"X": 20, "Y": 10, "Z": 2}, NUM_VIEWS=1, IMG_HEIGHT=128,
        IMG_WIDTH=128, ORI_IMG_HEIGHT=128, ORI_IMG_WIDTH=128, VEHICLE_TYPE_CODE=0, IMU_TO_RGB={0: [T.copy()]},
        INTRINSIC_K={0: [K.copy()]}, DAT_SCALE_OFFSET_RANGE=True, DAT_DROP_RATE=0.0, DAT_ATTN_DROP_RATE=0.0,
        DAT_DROP_PATH_RATE=0.0, DAT_BACKBONE_TYPE="ResNet18", DECODER_HID_DIM=64, REMOVE_REF_IN_GRAY=False,
        BOUND_CHECK_IMG_PATH=None)


def full_inputs():
    g = torch.Generator().manual_seed(IN_SEED)
    img = torch.randn(2, 2, 1, 3, 128, 128, generator=g) * 0.5
    pose = torch.zeros(2, 2, 3)
    vtype = torch.zeros(2, 1, dtype=torch.long)
    return img, pose, vtype


def sample_index(n, k, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:k]


# ---- G5c: the conditioned whole-model fixture (full_bevrender_cond.npz) ----
COT_SEED = 4321
COND_SCALE = 0.05               # condition_: every attention module's proj_k weight and bias times this
COND_OUT_SCALE = 0.15           # condition_: every attention module's proj_out weight and bias times this
COND_ROUND_W = True             # condition_: proj_k and proj_v weights moved onto bf16-representable values
COND_SAMPLES = 64               # stored entries per parameter gradient
COND_MAX_BYTES = 400 * 1000     # the fixture's size cap
COND_U = (1.0, 1.003, 1.007, 1.011)     # the rounding realisations of the yardstick (float32 skips 1.0: it is the identity)
# the yardsticks: name -> (the type the attention operands are rounded to, also round what STAGE_DTYPE stages)
COND_YARDSTICKS = {"f32": (torch.float32, False), "bf16": (torch.bfloat16, False), "f16": (torch.float16, False),
                   "bf16s": (torch.bfloat16, True)}
NULL_S_F32 = 0.1                # a gradient that float32 rounding alone moves by more than this is noise: "null"
# the conditions the fixture must meet (the generator and tests/test_full_model_fixture_cpu.py assert them)
COND_LIMIT_EMB, COND_LIMIT_MEDIAN, COND_MAX_NULL, COND_LIMIT_WORST3 = 0.06, 0.06, 25, 0.45


def cond_config():
    """full_config() with a BEV bound wide enough that the projector pins more than SCA's MIN_CELL_KEYS keys: the
    pinned keys become a second key segment (tap kernels in the 16-bit modes, cell kernels in the float ones)."""
    cfg = full_config()
    cfg["BEV_BOUND"] = {"X": 50, "Y": 50, "Z": 2}
    return cfg


def cond_cotangent(shape):
    """The loss of the conditioned fixture is (out * cot).sum() with this cot."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(COT_SEED))


def condition_(state_dict):
    """In place, three deterministic edits of the seeded weights that make the REFERENCE's own gradients insensitive
    enough to 16-bit rounding for a 3 s limit to mean something (the conditions below; DESIGN.md, "Whole-model golden"):
      * every attention module's key projection times COND_SCALE: the untrained model's keys have norms above 160 and
        its softmax rows are decided by near ties (bf16 rounding of K and V moves the embedding gradient by 17 %);
      * proj_k / proj_v weights on bf16-representable values: the fused K | V kernel of the 16-bit modes rounds its GEMM's
        weights, an error COMMON to all keys that attention's averaging does not shrink -- with the seeded weights it
        alone moves the bf16 modes' output by 5e-3 and the embedding gradient by 13 %, on the GPU and, with the same
        rounding hooked into the reference, on the CPU;
      * every attention module's output projection times COND_OUT_SCALE: two thirds of SCA's keys are pinned to the same
        few pixels, their rounded V rows are nearly equal and do not average either; a smaller attention branch flips
        fewer of the decoder's ReLUs (the gradients' error goes with the square root of the activations').
    Works on a copy of the state dict (the generator) and on model.state_dict() itself, whose tensors alias the
    parameters (the tests)."""
    n = 0
    with torch.no_grad():
        for k, v in state_dict.items():
            if k.endswith(".proj_k.weight") or k.endswith(".proj_k.bias"):
                v.mul_(COND_SCALE)
                n += 1
            elif k.endswith("_deform_attn.proj_out.weight") or k.endswith("_deform_attn.proj_out.bias"):
                v.mul_(COND_OUT_SCALE)
            if COND_ROUND_W and (k.endswith(".proj_k.weight") or k.endswith(".proj_v.weight")):
                v.copy_(v.to(torch.bfloat16).to(v.dtype))
    assert n > 0 and n % 2 == 0, n
    return state_dict


def pinned_keys(cfg):
    """How many of SCA's keys the oracle's projector pins to (-1, -1), per camera of vehicle code 0."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import bevrender_oracle as orc
    S, D = cfg["DAT_BEV_SHAPE"][0], cfg["DAT_BEV_DEPTH_DIM"]
    pts = orc.sample_3d_points(cfg["BEV_BOUND"], S, D, cfg["SAMPLE_Z_SHIFT"])
    cams = orc.bev_grid_to_camera(pts, cfg["IMU_TO_RGB"][0], cfg["INTRINSIC_K"][0], cfg["IMG_WIDTH"], cfg["IMG_HEIGHT"],
                                  cfg["ORI_IMG_WIDTH"], cfg["ORI_IMG_HEIGHT"])
    return [int((c.reshape(2, -1) == -1.0).all(0).sum()) for c in cams]


def min_cell_keys():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from bevrender_amd.model.SCA import MIN_CELL_KEYS
    return MIN_CELL_KEYS


def rel2(a, b):
    """relative 2-norm deviation of a from b"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d, n = np.linalg.norm(a - b), np.linalg.norm(b)
    return float(d / n) if n > 0 else (0.0 if d == 0 else float("inf"))


def load_cond(path=None):
    """The fixture as a dict; per parameter (in BACKWARD order: the order the reference's autograd finished them in)
    names[i], its sampled gradient idx[i] / val[i], and the arrays norm, s_<yardstick> (COND_YARDSTICKS), null, null_bound."""
    z = np.load(path or os.path.join(HERE, "full_bevrender_cond.npz"))
    d = {k: z[k] for k in z.files}
    off = d["g_off"]
    d["names"] = [str(n) for n in d["g_names"]]
    d["idx"] = [d["g_idx"][off[i]:off[i + 1]].astype(np.int64) for i in range(len(off) - 1)]
    d["val"] = [d["g_val"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    return d


def cond_conditions(d):
    """The four conditions of the yardstick on a loaded fixture: (embedding, median, n_null, worst 3 s_bf16)."""
    live = ~d["null"]
    emb = float(d["s_bf16"][d["names"].index("bev_embedding.weight")])
    return emb, float(np.median(d["s_bf16"][live])), int(d["null"].sum()), float(3.0 * d["s_bf16"][live].max())


class _Round(torch.autograd.Function):
    """x -> (x u) rounded to dt, / u, and the same for the cotangent: the identity up to one rounding to dt, a
    different realisation of that rounding for every u."""
    @staticmethod
    def forward(ctx, x, u, dt):
        ctx.u, ctx.dt = u, dt
        return (x * u).to(dt).float() / u

    @staticmethod
    def backward(ctx, g):
        return (g * ctx.u).to(ctx.dt).float() / ctx.u, None, None


class _RoundForward(_Round):
    """_Round with the cotangent left as it is"""
    @staticmethod
    def backward(ctx, g):
        return g, None, None


class _RoundCotangent(_Round):
    """the identity whose cotangent is rounded as _Round's is"""
    @staticmethod
    def forward(ctx, x, u, dt):
        ctx.u, ctx.dt = u, dt
        return x.view_as(x)


def yardstick_hooks(ref, u, dt, stage=False, sites=("kv", "q", "o", "w")):
    """Module hooks on the reference model that round, once each, what the 16-bit kernels round and a module boundary
    exposes -- in the forward the tensor, in the backward its cotangent (_Round) unless said otherwise.  `sites` selects
    among them ("kv" alone is the first form of this yardstick; it misses the fused kernel's roundings, which the bf16
    modes' errors on the GPU turned out to consist of).  Per attention module (TSA and SCA):
      K, V   the outputs of proj_k and proj_v (proj_q is hooked as well, but the reference's forward never calls it);
      Q      the module's `query` argument, as the attention reads it -- the offset head, which the kernels feed in
             float, gets the unrounded tensor back at its door (one group: the head's input IS the query), and so does a
             missing previous frame (TSA's x=None means x = query);
      dO     the cotangent of proj_out's input, the attention's output: the kernels' dO operand.  The output itself stays
             float, as the kernels leave it (rounding it to bf16 moves the embedding gradient by 0.26: no kernel does that).
      w      the GEMM operands of proj_k and proj_v, forward only, as the fused K | V kernel rounds them (csrc/kvproj.hip;
             its backward is the unfused float one): the sampled features, and the weights -- those always by plain
             round-to-nearest (u = 1): the kernel sees the very same bits, its rounding has one realisation.
    P and dS, which the kernels round as well, are exposed by no module boundary: the limits' factor covers them.
    stage: also what STAGE_DTYPE stages -- the images at the backbone's door and the features it returns.
    Returns the handles."""
    def rnd(t):
        return _Round.apply(t, u, dt)
    handles = []
    for att in [m for m in ref.modules() if hasattr(m, "proj_k") and hasattr(m, "proj_out")]:
        assert att.n_groups == 1
        for proj in (att.proj_q, att.proj_k, att.proj_v):
            def at_projection(mod, inp, out):
                if "w" in sites:
                    out = mod._conv_forward(_RoundForward.apply(inp[0], u, dt), _RoundForward.apply(mod.weight, 1.0, dt),
                                            mod.bias)
                return rnd(out) if "kv" in sites else out
            if "w" in sites or "kv" in sites:
                handles.append(proj.register_forward_hook(at_projection))
        if "o" in sites:
            handles.append(att.proj_out.register_forward_pre_hook(lambda mod, inp: (_RoundCotangent.apply(inp[0], u, dt),)))
        if "q" not in sites:
            continue
        kept = {}

        def at_attention(mod, args, kwargs, kept=kept):
            assert not args
            kept["query"] = kwargs["query"]
            kwargs = dict(kwargs, query=rnd(kwargs["query"]))
            if kwargs.get("x", 0) is None:
                kwargs["x"] = kept["query"].clone()
            return args, kwargs

        def at_offset_head(mod, inp, kept=kept):
            assert inp[0].shape == kept["query"].shape
            return (kept["query"].contiguous(),)
        handles.append(att.register_forward_pre_hook(at_attention, with_kwargs=True))
        head = att.conv_offset if hasattr(att, "conv_offset") else att.conv_offset_m0
        handles.append(head.register_forward_pre_hook(at_offset_head))
    if stage:
        backbone = ref.encoder.img_backbone
        handles.append(backbone.register_forward_pre_hook(lambda mod, inp: (rnd(inp[0]),)))
        handles.append(backbone.register_forward_hook(lambda mod, inp, out: rnd(out)))
    assert handles
    return handles


def gen_cond():
    """G5c: the reference's full model with conditioned weights, a random cotangent, every parameter's gradient, and
    the reference's own sensitivity to rounding its attention operands (the yardstick of the GPU test's limits)."""
    spec = importlib.util.spec_from_file_location("mg", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.install_import_stubs()
    log = logging.getLogger("golden")
    cfg = cond_config()
    pinned = pinned_keys(cfg)
    assert min(pinned) >= min_cell_keys(), (pinned, min_cell_keys())

    sys.path.insert(0, ROOT)
    from bevrender_amd.model.bevrender import BEVRender as Mine
    torch.manual_seed(SEED)
    mine = Mine(cond_config(), log, "train")
    sd = condition_({k: v.clone() for k, v in mine.state_dict().items()})
    sys.path.remove(ROOT)

    sys.path.insert(0, "/root/reference")
    from model.bevrender import BEVRender as Ref
    sys.path.remove("/root/reference")
    torch.manual_seed(0)
    ref = Ref(cond_config(), log, "train")
    ref.load_state_dict(sd, strict=True)
    img, pose, vtype = full_inputs()
    params = dict(ref.named_parameters())
    arrival = []
    for n, p in params.items():
        p.register_hook(lambda g, n=n: arrival.append(n))

    def run(u=None, dt=None, stage=False):
        handles = [] if dt is None else yardstick_hooks(ref, u, dt, stage)
        # every run from the same state: the history frame is computed in eval mode, from the batch norms' running
        # statistics, which a train-mode forward updates
        ref.load_state_dict(sd, strict=True)
        ref.zero_grad(set_to_none=True)
        del arrival[:]
        out, _ = ref(img, pose, vtype, {}, False)
        (out * cond_cotangent(out.shape)).sum().backward()
        for hd in handles:
            hd.remove()
        return out.detach().clone(), {n: p.grad.detach().clone() for n, p in params.items() if p.grad is not None}

    out0, g0 = run()
    names = [n for n in arrival if n in g0]
    names = list(dict.fromkeys(names))          # backward order, every parameter once
    assert set(names) == set(g0)
    oi = sample_index(out0.numel(), 256, 7)
    idx = [sample_index(g0[n].numel(), COND_SAMPLES, 100 + i) for i, n in enumerate(names)]
    take = lambda g: [g[n].flatten()[ix].numpy() for n, ix in zip(names, idx)]   # noqa: E731
    base_out, base = out0.flatten()[oi].numpy(), take(g0)
    s_out = {}
    s = {k: np.zeros(len(names)) for k in COND_YARDSTICKS}
    bound = np.array([np.linalg.norm(v.astype(np.float64)) for v in base])
    for key, (dt, stage) in COND_YARDSTICKS.items():
        s_out[key] = 0.0
        for u in COND_U:
            if dt == torch.float32 and u == 1.0:
                continue
            o, g = run(u, dt, stage)
            assert set(g) == set(g0)
            s_out[key] = max(s_out[key], rel2(o.flatten()[oi].numpy(), base_out))
            for i, v in enumerate(take(g)):
                s[key][i] = max(s[key][i], rel2(v, base[i]))
                bound[i] = max(bound[i], np.linalg.norm(v.astype(np.float64)))
    null = s["f32"] > NULL_S_F32
    off = np.cumsum([0] + [len(ix) for ix in idx])
    path = os.path.join(HERE, "full_bevrender_cond.npz")
    np.savez_compressed(
        path, seed=SEED, in_seed=IN_SEED, cot_seed=COT_SEED, cond_scale=COND_SCALE, cond_out_scale=COND_OUT_SCALE,
        n_state=len(sd),
        pinned=np.array(pinned), out_shape=np.array(out0.shape), out_idx=oi.numpy(), out_val=base_out,
        g_names=np.array(names), no_grad_names=np.array(sorted(set(params) - set(names))), g_off=off,
        g_idx=torch.cat(idx).numpy().astype(np.int32), g_val=np.concatenate(base),
        norm=np.array([float(g0[n].double().norm()) for n in names]), null=null, null_bound=bound,
        **{"s_out_" + k: v for k, v in s_out.items()}, **{"s_" + k: v for k, v in s.items()})
    d = load_cond(path)
    emb, med, n_null, worst3 = cond_conditions(d)
    print(f"wrote full_bevrender_cond.npz: {os.path.getsize(path)} bytes, pinned {pinned}, {len(names)} gradients, "
          f"{n_null} null; s(out) " + " ".join(f"{k} {v:.3e}" for k, v in s_out.items()))
    for k in COND_YARDSTICKS:
        live = s[k][~null]
        print(f"  s_{k}: embedding {s[k][names.index('bev_embedding.weight')]:.3e} median {np.median(live):.3e} "
              f"worst {live.max():.3e} ({names[int(np.flatnonzero(~null)[live.argmax()])]})")
    assert os.path.getsize(path) <= COND_MAX_BYTES
    assert emb <= COND_LIMIT_EMB and med <= COND_LIMIT_MEDIAN and n_null <= COND_MAX_NULL and worst3 <= COND_LIMIT_WORST3, \
        (emb, med, n_null, worst3)
    return d


def main():
    spec = importlib.util.spec_from_file_location("mg", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.install_import_stubs()
    log = logging.getLogger("golden")

    sys.path.insert(0, ROOT)
    from bevrender_amd.model.bevrender import BEVRender as Mine
    torch.manual_seed(SEED)
    mine = Mine(full_config(), log, "train")
    sd = {k: v.clone() for k, v in mine.state_dict().items()}
    sys.path.remove(ROOT)

    sys.path.insert(0, "/root/reference")
    from model.bevrender import BEVRender as Ref
    torch.manual_seed(0)
    ref = Ref(full_config(), log, "train")
    ref.load_state_dict(sd, strict=True)
    img, pose, vtype = full_inputs()
    out, _ = ref(img, pose, vtype, {}, False)
    out.sum().backward()
    g_emb = ref.bev_embedding.weight.grad
    oi = sample_index(out.numel(), 256, 7)
    gi = sample_index(g_emb.numel(), 256, 8)
    np.savez_compressed(
        os.path.join(HERE, "full_bevrender.npz"), seed=SEED, in_seed=IN_SEED, out_shape=np.array(out.shape),
        out_sum=out.detach().double().sum().numpy(), out_abs_sum=out.detach().double().abs().sum().numpy(),
        out_idx=oi.numpy(), out_val=out.detach().flatten()[oi].numpy(),
        gemb_idx=gi.numpy(), gemb_val=g_emb.flatten()[gi].numpy(), gemb_abs_sum=g_emb.double().abs().sum().numpy(),
        n_state=len(sd))
    print("wrote full_bevrender.npz: out", tuple(out.shape), "sum", float(out.sum()), "n_state", len(sd))


def decoder_input(S):
    return torch.randn(2, 64, S, S, generator=torch.Generator().manual_seed(300 + S))


def gen_decoder():
    """G6: BEVImageRenderDecoder (model/decoder_img_render.py:4-93) at the three BEV sides it is defined for, train
    mode (batch statistics).  Same seeded-weights scheme as G5; plain PyTorch on both sides, so this one runs on CPU."""
    log = logging.getLogger("golden")
    rec = {}
    for S in (14, 28, 56):
        for m in [k for k in sys.modules if k == "model" or k.startswith("model.")]:
            del sys.modules[m]
        sys.path.insert(0, ROOT)
        from bevrender_amd.model.decoder_img_render import BEVImageRenderDecoder as Mine
        torch.manual_seed(SEED + S)
        sd = {k: v.clone() for k, v in Mine(bev_spatial_dim=S, model_dim=64, hid_dim=64).state_dict().items()}
        sys.path.remove(ROOT)
        sys.path.insert(0, "/root/reference")
        from model.decoder_img_render import BEVImageRenderDecoder as Ref
        ref = Ref(bev_spatial_dim=S, model_dim=64, hid_dim=64, logger=log)
        ref.load_state_dict(sd, strict=True)
        sys.path.remove("/root/reference")
        ref.train()
        out = ref(decoder_input(S)).detach()
        oi = sample_index(out.numel(), 128, S)
        rec[f"s{S}.shape"] = np.array(out.shape)
        rec[f"s{S}.idx"] = oi.numpy()
        rec[f"s{S}.val"] = out.flatten()[oi].numpy()
        rec[f"s{S}.sum"] = out.double().sum().numpy()
        rec[f"s{S}.n_state"] = len(sd)
    np.savez_compressed(os.path.join(HERE, "decoder.npz"), seed=SEED, **rec)
    print("wrote decoder.npz")


if __name__ == "__main__":
    # no argument: every fixture of this script; else the named ones (full, decoder, cond)
    todo = sys.argv[1:] or ["full", "decoder", "cond"]
    for name in todo:
        {"full": main, "decoder": gen_decoder, "cond": gen_cond}[name]()
