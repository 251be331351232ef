"""Pin the CPU oracle against golden vectors produced by the reference's own modules
(tests/golden/make_golden.py).  CPU only."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import bevrender_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    z = np.load(os.path.join(GOLDEN, name))
    return {k: z[k] for k in z.files}


def params_of(z, dtype=torch.float32):
    return {k[len("param."):]: torch.tensor(v, dtype=dtype).requires_grad_(True)
            for k, v in z.items() if k.startswith("param.")}


def check_grads(z, p, inputs, rtol, atol):
    for k, v in z.items():
        if k.startswith("grad_param."):
            g = p[k[len("grad_param."):]].grad
            assert g is not None, k
            np.testing.assert_allclose(g.numpy(), v, rtol=rtol, atol=atol, err_msg=k)
        if k.startswith("grad_in."):
            g = inputs[k[len("grad_in."):]].grad
            np.testing.assert_allclose(g.numpy(), v, rtol=rtol, atol=atol, err_msg=k)


def _mkl_on_intel_avx512():
    """The CPU kernel path the goldens were recorded on and the bit-exact checks hold on: MKL on an Intel CPU with
    AVX-512.  MKL picks its GEMM and matrix-inverse kernels by CPU vendor, instruction set and operand shape (on AMD
    CPUs MKL_CBWR does not pin them), so elsewhere the same float op sequence rounds a few elements differently."""
    try:
        with open("/proc/cpuinfo") as fh:
            intel = "GenuineIntel" in fh.read()
    except OSError:
        intel = False
    return intel and torch.backends.mkl.is_available() and torch.backends.cpu.get_cpu_capability() == "AVX512"


EXACT_BLAS = _mkl_on_intel_avx512()

TSA = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "tsa_*.npz")))
SCA = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "sca_*.npz")))
PROJ = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "proj_*.npz")))


@pytest.mark.parametrize("name", TSA)
def test_tsa_matches_reference(name):
    z = load(name)
    B, C, h, g, S, k, s, sor, xnone = [int(v) for v in z["cfg"]]
    p = params_of(z)
    query = torch.tensor(z["query"]).requires_grad_(True)
    prev = None if xnone else torch.tensor(z["prev_bev"]).requires_grad_(True)
    out = O.tsa_forward(p, query, prev, n_heads=h, n_groups=g, kernel_size=k, stride=s,
                        scale_offset_range=bool(sor))
    np.testing.assert_allclose(out.detach().numpy(), z["out"], rtol=2e-5, atol=2e-6)
    out.backward(torch.tensor(z["cot"]))
    check_grads(z, p, {"query": query, "prev_bev": prev}, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("name", SCA)
def test_sca_matches_reference(name):
    z = load(name)
    B, C, h, g, S, D, Hi, Wi, sor = [int(v) for v in z["cfg"]]
    p = params_of(z)
    query = torch.tensor(z["query"]).requires_grad_(True)
    x = torch.tensor(z["x"]).requires_grad_(True)
    ref = torch.tensor(z["reference_points"])
    out = O.sca_forward(p, x, query, ref, n_heads=h, n_groups=g, depth_dim=D, scale_offset_range=bool(sor))
    np.testing.assert_allclose(out.detach().numpy(), z["out"], rtol=2e-5, atol=2e-6)
    out.backward(torch.tensor(z["cot"]))
    check_grads(z, p, {"query": query, "x": x}, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("name", PROJ)
def test_projector_matches_reference_bit_exact(name):
    z = load(name)
    S, D, X, Y, Z, zs, iw, ih, ow, oh = z["cfg"]
    S, D, iw, ih, ow, oh = int(S), int(D), int(iw), int(ih), int(ow), int(oh)
    pts = O.sample_3d_points({"X": X, "Y": Y, "Z": Z}, S, D, float(zs))
    assert pts.shape == (4, S // 2, S, D)
    np.testing.assert_array_equal(pts.numpy(), z["points_3d"])
    p2 = O.bev_grid_to_camera(pts, list(z["imu_to_rgb"]), list(z["K"]), iw, ih, ow, oh)
    got = torch.stack(p2, 0).numpy()
    if EXACT_BLAS:
        np.testing.assert_array_equal(got, z["points_2d"])
    else:   # a few float32 ulps of the pixel coordinates, scaled to [-1, 1]; a point flipping the mask moves by ~1
        np.testing.assert_allclose(got, z["points_2d"], rtol=0, atol=1e-6)
    # the fixture exercises the mask: some points are pinned to (-1, -1)
    masked = np.all(z["points_2d"] == -1.0, axis=1).mean()
    assert 0.0 < masked < 1.0


def test_encoder_layer_matches_reference():
    z = load("enclayer.npz")
    B, C, S, D, h, X, Y, Z = [int(v) for v in z["cfg"]]
    p = params_of(z)
    bev_query = torch.tensor(z["bev_query"]).requires_grad_(True)
    prev_bev = torch.tensor(z["prev_bev"]).requires_grad_(True)
    img_feat = torch.tensor(z["img_feat"]).requires_grad_(True)
    pts = O.sample_3d_points({"X": X, "Y": Y, "Z": Z}, S, D, -1.0)
    p2 = O.bev_grid_to_camera(pts, list(z["imu_to_rgb"]), list(z["K"]), 128, 128, 128, 128)
    ref = O.sca_reference_points(p2, B)
    out = O.encoder_layer_forward(p, bev_query, img_feat, prev_bev, ref, n_heads=h, n_groups=1, depth_dim=D,
                                  n_views=1, kernel_size=3, stride=1)
    np.testing.assert_allclose(out.detach().numpy(), z["out"], rtol=5e-5, atol=5e-6)
    out.backward(torch.tensor(z["cot"]))
    check_grads(z, p, {"bev_query": bev_query, "prev_bev": prev_bev, "img_feat": img_feat}, rtol=5e-4, atol=5e-5)


def test_recall_matches_reference():
    z = load("recall.npz")
    for tag in ("a", "b"):
        got = O.get_recall(z[f"cam_{tag}"], z[f"map_{tag}"])
        np.testing.assert_allclose(np.array(got), z[f"recall_{tag}"], rtol=0, atol=1e-12)
    assert 0 < z["recall_b"][0] < 100  # a non-trivial case


def test_retrieval_losses_basic_properties():
    """PARITY UNPINNED (pytorch_metric_learning absent): only sanity properties are asserted."""
    torch.manual_seed(0)
    cam = torch.randn(4, 32, dtype=torch.float64, requires_grad=True)
    mp = torch.randn(4, 32, dtype=torch.float64, requires_grad=True)
    for fn in (O.contrastive_loss, O.lifted_structure_loss):
        l = fn(cam, mp)
        assert l.ndim == 0 and l.item() >= 0
        l.backward()
        # scale invariance (embeddings are L2-normalised inside)
        assert abs(fn(cam * 3.0, mp * 0.5).item() - l.item()) < 1e-9
    # identical pairs -> zero positive distance
    l0 = O.contrastive_loss(cam.detach(), cam.detach())
    assert l0.item() >= 0


def _make_golden_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mg", os.path.join(GOLDEN, "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def enclayer_s56_setup(device="cpu", precision=None):
    """This repo's EncoderLayer with the name-seeded weights of G4b + the seeded inputs (shared with the GPU test)."""
    from bevrender_amd.model.bev_cmr_proj import BEV2CameraProjector
    from bevrender_amd.model.encoder import EncoderLayer
    mg = _make_golden_module()
    c = mg.ENC56
    T, K = mg.make_rig("front1")
    proj = BEV2CameraProjector(imu_to_rgb={0: T}, K={0: [k.copy() for k in K]}, vehicle_type_code=0, img_width=128,
                               img_height=128, ori_img_width=128, ori_img_height=128, device=device)
    layer = EncoderLayer(bev_bound=c["bound"], bev2cmr_projector=proj, n_views=1, bev_feat_shape=c["S"],
                         bev_depth_dim=c["D"], z_shift=-1.0, dim_embed=c["C"], expansion=4, stage_idx=0, n_groups=1,
                         n_heads=c["h"], stride=1, kernel_size=3, batch_size=c["B"], scale_offset_range=True,
                         drop_path_rate=0.0, precision=precision)
    mg.randomize_by_name_(layer, c["wseed"])
    return mg, c, T, K, layer


# gradients that are analytically zero: proj_k.bias shifts every logit of a query by the same amount and softmax is
# shift invariant, so the reference's own value is rounding noise
ANALYTIC_ZERO = ("proj_k.bias",)


def check_sampled(z, name, g, rtol, atol_frac, floor_frac):
    """Sampled entries of one gradient: |got - want| <= rtol |want| + atol_frac max|THIS gradient|.  No global floor: a
    floor relative to the largest gradient of the fixture (648, an MLP weight) exceeded the whole magnitude of the small
    tensors (d rpe_table 0.73, d prev_bev 0.65) in bf16 mode, so an all-zero gradient would have passed.
    Only the analytically-zero gradients (ANALYTIC_ZERO) are held to a noise floor instead, floor_frac of the
    fixture's largest gradient.  Returns err / absmax, or None for a noise tensor (not part of any 'worst' figure)."""
    idx, val, amax = z[name + ".idx"], z[name + ".val"], float(z[name + ".absmax"])
    got = g.detach().flatten().cpu().numpy()[idx]
    if name.endswith(ANALYTIC_ZERO):
        floor = floor_frac * max(float(z[str(n) + ".absmax"]) for n in z["names"])
        assert np.all(np.abs(got) <= floor + np.abs(val)), f"{name}: analytically zero, got {np.abs(got).max():.3e}"
        return None
    err = np.abs(got - val).max() / (amax + 1e-30)
    assert np.all(np.abs(got - val) <= rtol * np.abs(val) + atol_frac * amax), f"{name}: err/absmax {err:.3e}"
    return err


def test_encoder_layer_s56_matches_reference():
    """G4b: the oracle's EncoderLayer at S=56, C=64, D=5 (M=3136, N_sca=7840) against sampled outputs and gradients of
    the reference's own EncoderLayer -- the largest side the reference's materialised tensors fit in the container."""
    z = load("enclayer_s56.npz")
    mg, c, T, K, layer = enclayer_s56_setup()
    assert len(layer.state_dict()) == int(z["n_state"])
    p = {k: v.detach().clone().requires_grad_(True) for k, v in layer.state_dict().items()}
    bev_query, prev_bev, img_feat, cot = mg.enclayer_s56_inputs()
    ins = {"bev_query": bev_query, "prev_bev": prev_bev, "img_feat": img_feat}
    for v in ins.values():
        v.requires_grad_(True)
    pts = O.sample_3d_points(c["bound"], c["S"], c["D"], -1.0)
    ref = O.sca_reference_points(O.bev_grid_to_camera(pts, T, K, 128, 128, 128, 128), c["B"])
    out = O.encoder_layer_forward(p, bev_query, img_feat, prev_bev, ref, n_heads=c["h"], n_groups=1,
                                  depth_dim=c["D"], n_views=1, kernel_size=3, stride=1)
    got = out.detach().flatten().numpy()[z["out_idx"]]
    np.testing.assert_allclose(got, z["out_val"], rtol=1e-4, atol=1e-5)
    assert abs(out.detach().double().sum().item() - float(z["out_sum"])) <= 1e-5 * float(z["out_abs_sum"])
    out.backward(cot)
    for name in z["names"]:
        name = str(name)
        g = ins[name[len("grad_in."):]].grad if name.startswith("grad_in.") else p[name[len("grad_param."):]].grad
        assert g is not None, name
        check_sampled(z, name, g, rtol=1e-3, atol_frac=1e-4, floor_frac=2e-6)


def test_streaming_and_row_subset_forms_equal_the_materialised_core():
    """oracle.attention_core_streaming (tiled keys, online softmax, explicit 4-tap lookup at ty = i + a, tx = j rx + b:
    the algorithmic twin of csrc/attn_fwd.hip) and attention_core(rows=...) against the materialised formulation that
    the goldens pin -- float64, keys on / outside the border, g = 1 and g = 2."""
    torch.manual_seed(0)
    for (B, h, g, c, S, D, N) in [(2, 2, 1, 8, 6, 3, 50), (1, 4, 2, 4, 8, 2, 70)]:
        M = S * S
        q = torch.randn(B * h, c, M, dtype=torch.float64)
        k = torch.randn(B * h, c, N, dtype=torch.float64)
        v = torch.randn(B * h, c, N, dtype=torch.float64)
        pos = (torch.rand(B * g, N, 2, dtype=torch.float64) * 2 - 1) * 1.3
        pos[0, 0] = torch.tensor([-1.0, -1.0])
        pos[0, 1] = torch.tensor([1.0, 1.0])
        pos[0, 2] = torch.tensor([-3.0, 3.0])
        tab = torch.randn(h, 2 * S - 1, 2 * S * D - 1, dtype=torch.float64)
        full = O.attention_core(q, k, v, pos, tab, S, S, g, c ** -0.5)
        stream = O.attention_core_streaming(q, k, v, pos, tab, S, S, g, c ** -0.5, tile=16)
        np.testing.assert_allclose(stream.numpy(), full.numpy(), rtol=0, atol=1e-12)
        rows = torch.tensor([0, 5, M - 1, 7])
        sub = O.attention_core(q, k, v, pos, tab, S, S, g, c ** -0.5, rows=rows)
        if EXACT_BLAS:
            np.testing.assert_array_equal(sub.numpy(), full[:, :, rows].numpy())
        else:   # the 4-row products may run on another BLAS kernel than the 36-row ones: rounding of <= 70-term sums
            np.testing.assert_allclose(sub.numpy(), full[:, :, rows].numpy(), rtol=0, atol=1e-14)


def test_ego_motion_warp_restatement_properties():
    """oracle.tv_affine / project_history_bev_feat (PARITY UNPINNED: torchvision absent): zero pose is the identity,
    an integer translation is a shift with zero fill, a half-pixel shift attenuates the border twice (value x mask),
    and the two chained resamplings of model/encoder.py:436-453 compose as written."""
    torch.manual_seed(1)
    img = torch.randn(3, 6, 7)
    np.testing.assert_allclose(O.tv_affine(img, 0.0, (0, 0)).numpy(), img.numpy(), atol=2e-6)
    shifted = torch.zeros_like(img)
    shifted[:, :5, 2:] = img[:, 1:, :5]
    np.testing.assert_allclose(O.tv_affine(img, 0.0, (2, -1)).numpy(), shifted.numpy(), atol=2e-6)
    half = O.tv_affine(torch.ones(1, 4, 4), 0.0, (0.5, 0.0))
    np.testing.assert_allclose(half[0, :, 0].numpy(), 0.25, atol=1e-6)
    np.testing.assert_allclose(half[0, :, 1:].numpy(), 1.0, atol=1e-6)
    bev = torch.randn(2, 3, 8, 8)
    pose = torch.tensor([[[1.0, 2.0, 0.3], [0.5, -1.0, -0.2]], [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]])
    out = O.project_history_bev_feat(bev, pose)
    want0 = O.tv_affine(O.tv_affine(bev[0], np.degrees(0.3), (0.5, 3.0)), np.degrees(0.2), (0.0, 0.0))
    np.testing.assert_allclose(out[0].numpy(), want0.numpy(), atol=1e-6)
    np.testing.assert_allclose(out[1].numpy(), bev[1].numpy(), atol=4e-6)


def test_triplet_loss_restatement_properties():
    """oracle.triplet_margin_loss (PARITY UNPINNED): without semi-hard triplets only the embedding regulariser remains;
    with them the loss exceeds it; gradients flow."""
    torch.manual_seed(2)
    cam = torch.randn(6, 32, dtype=torch.float64, requires_grad=True)
    far = O.triplet_margin_loss(cam, cam.detach() + 1e-3 * torch.randn(6, 32, dtype=torch.float64))
    reg = torch.cat((cam, cam)).norm(dim=1).mean()
    assert abs(far.item() - reg.item()) < 1e-2                    # positives far closer than any negative: nothing mined
    mp = (cam.detach() + 3.0 * torch.randn(6, 32, dtype=torch.float64)).requires_grad_(True)
    loss = O.triplet_margin_loss(cam, mp)
    loss.backward()
    assert loss.item() >= torch.cat((cam, mp)).norm(dim=1).mean().item() - 1e-12
    assert cam.grad.abs().sum() > 0
