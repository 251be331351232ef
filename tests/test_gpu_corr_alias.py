"""pairwise_corr with aliased arguments against the float64 oracle: one tensor as both sides, a detached alias on either
side, a view off the 16-byte grid, a 16-bit input -- on the one-pass kernels (n <= 64, E % 4 == 0) and the general ones.
And bevr_corr_bwd's aliased-pointer contract through the C ABI (include/bevrender_hip.h): dcam holds both sides' sum,
dmap is not written, on both paths.  The retrieval losses keep the summed path."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from bevrender_amd import _lib, ops
from oracle import bevrender_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(n, E) for n in (8, 64, 80) for E in (1024, 1027)]


def _rel(got, want):
    return (got.double().cpu() - want).abs().max().item() / max(want.abs().max().item(), 1e-12)


def _want(x, normalize, cot, cam_grad=True, map_grad=True):
    """float64 oracle of pairwise_corr(x, x) with the gradient taken through the chosen sides only."""
    x64 = x.detach().double().cpu()
    cam = x64.clone().requires_grad_(cam_grad)
    mp = x64.clone().requires_grad_(map_grad)
    a, b = (F.normalize(cam, dim=1), F.normalize(mp, dim=1)) if normalize else (cam, mp)
    D = O.pairwise_corr(a, b)
    D.backward(cot)
    g = torch.zeros_like(x64)
    for t in (cam, mp):
        if t.grad is not None:
            g = g + t.grad
    return D.detach(), g


def _check(D, grad, want_D, want_g, tag):
    assert _rel(D.detach(), want_D) < 2e-5, f"{tag}: D"
    assert grad is not None, f"{tag}: no gradient"
    assert _rel(grad, want_g) < 1e-4, f"{tag}: grad {_rel(grad, want_g):.3e}"


def _data(n, E, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, E, generator=gen)
    cot = torch.randn(n, n, generator=gen, dtype=torch.float64)
    return x, cot


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("n,E", SHAPES)
def test_corr_one_tensor_as_both_sides(n, E, normalize):
    x, cot = _data(n, E, n + E)
    want_D, want_g = _want(x, normalize, cot)
    xg = x.to(DEV).requires_grad_(True)
    D = ops.pairwise_corr(xg, xg, normalize)
    D.backward(cot.float().to(DEV))
    _check(D, xg.grad, want_D, want_g, "(x, x)")


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("n,E", SHAPES)
def test_corr_detached_alias_takes_one_side_only(n, E, normalize):
    x, cot = _data(n, E, 2 * n + E)
    for cam_side in (True, False):
        want_D, want_g = _want(x, normalize, cot, cam_grad=cam_side, map_grad=not cam_side)
        xg = x.to(DEV).requires_grad_(True)
        args = (xg, xg.detach()) if cam_side else (xg.detach(), xg)
        D = ops.pairwise_corr(*args, normalize)
        D.backward(cot.float().to(DEV))
        _check(D, xg.grad, want_D, want_g, "(x, x.detach())" if cam_side else "(x.detach(), x)")


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("n,E", SHAPES)
def test_corr_view_off_the_16_byte_grid_as_both_sides(n, E, normalize):
    x, cot = _data(n, E, 3 * n + E)
    want_D, want_g = _want(x, normalize, cot)
    buf = torch.cat((torch.zeros(1), x.reshape(-1))).to(DEV).requires_grad_(True)
    y = buf[1:].view(n, E)                     # contiguous, 4 bytes past a 16-byte boundary
    assert y.is_contiguous() and y.data_ptr() % 16 == 4
    D = ops.pairwise_corr(y, y, normalize)
    D.backward(cot.float().to(DEV))
    assert buf.grad[0].item() == 0.0
    _check(D, buf.grad[1:].view(n, E), want_D, want_g, "offset view")


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("n,E", SHAPES)
def test_corr_bf16_input_as_both_sides(n, E, normalize):
    x, cot = _data(n, E, 4 * n + E)
    xb = x.to(torch.bfloat16)
    want_D, want_g = _want(xb.float(), normalize, cot)         # the oracle on the bf16 values themselves
    xg = xb.to(DEV).requires_grad_(True)
    D = ops.pairwise_corr(xg, xg, normalize)
    D.backward(cot.float().to(DEV))
    assert xg.grad.dtype == torch.bfloat16
    assert _rel(D.detach(), want_D) < 2e-5
    # the gradient itself is stored in bf16: its rounding (2^-9 relative) is the limit
    assert _rel(xg.grad.float(), want_g) < 2 ** -8, f"bf16 grad {_rel(xg.grad.float(), want_g):.3e}"


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("n,E", [(8, 1024), (64, 1024), (64, 1027), (80, 1024)])
def test_corr_bwd_c_abi_aliased_pointers(n, E, normalize):
    """bevr_corr_bwd(cam == map): dcam = both sides' sum, dmap (pre-filled with NaN) untouched -- on the one-pass path
    (n <= 64, E % 4 == 0) and the general one (n > 64 or E % 4 != 0)."""
    L = _lib.lib()
    x, cot = _data(n, E, 5 * n + E)
    want_D, want_g = _want(x, normalize, cot)
    xg = x.to(DEV).contiguous()
    D = torch.empty(n, n, device=DEV)
    inc, inm = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.bevr_corr_fwd(p(xg), p(xg), p(D), p(inc), p(inm), n, n, E, int(normalize), st) == 0
    dD = cot.float().to(DEV).contiguous()
    dcam = torch.full((n, E), float("nan"), device=DEV)
    dmap = torch.full((n, E), float("nan"), device=DEV)
    assert L.bevr_corr_bwd(p(xg), p(xg), p(D), p(dD), p(inc), p(inm), p(dcam), p(dmap), n, n, E, int(normalize), st) == 0
    torch.cuda.synchronize()
    assert _rel(D, want_D) < 2e-5
    assert _rel(dcam, want_g) < 1e-4, f"dcam {_rel(dcam, want_g):.3e}"
    assert torch.isnan(dmap).all(), "dmap was written"


@pytest.mark.parametrize("name", ["contrastive", "triplet"])
def test_retrieval_losses_keep_the_summed_path(name, monkeypatch):
    """pairwise_corr(emb, emb) of the losses: ONE bevr_corr_bwd launch with cam == map (the sum written once)."""
    from bevrender_amd.loss.contrastive_loss import ContrastiveLoss
    from bevrender_amd.loss.triplet_loss_metric import TripletLossMetricLearning
    L = _lib.lib()
    orig = L.bevr_corr_bwd
    seen = []

    def spy(*args):
        seen.append((args[0].value, args[1].value))
        return orig(*args)
    monkeypatch.setattr(L, "bevr_corr_bwd", spy)
    gen = torch.Generator().manual_seed(11)
    cmr = torch.randn(4, 8, 6, 6, generator=gen).to(DEV).requires_grad_(True)
    mp = (cmr.detach() + 0.5 * torch.randn(4, 8, 6, 6, generator=gen).to(DEV)).requires_grad_(True)
    loss = (ContrastiveLoss() if name == "contrastive" else TripletLossMetricLearning()).get_loss(cmr, mp)
    loss.backward()
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0][0] == seen[0][1], seen
    assert torch.isfinite(cmr.grad).all() and torch.isfinite(mp.grad).all()
