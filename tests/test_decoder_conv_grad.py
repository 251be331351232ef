"""The render decoder's 3x3 convolution with the backward built from forward kernels (model/decoder_img_render.py,
_ConvGradViaForwardKernels: DESIGN section 6.4).  Its input gradient (flipped, channel-transposed filter) and weight
gradient (unfold + batched GEMM) against autograd of F.conv2d in float64: gradcheck on the CPU, and on the device
against the CPU float64 reference -- never against the device's own convolution backward, the call the Function avoids."""
import pytest
import torch
import torch.nn.functional as F

from bevrender_amd.model.decoder_img_render import _Conv3x3, _ConvGradViaForwardKernels

DEV = "cuda"


@pytest.mark.parametrize("needs", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("shape", [(1, 2, 3, 4, 5), (2, 3, 2, 6, 3), (1, 1, 1, 1, 7)])
def test_conv_grad_function_gradcheck_float64(shape, needs):
    """shape = (B, Cin, Cout, H, W), non-square maps; every needs_input_grad combination."""
    B, Ci, Co, H, W = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, Ci, H, W, generator=gen, dtype=torch.float64).requires_grad_(needs[0])
    w = torch.randn(Co, Ci, 3, 3, generator=gen, dtype=torch.float64).requires_grad_(needs[1])
    assert torch.autograd.gradcheck(_ConvGradViaForwardKernels.apply, (x, w), eps=1e-6, atol=1e-8, rtol=1e-6)
    # the same gradients as the stock convolution's autograd, input by input
    y = _ConvGradViaForwardKernels.apply(x, w)
    cot = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    got = torch.autograd.grad(y, [t for t in (x, w) if t.requires_grad], cot)
    want = torch.autograd.grad(F.conv2d(x, w, None, 1, 1), [t for t in (x, w) if t.requires_grad], cot)
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("channels_last", [False, True])
def test_conv3x3_device_gradients_match_cpu_float64(channels_last):
    """Conv2d(16, 8, 3, 1, 1) -- the decoder layer of DESIGN section 6.4 -- on a non-square map, contiguous and
    channels_last: the output, d(input) and d(weight) against CPU float64 autograd of F.conv2d."""
    torch.manual_seed(0)
    conv = _Conv3x3(16, 8, 3, 1, 1, bias=False).to(DEV)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 16, 45, 62, generator=gen)
    cot = torch.randn(2, 8, 45, 62, generator=gen)
    xg = x.to(DEV)
    if channels_last:
        xg = xg.contiguous(memory_format=torch.channels_last)
        conv = conv.to(memory_format=torch.channels_last)
    xg.requires_grad_(True)
    y = conv(xg)
    assert type(y.grad_fn).__name__ == "_ConvGradViaForwardKernelsBackward", type(y.grad_fn)
    y.backward(cot.to(DEV))
    torch.cuda.synchronize()

    x64 = x.double().requires_grad_(True)
    w64 = conv.weight.detach().double().cpu().requires_grad_(True)
    want = F.conv2d(x64, w64, None, 1, 1)
    want.backward(cot.double())

    def rel(a, b):
        return (a.detach().double().cpu() - b).abs().max().item() / b.abs().max().item()
    # float32 arithmetic over contractions of 16 * 9 terms (output, d input) and 2 * 45 * 62 (d weight); 2e-4 leaves room
    # for a transform-based (Winograd / FFT) forward solver, whose f32 error is ~1e-5 relative
    assert rel(y, want.detach()) < 2e-4, rel(y, want.detach())
    assert rel(xg.grad, x64.grad) < 2e-4, rel(xg.grad, x64.grad)
    assert rel(conv.weight.grad, w64.grad) < 2e-4, rel(conv.weight.grad, w64.grad)
