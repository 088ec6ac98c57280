"""The tile kernel's routes that no other GPU test launches (the last column of tests/test_gemm_tile_forms.py): the
General epilogue behind the implicit-GEMM operand pairs -- a convolution with an fp32 output, bias and ReLU -- and
behind the dense weight-gradient pair with a bias.

Shapes are the smallest that cross each boundary: M = 200 rows (ragged against both tile heights), N = 64 (256 x 64
tiles) and N = 136 (128 x 128, ragged), K = 128 (single buffer, two steps) and K = 576 (double buffer, nine steps).
References and bounds are the sibling tests' (tests/test_gemm_conv_gpu.py): fp32 torch on the bf16 inputs, relative
Frobenius error below 1e-3 for an fp32 output.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _C():
    from k8s_amd.ops._ext import load

    return load()


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-6)).item()


# C, R, stride, pad, H: two images of 10 x 10 outputs (M = 200); K = R * R * C
CONV_A = [(128, 1, 2, 0, 19), (64, 3, 1, 1, 10)]   # C % 64 == 0: ConvA, K = 128 / 576
CONV_AG = [(32, 2, 1, 0, 11), (144, 2, 1, 0, 11)]  # any other C % 8 == 0: ConvAG, K = 128 / 576


@pytest.mark.parametrize("K", [64, 136])
@pytest.mark.parametrize("C,R,st,pad,H", CONV_A + CONV_AG)
def test_conv_fwd_general_epilogue(cuda, C, R, st, pad, H, K):
    torch.manual_seed(11)
    x = torch.randn(2, H, H, C, device=cuda).bfloat16()
    w = (torch.randn(K, R, R, C, device=cuda) * 0.05).bfloat16()
    bias = torch.randn(K, device=cuda)
    y = _C().conv_fwd(x, w, st, pad, 1, True, bias, 1, None)
    ref = torch.relu(F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), bias, st, pad))
    ref = ref.permute(0, 2, 3, 1)
    assert y.dtype == torch.float32 and y.shape == ref.shape == (2, 10, 10, K)
    assert _rel(y, ref) < 1e-3


@pytest.mark.parametrize("K", [128, 576])
def test_gemm_mn_major_pair_general_epilogue(cuda, K):
    """Both operands MN-major (the weight-gradient layout) with a bias: not the F32Rows form."""
    M, N = 200, 136
    torch.manual_seed(12)
    a = torch.randn(K, M, device=cuda).bfloat16()
    b = (torch.randn(K, N, device=cuda) * 0.05).bfloat16()
    bias = torch.randn(N, device=cuda)
    y = _C().gemm(a, False, b, False, None, True, bias, 0, None, False, 1.0, 1)
    assert _rel(y, a.float().t() @ b.float() + bias) < 1e-3
