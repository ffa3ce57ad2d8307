"""fp64 references of the depthwise-convolution tests (test_gpu_dwconv_fp64.py), on torch's CPU grouped convolution.

Channels-last operands as the kernels see them: x [N,H,W,C], dy [N,Ho,Wo,C]; the weight as the PARAMETER stores it,
w [C,K,K] (= weight[:, 0]).  The magnitude tensors of the per-element bound are the same functions on |operands|.  The
bound, its tolerance table and the teeth check are conv_ref's (``"fp32"``: exact products, 2^-19 of the magnitude for the
fp32 accumulation - the depthwise kernels add at most 32 products in fp32 before they continue in fp64)."""
import torch
import torch.nn.functional as F

from tests.conv_ref import _check, _nchw, _nhwc, _teeth, _within  # noqa: F401  (re-exported for the tests)


def dw_geom(H, W, K, s):
    pad = K // 2
    return pad, (H + 2 * pad - K) // s + 1, (W + 2 * pad - K) // s + 1


def dw_fwd_ref(x, w, s, pad=None):
    """x [N,H,W,C], w [C,K,K] (fp64 CPU) -> y [N,Ho,Wo,C]."""
    C, K = w.shape[0], w.shape[-1]
    return _nhwc(F.conv2d(_nchw(x), w.unsqueeze(1), stride=s, padding=K // 2 if pad is None else pad, groups=C))


def dw_dgrad_ref(dy, w, H, W, s):
    """dy [N,Ho,Wo,C] -> dx [N,H,W,C] = the grouped convolution's input gradient."""
    N, C, K = dy.shape[0], w.shape[0], w.shape[-1]
    return _nhwc(torch.nn.grad.conv2d_input((N, C, H, W), w.unsqueeze(1), _nchw(dy), stride=s, padding=K // 2, groups=C))


def dw_wgrad_ref(x, dy, K, s):
    """-> dw [C,K,K] = the grouped convolution's weight gradient."""
    C = x.shape[3]
    return torch.nn.grad.conv2d_weight(_nchw(x), (C, 1, K, K), _nchw(dy), stride=s, padding=K // 2, groups=C)[:, 0]


def shifted(t):
    """[N,H,W,C] moved one pixel to the right, zeros moving in: a reference on it is the convolution with its padding
    shifted by one (pad + 1 on the left, pad - 1 on the right)."""
    out = torch.zeros_like(t)
    out[:, :, 1:] = t[:, :, :-1]
    return out
