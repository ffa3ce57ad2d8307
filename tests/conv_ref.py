"""fp64 references and the per-element bound of the convolution tests (test_gpu_conv_layouts.py, test_gpu_halo_fp64.py).

Per element |out - ref| <= tol * mag + TINY, where mag is the same fp64 operation on |operands| (the sum of |products| of
each element): no channel or pixel can hide behind a norm."""
import torch
import torch.nn.functional as F

from tests.util import rel_err

TINY = 1e-12

# Per-element bound |out - ref| <= tol * mag + TINY, mag = the fp64 operation on |operands| (sum of |products| of each
# element).  A product formed from p-bit operand pieces is off by at most ~2^(1-p) of |product| (the neglected lo*lo
# term and the pieces' truncation of both operands), so over an element the product error is <= 2^(1-p) * mag.  The
# fp32 accumulation adds roundings of partial sums that are themselves <= mag: allowed 2^-19 (32 ulp) of mag, far above
# what the summation trees reach and far below a dropped input channel or tap (>= 1/K of mag, K <= 1600 here).
#   forward  fp16 x 3 : 22-bit products (11 + 11-bit pieces)      -> 2^-21, doubled for the power-of-two pre-scaling floor
#   forward  bf16 x 6 : the three 8-bit pieces carry all 24 bits  -> 2^-22
#   fp32              : exact products (fp32 MFMA / fmaf)          -> 0
#   backward bf16 x 3 : 16-bit products (8 + 8-bit pieces)         -> 2^-16, x 4 for the truncation of both operands
#   backward bf16 x 1 : each operand rounded once to 8 bits        -> 2 * 2^-9, doubled
PREC_TOL = {"fp16x3": 2.0 ** -20, "bf16x6": 2.0 ** -22, "fp32": 0.0, "bf16x3": 2.0 ** -14, "bf16x1": 2.0 ** -7}
ACC_TOL = 2.0 ** -19
# the norm-wise bounds of test_gpu_ops.py::test_conv2d_fwd_bwd (1e-5 in every parity mode); bf16 x 1 is no parity mode
NORM_TOL = {"fp16x3": 1e-5, "bf16x6": 1e-5, "fp32": 1e-5, "bf16x3": 1e-5, "bf16x1": 1e-2}


def _within(out, ref, mag, tol):
    """Per element: |out - ref| <= tol * mag + TINY (NaN, never written, fails).  Returns (ok, message)."""
    err = (out - ref).abs()
    bad = ~(err <= tol * mag + TINY)
    if not bool(bad.any()):
        return True, ""
    i = tuple(int(v) for v in bad.nonzero()[0])
    return False, (f"{int(bad.sum())} of {bad.numel()} elements off, first {i}: got {float(out[i])!r}, want "
                   f"{float(ref[i])!r} (mag {float(mag[i]):.3g})")


def _check(what, out, ref, mag, prec, extra_mag=None):
    tol = PREC_TOL[prec] + ACC_TOL
    ok, msg = _within(out, ref, mag if extra_mag is None else mag + extra_mag, tol)
    assert ok, f"{what}: {msg}"
    assert rel_err(out, ref) < NORM_TOL[prec], f"{what}: norm-wise {rel_err(out, ref):.3g}"


def _teeth(what, out, wrong_ref, mag, prec):
    """The same comparison against a slightly wrong float64 reference must fail."""
    ok, _ = _within(out, wrong_ref, mag, PREC_TOL[prec] + ACC_TOL)
    assert not ok, f"{what}: the per-element check does not catch a wrong reference"


# ---------------------------------------------------------------------------------------------------- fp64 references
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _fwd_ref(x, w, s, pad):
    """x [N,H,W,Ci], w [Co,KH,KW,Ci] (fp64 CPU) -> y [N,Ho,Wo,Co]."""
    return _nhwc(F.conv2d(_nchw(x), w.permute(0, 3, 1, 2), stride=s, padding=pad))


def _dgrad_ref(dy, w, H, W, s, pad):
    """dy [N,Ho,Wo,Co] -> dx [N,H,W,Ci] = conv2d's input gradient."""
    N, Ci = dy.shape[0], w.shape[3]
    return _nhwc(torch.nn.grad.conv2d_input((N, Ci, H, W), w.permute(0, 3, 1, 2), _nchw(dy), stride=s, padding=pad))


def _wgrad_ref(x, dy, KH, KW, s, pad):
    """-> dw [Co,KH,KW,Ci] = conv2d's weight gradient."""
    Co, Ci = dy.shape[3], x.shape[3]
    return torch.nn.grad.conv2d_weight(_nchw(x), (Co, Ci, KH, KW), _nchw(dy), stride=s, padding=pad).permute(0, 2, 3, 1)
