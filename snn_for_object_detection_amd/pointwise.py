"""Stateless pointwise and window operators: activations, pooling, the fused SPP pyramid kernel, nearest up-sampling."""

import functools
from typing import Tuple

import torch
from torch.autograd import Function

from . import _hip
from ._layout import (_F32, _cl_view, _dims5, _new_cl, _out_tensor, _ptr, _raw_dense_cl, _raw_to_cl, _require_device,
                      _stream, _through_fp32, as_sequence, cl_stride)


class _Act(Function):
    @staticmethod
    def forward(ctx, x, act: int):
        _require_device(x, "activation input")
        x = _raw_dense_cl(x)
        y = _cl_view(torch.empty(x.permute(0, 1, 3, 4, 2).shape, device=x.device, dtype=_F32))
        _hip.call("snn_act_fwd", act, x.data_ptr(), y.data_ptr(), x.numel(), _stream())
        ctx.act = act
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y = ctx.saved_tensors
        gy = _raw_dense_cl(gy)
        gx = _cl_view(torch.empty(x.permute(0, 1, 3, 4, 2).shape, device=x.device, dtype=_F32))
        _hip.call("snn_act_bwd", ctx.act, x.data_ptr(), y.data_ptr(), gy.data_ptr(), gx.data_ptr(), x.numel(),
                  _stream())
        return gx, None


def activation(x: torch.Tensor, act: int) -> torch.Tensor:
    def run(t, a):
        seq, single = as_sequence(t)
        y = _Act.apply(seq, a)
        return y[0] if single else y
    return _through_fp32(run, x, act)


class _Pool(Function):
    @staticmethod
    def forward(ctx, x, kind: int, k: int, stride: int):
        _require_device(x, "pool input")
        x = _raw_dense_cl(x)
        T, B, C, H, W = _dims5(x)
        Ho, Wo = (H - k) // stride + 1, (W - k) // stride + 1
        if Ho <= 0 or Wo <= 0:
            raise RuntimeError(f"pool: window {k} larger than input {H}x{W}")
        y = _new_cl((T, B), C, Ho, Wo, x)
        _hip.call("snn_pool_fwd", kind, x.data_ptr(), y.data_ptr(), T * B, H, W, C, Ho, Wo, k, stride, _stream())
        ctx.geom = (kind, k, stride, T, B, C, H, W, Ho, Wo)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        kind, k, stride, T, B, C, H, W, Ho, Wo = ctx.geom
        gy = _raw_dense_cl(gy)
        gx = _new_cl((T, B), C, H, W, x)
        _hip.call("snn_pool_bwd", kind, x.data_ptr(), gy.data_ptr(), gx.data_ptr(), T * B, H, W, C, Ho, Wo, k, stride,
                  _stream())
        return gx, None, None, None


def pool_covers(N: int, H: int, W: int, C: int, k: int, stride: int, pad: int) -> bool:
    """What the padded pooling kernels run: ``snn_pool2d_supported`` (host only; the library is the one place that says it)."""
    return bool(_hip.query("snn_pool2d_supported", N, H, W, C, k, stride, pad))


POOL2D_COVERED = ("snn_pool2d_supported: 2 <= kernel_size <= 7, 1 <= stride <= kernel_size, 0 <= padding <= kernel_size // 2, "
                  "the padded input at least one window in size")


@functools.lru_cache(maxsize=None)
def pool_sets() -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """``(kernel sizes of a padded pool, kernel sizes of SPP)`` - ASKED of the library over the candidates a description
    could name (what ``layer_gen.Pool.get`` / ``SPP.get`` name in their refusals)."""
    return (tuple(k for k in range(1, 16) if pool_covers(1, 16, 16, 1, k, 1, 0)),
            tuple(k for k in range(1, 16) if spp_covers(1, 16, 16, 1, k, 1)))


class _PoolPad(Function):
    """Avg / Max / SumPool2d(k, stride, padding) on csrc/pool.hip: ``x`` and ``gy`` are read at their own pixel strides
    (a channel slice of a concat buffer is not copied).  Returns dx to autograd, as ``_Pool`` does."""

    @staticmethod
    def forward(ctx, x, kind: int, k: int, stride: int, pad: int):
        _require_device(x, "pool input")
        T, B, C, H, W = _dims5(x)
        if not pool_covers(T * B, H, W, C, k, stride, pad):
            raise RuntimeError(f"pool2d: kernel_size {k}, stride {stride}, padding {pad} on {T * B} frames of {H}x{W}x{C} is "
                               f"not covered ({POOL2D_COVERED})")
        x = _raw_to_cl(x)
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        y = _new_cl((T, B), C, Ho, Wo, x)
        _hip.call("snn_pool2d_fwd", kind, x.data_ptr(), cl_stride(x), y.data_ptr(), cl_stride(y), T * B, H, W, C, k, stride,
                  pad, _stream())
        ctx.geom = (kind, k, stride, pad, T, B, C, H, W)
        if kind == _hip.POOL_MAX:
            ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        kind, k, stride, pad, T, B, C, H, W = ctx.geom
        x = ctx.saved_tensors[0] if kind == _hip.POOL_MAX else None
        gy = _raw_to_cl(gy)
        gx = _new_cl((T, B), C, H, W, gy)
        _hip.call("snn_pool2d_bwd", kind, _ptr(x), cl_stride(x) if x is not None else 0, gy.data_ptr(), cl_stride(gy), None, 0,
                  gx.data_ptr(), cl_stride(gx), T * B, H, W, C, k, stride, pad, _stream())
        return gx, None, None, None, None


def pool2d(x: torch.Tensor, kind: int, kernel_size: int, stride: int, padding: int = 0) -> torch.Tensor:
    """``padding == 0``: ``snn_pool_fwd`` / ``snn_pool_bwd`` (dense operands).  ``padding > 0``: the padded kernels of
    csrc/pool.hip (floor mode; max pads with -inf, average counts the padding in its divisor), which refuse what
    ``snn_pool2d_supported`` does not cover before anything is launched."""
    def run(t, *a):
        seq, single = as_sequence(t)
        y = _PoolPad.apply(seq, *a) if a[-1] else _Pool.apply(seq, *a[:-1])
        return y[0] if single else y
    return _through_fp32(run, x, kind, int(kernel_size), int(stride), int(padding))


def spp_covers(N: int, H: int, W: int, C: int, k: int, levels: int) -> bool:
    """What the fused pyramid forward runs: ``snn_spp_supported`` (host only)."""
    return bool(_hip.query("snn_spp_supported", N, H, W, C, k, levels))


class _SPP(Function):
    """``cat([x, P(x), P(P(x)), ...])`` on channels, ``P = MaxPool2d(k, 1, k // 2)``: one forward launch
    (``snn_spp_fwd``), ``levels`` backward launches of ``snn_pool2d_bwd`` on slices of the saved OUTPUT - nothing else is
    saved.  With ``G = [g_0 .. g_L]`` the slices of the incoming gradient: ``h_L = g_L``, ``h_j = g_j + R(y_j; h_{j+1})``
    (``R`` routes the gradient of ``MaxPool(y_j)`` to ``y_j``), ``dx = h_0`` - what autograd gives for the chained spelling.
    Returns dx to autograd: like ``_Pool`` it takes no part in the ``GradAccumulator`` protocol."""

    @staticmethod
    def forward(ctx, x, k: int, levels: int, dest=None):
        _require_device(x, "spp input")
        T, B, C, H, W = _dims5(x)
        if not spp_covers(T * B, H, W, C, k, levels):
            raise RuntimeError(f"spp: kernel_size {k}, levels {levels} on {T * B} frames of {H}x{W}x{C} is not covered "
                               "(snn_spp_supported: kernel_size in {3, 5}, levels in {1, 2, 3})")
        x = _raw_to_cl(x)
        y = _out_tensor(dest, T, B, (levels + 1) * C, H, W, x)
        _hip.call("snn_spp_fwd", x.data_ptr(), cl_stride(x), y.data_ptr(), cl_stride(y), T * B, H, W, C, k, levels, _stream())
        ctx.geom = (k, levels, T, B, C, H, W)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        k, levels, T, B, C, H, W = ctx.geom
        gy = _raw_to_cl(gy)
        ldy, ldg = cl_stride(y), cl_stride(gy)
        st = _stream()
        h, ldh = gy.data_ptr() + 4 * levels * C, ldg          # h_L = g_L, read in place
        keep = []
        for j in range(levels - 1, -1, -1):                    # h_j = g_j + R(y_j; h_{j+1})
            out = _new_cl((T, B), C, H, W, gy)
            keep.append(out)
            _hip.call("snn_pool2d_bwd", _hip.POOL_MAX, y.data_ptr() + 4 * j * C, ldy, h, ldh, gy.data_ptr() + 4 * j * C, ldg,
                      out.data_ptr(), C, T * B, H, W, C, k, 1, k // 2, st)
            h, ldh = out.data_ptr(), C
        return keep[-1], None, None, None


class _Upsample(Function):
    @staticmethod
    def forward(ctx, x, scale: int):
        _require_device(x, "upsample input")
        x = _raw_dense_cl(x)
        T, B, C, H, W = _dims5(x)
        y = _new_cl((T, B), C, H * scale, W * scale, x)
        _hip.call("snn_upsample_fwd", x.data_ptr(), y.data_ptr(), T * B, H, W, C, scale, _stream())
        ctx.geom = (scale, T, B, C, H, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        scale, T, B, C, H, W = ctx.geom
        gy = _raw_dense_cl(gy)
        gx = _new_cl((T, B), C, H, W, gy)
        _hip.call("snn_upsample_bwd", gy.data_ptr(), gx.data_ptr(), T * B, H, W, C, scale, _stream())
        return gx, None


def upsample_nearest(x: torch.Tensor, scale: int) -> torch.Tensor:
    def run(t, sc):
        seq, single = as_sequence(t)
        y = _Upsample.apply(seq, sc)
        return y[0] if single else y
    return _through_fp32(run, x, int(scale))
