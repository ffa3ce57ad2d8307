"""Stateless tensor plumbing under the operators: channels-last layout, destinations inside concat buffers, raw layout
changes and the fp32 <-> bf16 storage conversions.  Nothing here reads a lever or keeps module state."""

from typing import Optional, Sequence, Tuple

import torch
from torch.autograd import Function

from . import _hip

_F32 = torch.float32
_BF16 = torch.bfloat16


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _require_device(t: torch.Tensor, what: str, bf16_ok: bool = False) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensor is on {t.device}; the MI355X path has no CPU fallback "
                           "(move the model and its inputs to a HIP device)")
    if t.dtype == _BF16 and not bf16_ok:
        raise RuntimeError(f"{what}: this operator has no bf16-storage form (convolutions, Norm + LIF / LI / LI+Tanh / "
                           "none, and the Dense / Residual merges do); run the model with activation storage \"fp32\"")
    if t.dtype != _F32 and t.dtype != _BF16:
        raise RuntimeError(f"{what}: expected float32, got {t.dtype}")


def cl_stride(x: torch.Tensor) -> Optional[int]:
    """Pixel stride ``ld`` when the logical ``[..., C, H, W]`` tensor is stored frame-contiguously as
    ``[..., H, W, ld >= C]`` with channel stride 1 (dense channels-last, or a channel slice of a wider
    channels-last buffer); ``None`` otherwise."""
    if x.dim() < 3:
        return None
    *lead, C, H, W = x.shape
    st = x.stride()
    sc, sh, sw = st[-3], st[-2], st[-1]
    if C > 1 and sc != 1:
        return None
    if W > 1:
        ld = sw
    elif H > 1:
        ld = sh
    else:
        ld = C
        for d in range(len(lead) - 1, -1, -1):
            if lead[d] > 1:
                ld = st[d]
                break
    if ld < C or (W > 1 and sw != ld) or (H > 1 and sh != W * ld):
        return None
    expect = H * W * ld
    for d in range(len(lead) - 1, -1, -1):
        if lead[d] > 1 and st[d] != expect:
            return None
        expect *= lead[d]
    return ld


def is_channels_last(x: torch.Tensor) -> bool:
    """True when the logical ``[..., C, H, W]`` tensor is stored DENSELY as ``[..., H, W, C]``."""
    nd = x.dim()
    perm = list(range(nd - 3)) + [nd - 2, nd - 1, nd - 3]
    return x.permute(perm).is_contiguous()


def _cl_view(buf: torch.Tensor) -> torch.Tensor:
    """dense ``[..., H, W, C]`` buffer -> logical ``[..., C, H, W]`` view."""
    nd = buf.dim()
    return buf.permute(list(range(nd - 3)) + [nd - 1, nd - 3, nd - 2])


def _new_cl(lead: Sequence[int], C: int, H: int, W: int, like: torch.Tensor, dtype=None) -> torch.Tensor:
    """Dense channels-last tensor on ``like``'s device, in ``like``'s storage type unless ``dtype`` says otherwise."""
    return _cl_view(torch.empty((*lead, H, W, C), device=like.device, dtype=dtype or like.dtype))


def _alias(root: torch.Tensor, storage_offset: int, T: int, B: int, C: int, H: int, W: int, ld: int) -> torch.Tensor:
    """A fresh tensor (no autograd view relation) over ``root``'s storage: logical ``[T,B,C,H,W]``,
    channels-last with pixel stride ``ld``.  Only the HIP kernels write through such aliases."""
    t = torch.empty(0, device=root.device, dtype=root.dtype)
    t.set_(root.untyped_storage(), storage_offset, (T, B, C, H, W), (B * H * W * ld, H * W * ld, 1, W * ld, ld))
    return t


class ConcatPromise:
    """A lazily allocated channels-last buffer ``[T,B,H,W,total_c]`` that several producers fill slice by
    slice (the Dense merge of generator.py:157-161 without the copy).  A promise nested in a parent
    destination is itself a channel slice of the parent's buffer."""

    def __init__(self, total_c: int, parent: "Optional[Dest]" = None):
        self.total_c, self.parent = total_c, parent
        self.buf: Optional[torch.Tensor] = None

    def get(self, T: int, B: int, H: int, W: int, like: torch.Tensor, dtype=None) -> torch.Tensor:
        if self.buf is None:
            if self.parent is not None:
                self.buf = self.parent.tensor(T, B, self.total_c, H, W, like, dtype)
            else:
                self.buf = _new_cl((T, B), self.total_c, H, W, like, dtype)
        if self.buf.dtype != (dtype or like.dtype):
            raise RuntimeError("Dense merge: branches store their outputs in different types (fp32 / bf16 storage mixed)")
        if tuple(self.buf.shape) != (T, B, self.total_c, H, W):
            raise RuntimeError(f"Dense merge: branch outputs differ in shape: {tuple(self.buf.shape)} vs "
                               f"{(T, B, self.total_c, H, W)}")
        return self.buf


class Dest:
    """Where an operator must put its ``[T,B,c,H,W]`` result: channels ``off .. off+c`` of a promise."""

    def __init__(self, promise: ConcatPromise, off: int, c: int):
        self.promise, self.off, self.c = promise, off, c

    def tensor(self, T: int, B: int, C: int, H: int, W: int, like: torch.Tensor, dtype=None) -> torch.Tensor:
        if C != self.c:
            raise RuntimeError(f"destination slice holds {self.c} channels, operator produces {C}")
        buf = self.promise.get(T, B, H, W, like, dtype)
        return _alias(buf, buf.storage_offset() + self.off, T, B, C, H, W, cl_stride(buf))

    def holds(self, x: torch.Tensor) -> bool:
        """True when ``x`` already IS this destination (same storage, offset and pixel stride)."""
        buf = self.promise.buf
        if buf is None or x.dim() != 5 or x.shape[2] != self.c:
            return False
        return (x.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
                and x.storage_offset() == buf.storage_offset() + self.off and cl_stride(x) == cl_stride(buf)
                and tuple(x.shape[:2]) == tuple(buf.shape[:2]) and tuple(x.shape[3:]) == tuple(buf.shape[3:]))


def _out_tensor(dest: Optional[Dest], T: int, B: int, C: int, H: int, W: int, like: torch.Tensor, dtype=None) -> torch.Tensor:
    return dest.tensor(T, B, C, H, W, like, dtype) if dest is not None else _new_cl((T, B), C, H, W, like, dtype)


def _raw_to_cl(x: torch.Tensor) -> torch.Tensor:
    """Non-differentiable layout change to (possibly channel-sliced) channels-last memory."""
    if cl_stride(x) is not None:
        return x
    _require_device(x, "layout", bf16_ok=True)
    if x.dtype == _BF16:   # (rare: bf16 tensors are born channels-last) torch's strided copy
        out = _new_cl(x.shape[:-3], *x.shape[-3:], x)
        out.copy_(x)
        return out
    xc = x.contiguous()
    lead, (C, H, W) = xc.shape[:-3], xc.shape[-3:]
    n = 1
    for d in lead:
        n *= d
    out = _new_cl(lead, C, H, W, xc)
    _hip.call("snn_nchw_to_nhwc", xc.data_ptr(), out.data_ptr(), n, C, H, W, _stream())
    return out


def _raw_dense_cl(x: torch.Tensor) -> torch.Tensor:
    """Dense channels-last copy of a channel-sliced tensor (operators without a pixel-stride argument)."""
    x = _raw_to_cl(x)
    if is_channels_last(x):
        return x
    lead, (C, H, W) = x.shape[:-3], x.shape[-3:]
    n = 1
    for d in lead:
        n *= d
    out = _new_cl(lead, C, H, W, x)
    _hip.call("snn_copy_channels_bf16" if x.dtype == _BF16 else "snn_copy_channels", x.data_ptr(), cl_stride(x),
              out.data_ptr(), C, n * H * W, C, _stream())
    return out


def _raw_to_nchw(x: torch.Tensor) -> torch.Tensor:
    if x.is_contiguous():
        return x
    if x.dtype == _BF16:
        return x.contiguous()
    x = _raw_dense_cl(x)
    lead, (C, H, W) = x.shape[:-3], x.shape[-3:]
    n = 1
    for d in lead:
        n *= d
    out = torch.empty(x.shape, device=x.device, dtype=_F32)
    _hip.call("snn_nhwc_to_nchw", x.data_ptr(), out.data_ptr(), n, C, H, W, _stream())
    return out


class _ToChannelsLast(Function):
    @staticmethod
    def forward(ctx, x):
        return _raw_to_cl(x)

    @staticmethod
    def backward(ctx, g):
        return _raw_to_nchw(g)


def to_channels_last(x: torch.Tensor) -> torch.Tensor:
    """Differentiable entry adapter for callers holding NCHW-contiguous frames (soda.py:138-144)."""
    if cl_stride(x) is not None:
        return x
    return _ToChannelsLast.apply(x)


def as_sequence(x: torch.Tensor) -> Tuple[torch.Tensor, bool]:
    """``[B,C,H,W]`` or ``[T,B,C,H,W]`` -> channels-last ``[T,B,C,H,W]`` and "was a single step"."""
    if x.dim() == 4:
        return to_channels_last(x).unsqueeze(0), True
    if x.dim() == 5:
        return to_channels_last(x), False
    raise RuntimeError(f"expected [B,C,H,W] or [T,B,C,H,W], got shape {tuple(x.shape)}")


def _dims5(x: torch.Tensor):
    T, B, C, H, W = x.shape
    return T, B, C, H, W


def _copy_cl(src: torch.Tensor, dst: torch.Tensor) -> None:
    """dst = src, both (possibly channel-sliced) channels-last ``[T,B,C,H,W]``."""
    if src.dtype != dst.dtype:
        raise RuntimeError("merge: operands are stored in different types (fp32 / bf16 storage mixed)")
    T, B, C, H, W = _dims5(src)
    _hip.call("snn_copy_channels_bf16" if src.dtype == _BF16 else "snn_copy_channels", src.data_ptr(), cl_stride(src),
              dst.data_ptr(), cl_stride(dst), T * B * H * W, C, _stream())


def _add_cl(a: torch.Tensor, b: torch.Tensor, dst: torch.Tensor) -> None:
    """dst = a + b over channels-last ``[T,B,C,H,W]`` operands with their own pixel strides (dst may be a)."""
    if not (a.dtype == b.dtype == dst.dtype):
        raise RuntimeError("merge: operands are stored in different types (fp32 / bf16 storage mixed)")
    T, B, C, H, W = _dims5(a)   # (bf16 storage: the sum is formed in fp32 and rounded once)
    _hip.call("snn_add_bf16" if a.dtype == _BF16 else "snn_add", a.data_ptr(), cl_stride(a), b.data_ptr(), cl_stride(b),
              dst.data_ptr(), cl_stride(dst), T * B * H * W, C, _stream())


def _raw_convert(x: torch.Tensor, dtype) -> torch.Tensor:
    """fp32 <-> bf16 copy of a tensor in the same memory order (snn_convert_bf16; round to nearest even).  Dense
    channels-last or contiguous tensors are converted in place order; anything else is made dense channels-last first."""
    if x.dtype == dtype:
        return x
    _require_device(x, "storage conversion", bf16_ok=True)
    if x.dim() >= 3 and not x.is_contiguous():
        x = _raw_dense_cl(x)
        out = _new_cl(x.shape[:-3], *x.shape[-3:], x, dtype)
    else:
        x = x.contiguous()
        out = torch.empty(x.shape, device=x.device, dtype=dtype)
    if x.numel():
        _hip.call("snn_convert_bf16", x.data_ptr(), out.data_ptr(), x.numel(), 1 if dtype == _BF16 else 0, _stream())
    return out


class _Convert(Function):
    """Leaves / enters the bf16-storage domain: the gradient crosses the boundary the other way."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src_dtype = x.dtype
        return _raw_convert(x, dtype)

    @staticmethod
    def backward(ctx, g):
        return _raw_convert(g, ctx.src_dtype), None


def to_float32(x: torch.Tensor) -> torch.Tensor:
    return x if x.dtype == _F32 else _Convert.apply(x, _F32)


def to_bfloat16(x: torch.Tensor) -> torch.Tensor:
    return x if x.dtype == _BF16 else _Convert.apply(x, _BF16)


def _through_fp32(op, x: torch.Tensor, *args):
    """Operators without a bf16-storage kernel (activations, pooling, up-sampling, ConvLSTM, SLI / Synapse: none of them is
    on the TinyYolo path) still work in that mode: the tensor is widened to fp32 for the operator and its result is
    narrowed again (two conversion passes - correct, not fast)."""
    if x.dtype != _BF16:
        return op(x, *args)
    return to_bfloat16(op(to_float32(x), *args))
