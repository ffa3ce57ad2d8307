"""Torch restatement, on CPU tensors, of the five predicates ``snn_activity_count`` counts (include/snn_hip.h, SNN_ACT_*).

The predicates are stated on bit patterns and in fp64, so that nothing here depends on how the host treats denormals."""
import torch

NONZERO_F32, NONZERO_BF16, ABOVE_F32, ABOVE_BF16, MASK = 0, 1, 2, 3, 4


def hits(src: torch.Tensor, kind: int, C: int, threshold: float = 0.0) -> torch.Tensor:
    """``src[T, M, ld]`` (fp32 / bf16 elements, or int32 mask words) -> bool ``[T, M, C]``: the elements that count."""
    if kind == MASK:
        assert src.dtype == torch.int32 and C % 32 == 0
        bits = (src[..., : C // 32].unsqueeze(-1) >> torch.arange(32, dtype=torch.int32)) & 1   # bit c & 31 of word c >> 5
        return bits.reshape(*src.shape[:-1], C).bool()
    x = src[..., :C]
    if kind == NONZERO_F32:
        assert x.dtype == torch.float32
        return (x.contiguous().view(torch.int32) & 0x7FFFFFFF) != 0          # -0.0 is zero; NaN and denormals are not
    if kind == NONZERO_BF16:
        assert x.dtype == torch.bfloat16
        return (x.contiguous().view(torch.int16) & 0x7FFF) != 0
    if kind in (ABOVE_F32, ABOVE_BF16):
        assert x.dtype == (torch.float32 if kind == ABOVE_F32 else torch.bfloat16)
        th = torch.tensor(threshold, dtype=torch.float32).double()              # the threshold as the fp32 the call passes
        return x.double() > th                                                  # strict; NaN is not above
    raise ValueError(f"unknown kind {kind}")


def count(src: torch.Tensor, kind: int, C: int, threshold: float = 0.0, per_step: bool = False) -> torch.Tensor:
    """int64 ``[T, C]`` (``per_step``) or ``[C]``."""
    per = hits(src, kind, C, threshold).to(torch.int64).sum(1)
    return per if per_step else per.sum(0)
