"""Plain fp64 CPU references of the padded pooling kernels and the SPP pyramid (csrc/pool.hip), written as loops over
window taps with explicit padding, tie and NaN rules - not as calls of the torch operators they stand for
(tests/test_pool_pad_host.py proves them against torch's own CPU operators and autograd).

Like tests/elementwise_ref.py every reference of a SUM returns ``(value, mag)``: ``mag[e]`` is the sum of the absolute
values of the terms that went into element ``e``.  Tensors are channels-last ``[N,H,W,C]`` like the kernels' operands."""
import math

import torch

U = 2.0 ** -24          # fp32 unit roundoff (round to nearest)
POOL_AVG, POOL_MAX, POOL_SUM = 0, 1, 2


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def _padded(x, pad, fill=0.0):
    """(x with ``pad`` pixels of ``fill`` around every frame, the mask of the pixels that are the image's own)."""
    N, H, W, C = x.shape
    xp = torch.full((N, H + 2 * pad, W + 2 * pad, C), fill, dtype=x.dtype)
    inside = torch.zeros((1, H + 2 * pad, W + 2 * pad, 1), dtype=torch.bool)
    xp[:, pad:pad + H, pad:pad + W, :] = x
    inside[:, pad:pad + H, pad:pad + W, :] = True
    return xp, inside


def _taps(H, W, k, stride, pad):
    """(tap index, row slice, column slice) into the PADDED frame: the pixels tap (i, j) of every window reads."""
    Ho, Wo = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    for i in range(k):
        for j in range(k):
            yield i * k + j, slice(i, i + (Ho - 1) * stride + 1, stride), slice(j, j + (Wo - 1) * stride + 1, stride)


def pool2d_argmax(x, k, stride, pad):
    """(max value, tap index of the arg-max) per window.  Row-major scan over the taps INSIDE the image: the first of
    them starts the scan, a later one replaces it when ``v > best or v != v`` (ATen: the first maximum wins a tie, a NaN
    beats everything before it and is only replaced by a later NaN, an all -inf window points at its first in-image tap)."""
    x = x.double()
    N, H, W, C = x.shape
    Ho, Wo = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    xp, inside = _padded(x, pad)
    best = torch.full((N, Ho, Wo, C), -math.inf, dtype=torch.float64)
    arg = torch.full((N, Ho, Wo, C), -1, dtype=torch.int64)
    for t, rs, cs in _taps(H, W, k, stride, pad):
        v = xp[:, rs, cs, :]
        upd = inside[:, rs, cs, :] & ((arg < 0) | (v > best) | (v != v))
        best = torch.where(upd, v, best)
        arg = torch.where(upd, torch.full_like(arg, t), arg)
    return best, arg


def pool2d_fwd_ref(kind, x, k, stride, pad):
    """MAX: -inf padding.  AVG: sum of the in-image taps / (k * k) (count_include_pad).  SUM: the sum itself."""
    x = x.double()
    N, H, W, C = x.shape
    if kind == POOL_MAX:
        best, _ = pool2d_argmax(x, k, stride, pad)
        return best, best.abs()
    Ho, Wo = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    xp, _ = _padded(x, pad)
    acc = torch.zeros((N, Ho, Wo, C), dtype=torch.float64)
    mag = torch.zeros_like(acc)
    for _, rs, cs in _taps(H, W, k, stride, pad):
        acc += xp[:, rs, cs, :]
        mag += xp[:, rs, cs, :].abs()
    if kind == POOL_AVG:
        acc, mag = acc / (k * k), mag / (k * k)
    return acc, mag


def pool2d_bwd_ref(kind, x, gy, k, stride, pad, addend=None):
    """addend (or 0) + the gradient of pool2d_fwd_ref with respect to x.  Windows that share tap (i, j) never share a
    pixel, so the strided ``+=`` adds every window exactly once; what lands on the padding is cut off."""
    gy = gy.double()
    N, Ho, Wo, C = gy.shape
    H, W = (x.shape[1], x.shape[2]) if x is not None else (addend.shape[1], addend.shape[2])
    gp = torch.zeros((N, H + 2 * pad, W + 2 * pad, C), dtype=torch.float64)
    mp = torch.zeros_like(gp)
    arg = pool2d_argmax(x, k, stride, pad)[1] if kind == POOL_MAX else None
    for t, rs, cs in _taps(H, W, k, stride, pad):
        if kind == POOL_MAX:
            g = torch.where(arg == t, gy, torch.zeros_like(gy))
        elif kind == POOL_AVG:
            g = gy / (k * k)
        else:
            g = gy
        gp[:, rs, cs, :] += g
        mp[:, rs, cs, :] += g.abs()
    gx, mag = gp[:, pad:pad + H, pad:pad + W, :].clone(), mp[:, pad:pad + H, pad:pad + W, :].clone()
    if addend is not None:
        gx += addend.double()
        mag += addend.double().abs()
    return gx, mag


def spp_fwd_ref(x, k, levels):
    """[x | P(x) | P(P(x)) | ...] on channels, P = max pool (k, 1, k // 2) with -inf padding: the chain, level by level."""
    outs = [x.double()]
    for _ in range(levels):
        outs.append(pool2d_argmax(outs[-1], k, 1, k // 2)[0])
    return torch.cat(outs, dim=-1)


def spp_bwd_ref(y, g, k, levels):
    """d loss / d x from the saved pyramid ``y`` and its gradient ``g`` (both ``[N,H,W,(levels+1)*C]``):
    ``h_L = g_L``, ``h_j = g_j + R(y_j; h_{j+1})``, ``dx = h_0``.  -> (dx, mag)."""
    C = y.shape[-1] // (levels + 1)
    sl = lambda t, j: t[..., j * C:(j + 1) * C]
    h, mag = sl(g, levels).double(), sl(g, levels).double().abs()
    for j in range(levels - 1, -1, -1):
        h, m1 = pool2d_bwd_ref(POOL_MAX, sl(y, j), h, k, 1, k // 2, addend=sl(g, j))
        mag = m1
    return h, mag


def same_bits(a, b):
    """fp32 tensors equal bit for bit (NaNs by payload, zeros by sign)."""
    a, b = a.float().contiguous().cpu(), b.float().contiguous().cpu()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def inputs(kind, shape, seed):
    """Test inputs ``[N,H,W,C]`` fp32: "binary" spikes (ties everywhere), "normal", "nan" (normal with NaNs and whole
    NaN-free rows), "inf" (normal with +-inf, and one frame that is -inf throughout: all -inf windows)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "binary":
        return (torch.rand(shape, generator=g) < 0.3).float()
    x = torch.randn(shape, generator=g)
    if kind == "normal":
        return x
    r = torch.rand(shape, generator=g)
    if kind == "nan":
        return torch.where(r < 0.1, torch.full_like(x, math.nan), x)
    x = torch.where(r < 0.1, torch.full_like(x, math.inf), x)
    x = torch.where(r > 0.8, torch.full_like(x, -math.inf), x)
    x[-1] = -math.inf
    return x
