"""Plain fp64 CPU references of the layout / merge / pooling / up-sampling / activation kernels (csrc/elementwise.hip) and
of the small GEMM (csrc/small_gemm.hip), written as loops over taps and strided indexing - not as calls of the torch operator
they stand for (tests/test_elementwise_host.py proves them against torch's own fp64 CPU operators).

Every reference returns ``(value, mag)``: ``mag[e]`` is the sum of the absolute values of the terms that went into element
``e``, the quantity the error bounds of tests/test_gpu_elementwise_fp64.py are stated against.  Tensors are channels-last
``[N,H,W,C]`` like the kernels' operands."""
import math

import torch

U = 2.0 ** -24          # fp32 unit roundoff (round to nearest)
POOL_AVG, POOL_MAX, POOL_SUM = 0, 1, 2
ACT_RELU, ACT_SILU, ACT_TANH = 0, 1, 2


def pool_out(H, k, stride):
    return (H - k) // stride + 1


def _taps(H, W, k, stride):
    """(tap index, row slice, column slice): the input pixels tap (i, j) of every window reads, windows in row-major order."""
    Ho, Wo = pool_out(H, k, stride), pool_out(W, k, stride)
    for i in range(k):
        for j in range(k):
            yield i * k + j, slice(i, i + (Ho - 1) * stride + 1, stride), slice(j, j + (Wo - 1) * stride + 1, stride)


def pool_argmax(x, k, stride):
    """(max value, tap index of the arg-max) per window: the tap for which ``v > best or v != v`` LAST became true in a
    row-major scan starting from best = -inf at tap 0 (ATen's max_pool2d rule: the first maximum wins a tie, a NaN beats
    everything before it and is only replaced by a later NaN, an all -inf window points at tap 0)."""
    x = x.double()
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H, k, stride), pool_out(W, k, stride)
    best = torch.full((N, Ho, Wo, C), -math.inf, dtype=torch.float64)
    arg = torch.zeros((N, Ho, Wo, C), dtype=torch.int64)
    for t, rs, cs in _taps(H, W, k, stride):
        v = x[:, rs, cs, :]
        upd = (v > best) | (v != v)
        best = torch.where(upd, v, best)
        arg = torch.where(upd, torch.full_like(arg, t), arg)
    return best, arg


def pool_fwd_ref(kind, x, k, stride):
    x = x.double()
    N, H, W, C = x.shape
    if kind == POOL_MAX:
        best, _ = pool_argmax(x, k, stride)
        return best, best.abs()
    Ho, Wo = pool_out(H, k, stride), pool_out(W, k, stride)
    acc = torch.zeros((N, Ho, Wo, C), dtype=torch.float64)
    mag = torch.zeros_like(acc)
    for _, rs, cs in _taps(H, W, k, stride):
        acc += x[:, rs, cs, :]
        mag += x[:, rs, cs, :].abs()
    if kind == POOL_AVG:
        acc, mag = acc / (k * k), mag / (k * k)
    return acc, mag


def pool_cover(H, W, k, stride):
    """[H,W] number of windows that cover each input pixel (0: a pixel between windows or in the ragged tail)."""
    n = torch.zeros((H, W), dtype=torch.int64)
    for _, rs, cs in _taps(H, W, k, stride):
        n[rs, cs] += 1
    return n


def pool_bwd_ref(kind, x, gy, k, stride):
    """Gradient of pool_fwd_ref with respect to x.  Windows that share tap (i, j) never share a pixel, so the strided
    ``+=`` below adds every window exactly once."""
    gy = gy.double()
    N, H, W, C = x.shape
    gx = torch.zeros((N, H, W, C), dtype=torch.float64)
    mag = torch.zeros_like(gx)
    arg = pool_argmax(x, k, stride)[1] if kind == POOL_MAX else None
    for t, rs, cs in _taps(H, W, k, stride):
        if kind == POOL_MAX:
            g = torch.where(arg == t, gy, torch.zeros_like(gy))
        elif kind == POOL_AVG:
            g = gy / (k * k)
        else:
            g = gy
        gx[:, rs, cs, :] += g
        mag[:, rs, cs, :] += g.abs()
    return gx, mag


def upsample_fwd_ref(x, s):
    x = x.double()
    N, H, W, C = x.shape
    y = torch.empty((N, H * s, W * s, C), dtype=torch.float64)
    for i in range(s):
        for j in range(s):
            y[:, i::s, j::s, :] = x
    return y, y.abs()


def upsample_bwd_ref(gy, s):
    gy = gy.double()
    N, Ho, Wo, C = gy.shape
    gx = torch.zeros((N, Ho // s, Wo // s, C), dtype=torch.float64)
    mag = torch.zeros_like(gx)
    for i in range(s):
        for j in range(s):
            gx += gy[:, i::s, j::s, :]
            mag += gy[:, i::s, j::s, :].abs()
    return gx, mag


def _sigmoid(x):
    # 1 / (1 + e^-x) without overflow: e = exp(-|x|) <= 1
    e = torch.exp(-x.abs())
    return torch.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def act_ref(act, x):
    x = x.double()
    if act == ACT_RELU:
        y = torch.where(x <= 0, torch.zeros_like(x), x)      # NaN stays NaN
    elif act == ACT_SILU:
        y = x * _sigmoid(x)                                  # (-inf * 0 = NaN, as x / (1 + inf))
    else:
        m = torch.expm1(-2.0 * x.abs())                      # tanh|x| = (1 - e) / (1 + e), e = exp(-2|x|) = 1 + m
        y = torch.sign(x) * (-m) / (2.0 + m)
        y = torch.where(x != x, x, y)
    return y, y.abs()


def act_grad_ref(act, x, gy):
    """gy * act'(x); the tanh gradient is gy * (1 - tanh(x)^2)."""
    x, gy = x.double(), gy.double()
    if act == ACT_RELU:
        d = torch.where(x <= 0, torch.zeros_like(x), torch.ones_like(x))   # (NaN: 1, torch's threshold rule)
    elif act == ACT_SILU:
        s = _sigmoid(x)
        d = s * (1.0 + x * (1.0 - s))
    else:
        y = act_ref(ACT_TANH, x)[0]
        d = 1.0 - y * y
    g = gy * d
    return g, g.abs()


def act_inputs(seed=11):
    """The activation inputs of both test files (host and GPU): a grid over [-100, 100], the special values, random values."""
    g = torch.Generator().manual_seed(seed)
    grid = torch.arange(-800, 801, dtype=torch.float64) / 8.0
    special = torch.tensor([0.0, -0.0, 88.0, -88.0, 104.0, -104.0, 1e-40, -1e-40, math.inf, -math.inf, math.nan])
    rnd = torch.randn(2048, generator=g) * torch.tensor([0.5, 3.0, 20.0, 1e-3]).repeat(512)
    return torch.cat([grid.float(), special, rnd]).float()


def small_gemm_ref(a, trans_a, b, trans_b):
    """op(A) op(B) in fp64 as a loop over k; mag = sum_k |a_mk b_kn|."""
    a = a.double().t() if trans_a else a.double()
    b = b.double().t() if trans_b else b.double()
    M, K = a.shape
    N = b.shape[1]
    c = torch.zeros((M, N), dtype=torch.float64)
    mag = torch.zeros_like(c)
    for kk in range(K):
        t = a[:, kk:kk + 1] * b[kk:kk + 1, :]
        c += t
        mag += t.abs()
    return c, mag


def ulps(out, ref, scale=None):
    """|out - ref| in fp32 ulps of max(|scale|, 2^-126) (scale: ref unless given).  Elements where both are NaN or the same
    infinity count 0; a NaN / infinity on one side only counts inf."""
    out, ref = out.double(), ref.double()
    scale = ref.abs() if scale is None else scale.double().abs()
    scale = torch.where(torch.isfinite(scale), scale, torch.ones_like(scale))
    expo = torch.floor(torch.log2(scale.clamp_min(2.0 ** -126)))
    ulp = torch.exp2(expo - 23)
    d = (out - ref).abs() / ulp
    same = ((out != out) & (ref != ref)) | (out == ref)
    d = torch.where(same, torch.zeros_like(d), d)
    return torch.where(d != d, torch.full_like(d, math.inf), d)
