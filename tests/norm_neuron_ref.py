"""Float64 restatement of the fused ``[BatchNorm] -> [neuron] [+ addend]`` layer (TEST INFRASTRUCTURE ONLY).

Plain torch float64; nothing here calls into the package.  It restates

* BatchNorm2d as ``layer_gen.py`` applies it to a sequence: one module called once per timestep, so mean and biased
  variance are taken over (B, H, W) of each t, and the running statistics are updated T times in order with the unbiased
  variance and ``momentum``; eval mode normalises with the running statistics;
* the neuron steps of ``oracle/neurons.py`` (LIF, LI, LI + Tanh) and ``oracle/net.py`` (SLI, Synapse), evaluated on
  float64 tensors with their own fp32 constants (the numbers ``functional.neuron_params()`` hands the kernels);
* the backward pass by autograd through all of the above.

Teacher forcing: the Heaviside of LIF takes the spike decisions of the kernel under test (``z_kernel``), so a spike that
flips within rounding of the threshold changes nothing downstream; the SuperSpike backward is unchanged.  The Synapse's
``x > 0`` choice of time constant is taken from the reference's own x; lanes where |x| is within fp32 rounding of 0 are
reported in ``near_zero`` for the caller to keep out of its elementwise bounds.
"""

from typing import NamedTuple, Optional

import torch

from oracle.net import SLICell, SynapseCell
from oracle.neurons import LIParameters, LIState, li_feed_forward_step

NONE, LIF, LI, LI_TANH, SLI, SYNAPSE = 0, 1, 2, 3, 4, 5   # SNN_NEURON_* of include/snn_hip.h
V_TH, V_RESET, ALPHA = 1.0, 0.0, 100.0                    # norse LIFParameters


class _ForcedSpike(torch.autograd.Function):
    """Forward: the given spikes.  Backward: SuperSpike, g / (alpha * |u| + 1)^2."""

    @staticmethod
    def forward(ctx, u, z, alpha):
        ctx.save_for_backward(u)
        ctx.alpha = alpha
        return z.to(u.dtype).clone()

    @staticmethod
    def backward(ctx, g):
        (u,) = ctx.saved_tensors
        return g / (ctx.alpha * u.abs() + 1.0).pow(2), None, None


class BnStats(NamedTuple):
    mean: torch.Tensor      # [T, C] (eval: the running mean, repeated)
    var: torch.Tensor       # [T, C] biased batch variance (eval: the running variance)
    xhat: torch.Tensor      # [T, B, C, H, W]
    invstd: torch.Tensor    # [T, C]
    running_mean: Optional[torch.Tensor]
    running_var: Optional[torch.Tensor]


def batch_norm(y, gamma, bias, training: bool, eps: float, momentum: float, running_mean=None, running_var=None,
               unbiased_running: bool = True):
    """``x[t] = BatchNorm2d(y[t])`` for every t; returns ``(x, BnStats)``.  y is [T, B, C, H, W]."""
    T, B, C, H, W = y.shape
    if training:
        mean = y.mean(dim=(1, 3, 4))
        var = (y - mean[:, None, :, None, None]).square().mean(dim=(1, 3, 4))
    else:
        mean = running_mean.to(y.dtype).expand(T, C)
        var = running_var.to(y.dtype).expand(T, C)
    invstd = (var + eps).rsqrt()
    xhat = (y - mean[:, None, :, None, None]) * invstd[:, None, :, None, None]
    x = xhat
    if gamma is not None:
        x = x * gamma[None, None, :, None, None]
    if bias is not None:
        x = x + bias[None, None, :, None, None]
    rm = rv = None
    if training and running_mean is not None:
        n = B * H * W
        rm, rv = running_mean.detach().to(y.dtype).clone(), running_var.detach().to(y.dtype).clone()
        for t in range(T):
            v = var[t].detach() * (n / (n - 1.0) if unbiased_running else 1.0)
            rm = (1.0 - momentum) * rm + momentum * mean[t].detach()
            rv = (1.0 - momentum) * rv + momentum * v
    return x, BnStats(mean, var, xhat, invstd, rm, rv)


class ScanResult(NamedTuple):
    out: torch.Tensor                 # [T, B, C, H, W], or [B, C, H, W] when last_only
    vT: Optional[torch.Tensor]
    iT: Optional[torch.Tensor]
    vdec: Optional[torch.Tensor]      # LIF: [T, B, C, H, W] membrane potential before the threshold
    near_zero: Optional[torch.Tensor]  # Synapse: [B, C, H, W] lanes whose x came within fp32 rounding of 0


def neuron_scan(x, neuron: int, v0=None, i0=None, z_kernel=None, alpha: float = ALPHA, sigma: float = 0.0,
                dt: float = 0.001, x_scale=None, last_only: bool = False) -> ScanResult:
    """The neuron over ``x`` [T, B, C, H, W] from state (v0, i0) (None: the cell's own initial state).

    ``z_kernel`` (LIF): the spikes to force.  ``x_scale`` (Synapse): |alpha*y| + |beta| per element, the magnitude that
    sets the fp32 rounding of the kernel's x.  ``dt``: the fp32 step the Synapse kernel uses."""
    T = x.shape[0]
    if neuron == NONE:
        return ScanResult(x[-1] if last_only else x, None, None, None, None)
    outs, vdecs = [], []
    if neuron == SYNAPSE:
        cell = SynapseCell(dt=dt, sigma_inhibition=sigma)
        state = None if v0 is None else (v0 + torch.zeros_like(x[0]),)
        near = torch.zeros_like(x[0], dtype=torch.bool)
        for t in range(T):
            g, state = cell(x[t], state)
            outs.append(g)
            if x_scale is not None:
                near |= x[t].detach().abs() <= 1e-6 * x_scale[t]
        out = torch.stack(outs)
        return ScanResult(out[-1] if last_only else out, state[0], None, None, near)
    if neuron == SLI:
        cell = SLICell()
        state = None if v0 is None else (v0, i0 if i0 is not None else torch.zeros_like(x[0]))
        for t in range(T):
            v_new, state = cell(x[t], state)
            outs.append(v_new)
        out = torch.stack(outs)
        return ScanResult(out[-1] if last_only else out, state[0] + torch.zeros_like(x[0]), state[1], None, None)
    p = LIParameters()
    v = v0 if v0 is not None else p.v_leak.to(x.dtype)
    i = i0 if i0 is not None else torch.zeros_like(x[0])
    for t in range(T):
        # LIF's sub-threshold step is the LI step: current jump, voltage, current decay (oracle/neurons.py)
        v_dec, st = li_feed_forward_step(x[t], LIState(v, i), p)
        i = st.i
        if neuron == LIF:
            z = _ForcedSpike.apply(v_dec - V_TH, z_kernel[t], alpha)
            v = (1 - z) * v_dec + z * V_RESET
            outs.append(z)
            vdecs.append(v_dec.detach())
        else:
            v = v_dec
            outs.append(torch.tanh(v_dec) if neuron == LI_TANH else v_dec)
    out = outs[-1] if last_only else torch.stack(outs)
    return ScanResult(out, v + torch.zeros_like(x[0]), i, torch.stack(vdecs) if vdecs else None, None)


def bn_backward_sums(gx, xhat, keep=None):
    """``(sum gx, sum gx * xhat)`` per (t, c) over (B, H, W); ``keep`` [B, H, W] (bool) restricts the pixels summed."""
    if keep is not None:
        w = keep[None, :, None].to(gx.dtype)
        gx, xhat = gx * w, xhat * w
    return gx.sum(dim=(1, 3, 4)), (gx * xhat).sum(dim=(1, 3, 4))


def bn_train_dy(gx, xhat, invstd, gamma, n: int, keep=None):
    """The train-mode BatchNorm input gradient in closed form, dy = gamma*invstd*(gx - mean(gx) - xhat*mean(gx*xhat)),
    from the sums of ``bn_backward_sums(gx, xhat, keep)`` (``keep`` lets a caller drop pixels from the sums)."""
    s1, s2 = bn_backward_sums(gx, xhat, keep)
    g = invstd if gamma is None else invstd * gamma[None, :]
    e = lambda a: a[:, None, :, None, None]   # noqa: E731
    return e(g) * (gx - e(s1) / n - xhat * e(s2) / n), s1, s2
