"""Float64 restatement of the LIF layer with a selectable backward rule (TEST INFRASTRUCTURE ONLY).

Plain torch float64 in the structure of ``tests/norm_neuron_ref.py``'s LIF branch (whose BatchNorm and constants it
imports): the sub-threshold step is the LI step of ``oracle/neurons.py``, the Heaviside takes the spike decisions of the
kernel under test (teacher forcing, as there), and the backward pass is autograd through

* one autograd function per surrogate ``dz/du`` of ``include/snn_hip.h`` (``SNN_SURR_*``; u = v_dec - v_th, a = alpha,
  every one with value 1 at u = 0):

      super     1 / (a|u| + 1)^2
      triangle  max(0, 1 - a|u|)
      sigmoid   4 s(au) (1 - s(au)),  s(x) = 1 / (1 + exp(-x))
      atan      1 / (1 + (au)^2)

* the reset ``v = (1 - z) v_dec + z v_reset`` with z as it is (default) or ``z.detach()`` (``detach_reset``).

Nothing here calls into the package.
"""

from typing import Optional

import torch

from oracle.neurons import LIParameters, LIState, li_feed_forward_step
from tests.norm_neuron_ref import ALPHA, LIF, V_RESET, V_TH, ScanResult, batch_norm  # noqa: F401  (re-exported)

SURROGATE_NAMES = ("super", "triangle", "sigmoid", "atan")
RULES = tuple((s, d) for s in SURROGATE_NAMES for d in (False, True))   # (surrogate, detach_reset)
DEFAULT_RULE = ("super", False)


def surrogate_super(u, a):
    return 1.0 / (a * u.abs() + 1.0).pow(2)


def surrogate_triangle(u, a):
    return (1.0 - a * u.abs()).clamp_min(0.0)


def surrogate_sigmoid(u, a):
    s = torch.sigmoid(a * u)
    return 4.0 * s * (1.0 - s)


def surrogate_atan(u, a):
    return 1.0 / (1.0 + (a * u).pow(2))


SURROGATES = {"super": surrogate_super, "triangle": surrogate_triangle, "sigmoid": surrogate_sigmoid,
              "atan": surrogate_atan}


def _forced_spike(fn):
    class _Forced(torch.autograd.Function):
        """Forward: the given spikes.  Backward: g * dz/du of one surrogate."""

        @staticmethod
        def forward(ctx, u, z, alpha):
            ctx.save_for_backward(u)
            ctx.alpha = alpha
            return z.to(u.dtype).clone()

        @staticmethod
        def backward(ctx, g):
            (u,) = ctx.saved_tensors
            return g * fn(u, ctx.alpha), None, None

    _Forced.__name__ = f"_Forced_{fn.__name__}"
    return _Forced


FORCED_SPIKE = {name: _forced_spike(fn) for name, fn in SURROGATES.items()}


def lif_scan(x, z_kernel, v0=None, i0=None, surrogate: str = "super", alpha: float = ALPHA, detach_reset: bool = False,
             v_th: float = V_TH, v_reset: float = V_RESET, last_only: bool = False) -> ScanResult:
    """LIF over ``x`` [T, B, C, H, W] from state (v0, i0) (None: v_leak = 0, i = 0), spikes forced to ``z_kernel``."""
    spike = FORCED_SPIKE[surrogate]
    p = LIParameters()
    v = v0 if v0 is not None else p.v_leak.to(x.dtype)
    i = i0 if i0 is not None else torch.zeros_like(x[0])
    outs, vdecs = [], []
    for t in range(x.shape[0]):
        v_dec, st = li_feed_forward_step(x[t], LIState(v, i), p)
        i = st.i
        z = spike.apply(v_dec - v_th, z_kernel[t], alpha)
        zr = z.detach() if detach_reset else z
        v = (1 - zr) * v_dec + zr * v_reset
        outs.append(z)
        vdecs.append(v_dec.detach())
    out = outs[-1] if last_only else torch.stack(outs)
    return ScanResult(out, v + torch.zeros_like(x[0]), i, torch.stack(vdecs), None)


def spikes_of(x, v0=None, i0=None, v_th: float = V_TH, v_reset: float = V_RESET) -> torch.Tensor:
    """The reference's OWN spike decisions (no kernel at hand: the host tests force these)."""
    p = LIParameters()
    v = v0 if v0 is not None else p.v_leak.to(x.dtype)
    i = i0 if i0 is not None else torch.zeros_like(x[0])
    zs = []
    with torch.no_grad():
        for t in range(x.shape[0]):
            v_dec, st = li_feed_forward_step(x[t], LIState(v, i), p)
            i = st.i
            z = (v_dec - v_th > 0).to(x.dtype)
            v = (1 - z) * v_dec + z * v_reset
            zs.append(z)
    return torch.stack(zs)
