"""Float64 restatement of the LIF layer with per-channel time constants (TEST INFRASTRUCTURE ONLY).

The step of ``include/snn_hip.h`` with ``c_mem`` and ``c_syn`` as ``[C]`` tensors that may require a gradient:

    i'[t] = i[t-1] + x[t]
    vd[t] = v[t-1] + c_mem[c] ((v_leak - v[t-1]) + i'[t])
    i[t]  = i'[t] + c_syn[c] i'[t]
    z[t]  = (vd[t] - v_th > 0);   v[t] = (1 - z) vd[t] + z v_reset

in the structure of ``tests/lif_gradient_ref.py`` (whose forced spikes - one autograd function per surrogate - it imports):
the Heaviside takes the spike decisions handed in (teacher forcing), the backward pass is autograd, the reset sees the
spike as it is or detached.  The step is restated here, not taken from ``oracle/``.  Every tensor handed in decides the
precision: float64 for the reference, float32 (on the CPU) for the yardstick of the bounds.  ``chain_rule`` turns the
gradients of the constants into those of the raw parameters under ``c_mem = sigmoid(w_mem)``, ``1 + c_syn =
sigmoid(w_syn)``.  Nothing here calls into the package.
"""
import torch

from tests.lif_gradient_ref import FORCED_SPIKE
from tests.norm_neuron_ref import ALPHA, V_RESET, V_TH, ScanResult

V_LEAK = 0.0


def _per_channel(c, like):
    return c.to(like.dtype).reshape(1, -1, 1, 1)


def lif_tau_scan(x, z_kernel, c_mem, c_syn, v0=None, i0=None, surrogate: str = "super", alpha: float = ALPHA,
                 detach_reset: bool = False, v_th: float = V_TH, v_reset: float = V_RESET, v_leak: float = V_LEAK) -> ScanResult:
    """LIF over ``x`` [T, B, C, H, W] from state (v0, i0) (None: v_leak, 0), spikes forced to ``z_kernel``."""
    spike = FORCED_SPIKE[surrogate]
    cm, cs = _per_channel(c_mem, x), _per_channel(c_syn, x)
    v = v0 if v0 is not None else torch.full_like(x[0], v_leak)
    i = i0 if i0 is not None else torch.zeros_like(x[0])
    outs, vdecs = [], []
    for t in range(x.shape[0]):
        i_new = i + x[t]
        v_dec = v + cm * ((v_leak - v) + i_new)
        i = i_new + cs * i_new
        z = spike.apply(v_dec - v_th, z_kernel[t].to(x.dtype), alpha)
        zr = z.detach() if detach_reset else z
        v = (1 - zr) * v_dec + zr * v_reset
        outs.append(z)
        vdecs.append(v_dec.detach())
    return ScanResult(torch.stack(outs), v + torch.zeros_like(x[0]), i, torch.stack(vdecs), None)


def spikes_of(x, c_mem, c_syn, v0=None, i0=None, v_th: float = V_TH, v_reset: float = V_RESET, v_leak: float = V_LEAK):
    """The restatement's OWN spike decisions, in the precision of ``x`` (no kernel at hand: the host tests force these)."""
    cm, cs = _per_channel(c_mem, x), _per_channel(c_syn, x)
    v = v0 if v0 is not None else torch.full_like(x[0], v_leak)
    i = i0 if i0 is not None else torch.zeros_like(x[0])
    zs, vds = [], []
    with torch.no_grad():
        for t in range(x.shape[0]):
            i_new = i + x[t]
            v_dec = v + cm * ((v_leak - v) + i_new)
            i = i_new + cs * i_new
            z = (v_dec - v_th > 0).to(x.dtype)
            v = (1 - z) * v_dec + z * v_reset
            zs.append(z)
            vds.append(v_dec)
    return torch.stack(zs), torch.stack(vds)


def chain_rule(d_cmem, d_csyn, c_mem, c_syn, per_layer: bool):
    """dL/dw_mem = dL/dc_mem c_mem (1 - c_mem), dL/dw_syn = dL/dc_syn s (1 - s) with s = 1 + c_syn; per layer: summed."""
    s = 1.0 + c_syn
    dm, ds = d_cmem * c_mem * (1.0 - c_mem), d_csyn * s * (1.0 - s)
    return (dm.sum().reshape(1), ds.sum().reshape(1)) if per_layer else (dm, ds)
