"""Hand-derived cases that pin tests/norm_neuron_ref.py (the fp64 restatement of the fused Norm -> neuron layer that
tests/test_gpu_norm_neuron_fp64.py checks the kernels against).  Host only.  Each case states its derivation.

Constants: c_mem = fp32(1e-3 * 100) = 0.1 + 1.49e-9 and c_syn = fp32(-1e-3 * 200) = -0.2 - 2.98e-9 (oracle/neurons.py);
from v = v_leak = 0, i = 0 one step gives v_dec = c_mem * x and i = (1 + c_syn) * x.
"""
import pytest
import torch

from oracle.neurons import neuron_constants
from tests.norm_neuron_ref import LI_TANH, LIF, batch_norm, bn_train_dy, neuron_scan

C_MEM, C_SYN = neuron_constants()[:2]
D = torch.float64


def _x(*vals):
    return torch.tensor(vals, dtype=D).reshape(len(vals), 1, 1, 1, 1)


def test_one_spike_and_its_reset():
    # step 0: x = 20 -> v_dec = 20 c_mem = 2 > 1: spike, v = v_reset = 0, i = 20 (1 + c_syn) = 16
    # step 1: x = -16, so that i_new = 16 - 16 = 0: v_dec = c_mem * ((0 - 0) + 0) = 0, no spike
    i1 = 20.0 * (1.0 + C_SYN)
    x = _x(20.0, -i1).requires_grad_()
    z = torch.tensor([1.0, 0.0], dtype=D).reshape(2, 1, 1, 1, 1)
    r = neuron_scan(x, LIF, z_kernel=z)
    assert r.out.flatten().tolist() == [1.0, 0.0]
    assert r.vdec[0].item() == pytest.approx(20.0 * C_MEM, rel=1e-15)
    assert r.vdec[1].item() == 0.0 and r.vT.item() == 0.0 and r.iT.item() == pytest.approx(0.0, abs=1e-15)
    # d z0 / d x0 = SuperSpike(u0) * c_mem with u0 = 20 c_mem - 1 (the reset's own path carries g = 0 here)
    (g,) = torch.autograd.grad(r.out[0].sum(), x, retain_graph=True)
    u0 = 20.0 * C_MEM - 1.0
    assert g[0].item() == pytest.approx(C_MEM / (100.0 * u0 + 1.0) ** 2, rel=1e-13)
    assert g[1].item() == 0.0
    # the reset is differentiable through z: v0' = (1 - z0) v_dec0 + z0 v_reset has d v0' / d x0 = -v_dec0 * s0 * c_mem
    # (z0 = 1 zeroes the direct term), and v_dec1 = v0' + c_mem ((0 - v0') + i0' + x1) with i0' = (1 + c_syn) x0; step 1's
    # v_1 = (1 - z1) v_dec1 + z1 v_reset has d v_1 / d v_dec1 = 1 - z1 + (v_reset - v_dec1) s1 = 1 (v_dec1 = 0)
    (gv,) = torch.autograd.grad(r.vT.sum(), x)
    s0 = 1.0 / (100.0 * u0 + 1.0) ** 2
    dvdec1_dx0 = (1.0 - C_MEM) * (-(20.0 * C_MEM) * s0 * C_MEM) + C_MEM * (1.0 + C_SYN)
    assert gv[0].item() == pytest.approx(dvdec1_dx0, rel=1e-12)


def test_li_tanh_derivative():
    # one step from rest: out = tanh(c_mem x), d out / d x = c_mem (1 - tanh^2(c_mem x))
    x = _x(3.0).requires_grad_()
    r = neuron_scan(x, LI_TANH)
    assert r.out.item() == pytest.approx(torch.tanh(torch.tensor(3.0 * C_MEM, dtype=D)).item(), rel=1e-15)
    (g,) = torch.autograd.grad(r.out.sum(), x)
    t = torch.tanh(torch.tensor(3.0 * C_MEM, dtype=D)).item()
    assert g.item() == pytest.approx(C_MEM * (1.0 - t * t), rel=1e-14)


def test_per_timestep_statistics_on_a_two_pixel_batch():
    # y[t] = (a_t, b_t) on one channel: mean (a+b)/2, biased variance ((a-b)/2)^2, xhat = +-|a-b|/2 / sqrt(var + eps)
    y = torch.tensor([[1.0, 3.0], [-2.0, 6.0]], dtype=D).reshape(2, 1, 1, 1, 2)
    eps = 1e-5
    gamma = torch.tensor([2.0], dtype=D)
    bias = torch.tensor([0.5], dtype=D)
    x, st = batch_norm(y, gamma, bias, True, eps, 0.1)
    assert st.mean.flatten().tolist() == [2.0, 2.0]
    assert st.var.flatten().tolist() == [1.0, 16.0]
    for t, (d, var) in enumerate(((1.0, 1.0), (4.0, 16.0))):
        xh = d / (var + eps) ** 0.5
        assert x[t].flatten().tolist() == pytest.approx([0.5 - 2.0 * xh, 0.5 + 2.0 * xh], rel=1e-15)
    # the closed-form input gradient agrees with autograd through the same statement
    yr = y.clone().requires_grad_()
    xr, st = batch_norm(yr, gamma, bias, True, eps, 0.1)
    g = torch.tensor([[0.3, -1.1], [2.0, 0.7]], dtype=D).reshape(2, 1, 1, 1, 2)
    (dy,) = torch.autograd.grad(xr, yr, g)
    dy2, s1, s2 = bn_train_dy(g, st.xhat, st.invstd, gamma, 2)
    assert torch.allclose(dy, dy2, rtol=1e-13, atol=1e-15)
    assert s1.flatten().tolist() == pytest.approx([-0.8, 2.7], rel=1e-15)


def test_one_running_update():
    # T = 1, n = 2 pixels: running_mean = 0.9 * 0 + 0.1 * 2, running_var = 0.9 * 1 + 0.1 * (1 * 2 / 1)
    y = torch.tensor([1.0, 3.0], dtype=D).reshape(1, 1, 1, 1, 2)
    _, st = batch_norm(y, None, None, True, 1e-5, 0.1, torch.zeros(1, dtype=D), torch.ones(1, dtype=D))
    assert st.running_mean.item() == pytest.approx(0.2, rel=1e-15)
    assert st.running_var.item() == pytest.approx(1.1, rel=1e-15)
    # ... and the biased form a wrong reference would use differs: 0.9 + 0.1 * 1
    _, st = batch_norm(y, None, None, True, 1e-5, 0.1, torch.zeros(1, dtype=D), torch.ones(1, dtype=D),
                       unbiased_running=False)
    assert st.running_var.item() == pytest.approx(1.0, rel=1e-15)
