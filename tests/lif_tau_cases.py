"""The rows, inputs and reference runs that tests/test_gpu_lif_tau.py (on the device) and tests/test_lif_tau_host.py
(without one) share (TEST INFRASTRUCTURE ONLY; nothing here touches a device).

``Case``, the inputs, the result tuples and ``check_grads`` with its bound ``TOL_STATE`` are those of
tests/test_gpu_norm_neuron_fp64.py and tests/lif_gradient_cases.py, imported.  The shapes are those of
tests/test_lif_gradient_host.py::test_planner_accepts_and_refuses_rules (plus its 24-channel LDS-atomics neighbour and
the layer that stores no spikes): the smallest that reach each class of the reverse scan.
"""
from typing import NamedTuple, Optional, Tuple

import torch

from tests import lif_gradient_cases as G
from tests import lif_gradient_ref as L
from tests import lif_tau_ref as TR
from tests import norm_neuron_ref as R
from tests import test_gpu_norm_neuron_fp64 as F
from tests.test_gpu_norm_neuron_fp64 import Case, D

TAU_FACTOR = 16.0   # bound of dL/dw: this many times the float32 restatement's own error (see tests/test_gpu_lif_tau.py)


class Row(NamedTuple):
    cs: Case
    classes: Tuple[str, ...]
    ordered: int                               # the two sums in fixed order (0: LDS float atomics)
    learn: str = "channel"                     # "channel" or "layer"
    rule: Tuple[str, bool] = L.DEFAULT_RULE
    variant: str = "default"                   # "default" or "wide"
    multi_pixel: bool = False                  # buffer addressing, three pixel rows per thread, rpb > 3 and no multiple of 3


ROWS = [
    Row(Case("c4_vec4_ordered_state", R.LIF, 8, 2, 4, 7, 7, state=True), ("mode1", "vec4"), 1),
    Row(Case("c3_vec1_layer", R.LIF, 6, 2, 3, 9, 10), ("vec1", "mode2"), 0, learn="layer"),
    Row(Case("c16_nobn_mode0", R.LIF, 8, 2, 16, 6, 7, bn=None), ("mode0",), 1),
    Row(Case("c24_atomics_addend", R.LIF, 6, 2, 24, 6, 7, addend=True), ("mode2", "vec4"), 0),
    Row(Case("c512_gy_atan_detached", R.LIF, 32, 1, 512, 6, 7), ("mode1", "gy>1"), 1, rule=("atan", True)),
    Row(Case("c16_wide", R.LIF, 6, 2, 16, 6, 7), ("mode1",), 1, variant="wide"),
    Row(Case("c32_spikes_never_stored", R.LIF, 8, 2, 32, 6, 7, spikes_ok=True), ("mode1",), 1),
    # more than one pixel row per block, the last group of rows partial: the multi-pixel buffer-addressed instance the
    # production maps take (sums carried over the row groups, step 0's terms once per group, masked pixel slots)
    Row(Case("c16_rpb_gt1", R.LIF, 4, 4, 16, 159, 161), ("mode1", "rpb>1_partial"), 1, multi_pixel=True),
]


make_inputs = G.make_inputs   # (driven harder than F.make_inputs: see there)


def raw_parameters(row):
    """w_mem, w_syn (fp32, [C] or [1]) with c_mem in [0.1, 0.5] and 1 + c_syn in [0.5, 0.95], different in every channel."""
    C = row.cs.C
    g = torch.Generator().manual_seed(G.seed_of(row.cs) + 3)
    if row.learn == "layer":
        cm, s = torch.tensor([0.23], dtype=D), torch.tensor([0.8], dtype=D)
    else:
        cm = torch.linspace(0.1, 0.5, C, dtype=D)[torch.randperm(C, generator=g)]
        s = torch.linspace(0.5, 0.95, C, dtype=D)[torch.randperm(C, generator=g)]
    return torch.logit(cm).to(torch.float32), torch.logit(s).to(torch.float32)


def host_constants(row):
    """c_mem[C], c_syn[C] as fp32 torch forms them on the host (the device tests read the kernel's own back)."""
    w_mem, w_syn = raw_parameters(row)
    return torch.sigmoid(w_mem).expand(row.cs.C).clone(), (torch.sigmoid(w_syn) - 1.0).expand(row.cs.C).clone()


def neuron_input(cs, inp, dtype=D):
    with torch.no_grad():
        y = inp.y.to(dtype)
        if cs.bn is None:
            return y
        x, _ = L.batch_norm(y, inp.gamma.to(dtype), inp.bias.to(dtype), cs.bn == "train", 1e-5, 0.1, inp.rm.to(dtype),
                            inp.rv.to(dtype))
        return x


def state_of(cs, inp, dtype=D):
    return (inp.v0.to(dtype), inp.i0.to(dtype)) if cs.state else (None, None)


class TauRef(NamedTuple):
    ref: F.RefResult
    d_wmem: torch.Tensor
    d_wsyn: torch.Tensor
    d_cmem: torch.Tensor
    d_csyn: torch.Tensor


def run_ref(row, inp, z, c_mem, c_syn, dtype=D, rule: Optional[Tuple[str, bool]] = None) -> TauRef:
    """G.run_ref with the LIF of tests/lif_tau_ref.py: ``z`` are the spikes to force, ``c_mem`` / ``c_syn`` the [C] constants
    (their fp32 values, carried into ``dtype``); the whole run - BatchNorm, scan, backward - is in ``dtype`` on the host."""
    cs = row.cs
    rule = rule or row.rule
    y = inp.y.to(dtype).requires_grad_()
    cm, cn = c_mem.detach().cpu().to(dtype).requires_grad_(), c_syn.detach().cpu().to(dtype).requires_grad_()
    wrt = [y]
    gamma = st = None
    if cs.bn is not None:
        gamma = inp.gamma.to(dtype).requires_grad_()
        bias = inp.bias.to(dtype).requires_grad_()
        wrt += [gamma, bias]
        x, st = L.batch_norm(y, gamma, bias, cs.bn == "train", 1e-5, 0.1, inp.rm.to(dtype), inp.rv.to(dtype))
    else:
        x = y * 1.0
    v0 = i0 = None
    if cs.state:
        v0, i0 = inp.v0.to(dtype).requires_grad_(), inp.i0.to(dtype).requires_grad_()
        wrt += [v0, i0]
    r = TR.lif_tau_scan(x, z.cpu(), cm, cn, v0, i0, rule[0], G.SLOPE[rule[0]], rule[1])
    out = r.out
    if cs.addend:
        addend = inp.addend.to(dtype).requires_grad_()
        wrt.append(addend)
        out = out + addend
    outs, gouts = [out, r.vT, r.iT], [inp.g_out.to(dtype), inp.g_vT.to(dtype), inp.g_iT.to(dtype)]
    gr = torch.autograd.grad(outs, wrt + [x, cm, cn], gouts, allow_unused=True)
    names = ["dy"] + (["dgamma", "dbias"] if cs.bn is not None else []) + (["dv0", "di0"] if cs.state else []) + \
            (["daddend"] if cs.addend else [])
    grads = {k: v.detach() for k, v in zip(names, gr[:-3])}
    bn_st = None
    if st is not None:
        bn_st = R.BnStats(st.mean.detach(), st.var.detach(), st.xhat.detach(), st.invstd.detach(), st.running_mean,
                          st.running_var)
    ref = F.RefResult(out.detach(), r.vdec, r.vT.detach(), r.iT.detach(),
                      None if st is None else st.running_mean, None if st is None else st.running_var,
                      grads, gr[-3].detach(), bn_st, None if gamma is None else gamma.detach(), None)
    d_cmem, d_csyn = gr[-2].detach(), gr[-1].detach()
    d_wmem, d_wsyn = TR.chain_rule(d_cmem, d_csyn, cm.detach(), cn.detach(), row.learn == "layer")
    return TauRef(ref, d_wmem, d_wsyn, d_cmem, d_csyn)


def rel_err(got, ref):
    """The measure of the new quantities: ||got - ref||_2 / ||ref||_2 per tensor."""
    ref = ref.to(D)
    return float((got.detach().cpu().to(D) - ref).norm() / ref.norm())


def yardstick(row, inp, z, c_mem, c_syn, ref64: TauRef):
    """The float32 restatement's own error of (dL/dw_mem, dL/dw_syn) against float64, same inputs, same forced spikes."""
    r32 = run_ref(row, inp, z, c_mem, c_syn, torch.float32)
    return rel_err(r32.d_wmem, ref64.d_wmem), rel_err(r32.d_wsyn, ref64.d_wsyn)
