"""The rows, inputs and float64 reference runs that tests/test_gpu_lif_gradient.py (on the device) and
tests/test_lif_gradient_host.py (without one) share (TEST INFRASTRUCTURE ONLY; nothing here touches a device).

``Case``, ``make_inputs``, the result tuples and ``check_grads`` - with its bound ``TOL_STATE`` and its norm-wise grouping -
are those of tests/test_gpu_norm_neuron_fp64.py, imported, not copied: the new rule is held to the bounds of the old one.
"""
import zlib
from typing import NamedTuple, Tuple

import torch

from tests import lif_gradient_ref as L
from tests import norm_neuron_ref as R
from tests import test_gpu_norm_neuron_fp64 as F
from tests.test_gpu_norm_neuron_fp64 import Case, D

SLOPE = {"super": 100.0, "triangle": 100.0, "atan": 100.0, "sigmoid": 200.0}
COMMON_RULES = (("triangle", True), ("super", True))


class Row(NamedTuple):
    cs: Case
    classes: Tuple[str, ...] = ()             # plan classes (F.plan_classes) the row is there for
    variants: Tuple[str, ...] = ("default",)  # "default", "no_yfree", "wide": as F.run_device selects them
    rules: Tuple[Tuple[str, bool], ...] = COMMON_RULES
    v_ths: Tuple[float, ...] = (1.0,)
    lookback: bool = False                    # the default variant must take the from-state sums with look-back


ROWS = [
    Row(Case("c4_partial_row", R.LIF, 8, 2, 4, 7, 7), ("mode1", "vec4", "rpb1_partial"), rules=L.RULES),
    Row(Case("c4_partial_row_vth08", R.LIF, 8, 2, 4, 7, 7), ("mode1", "vec4", "rpb1_partial"), v_ths=(0.8,)),
    Row(Case("c3_vec1", R.LIF, 6, 2, 3, 9, 10), ("vec1", "mode2")),
    Row(Case("nobn_mode0", R.LIF, 8, 2, 16, 6, 7, bn=None), ("mode0",)),
    Row(Case("evalgrad_apply_scale", R.LIF, 6, 2, 64, 5, 6, bn="eval_grad"), ("mode1",)),
    Row(Case("carried_state", R.LIF, 6, 2, 8, 9, 11, state=True), ("mode1",)),
    Row(Case("t70_segments", R.LIF, 70, 1, 16, 5, 6), ("mode1",), variants=("default", "no_yfree"), lookback=True),
    Row(Case("c512_gy", R.LIF, 32, 1, 512, 6, 7), ("mode1", "gy>1")),
    Row(Case("spikes_never_stored", R.LIF, 8, 2, 32, 6, 7, spikes_ok=True), ("mode1",), v_ths=(0.8,)),
    Row(Case("wide_addressing", R.LIF, 6, 2, 16, 6, 7), ("mode1",), variants=("wide",)),
    Row(Case("last_step_only", R.LIF, 6, 2, 16, 6, 7, last_only=True), ("mode1",)),
    # more than one pixel row per block: the four-pixel instance of the plain scan and the multi-pixel from-state ones,
    # which the production maps take and none of the small rows above reaches
    Row(Case("rpb_gt1", R.LIF, 8, 4, 16, 90, 100), ("mode1", "rpb>1_partial"), variants=("default", "no_yfree"),
        rules=(("triangle", True),)),
]
def seed_of(cs):
    return zlib.crc32(cs.id.encode()) % 10007


def make_inputs(cs):
    """F.make_inputs, driven harder: that file's short rows hardly spike (0.5 % of the decisions at T = 6), and the rules
    differ where potentials lie near the threshold and a gradient arrives through the reset.  The neuron input gets a
    positive mean (BatchNorm bias + 0.8, gamma x 1.5 - gamma[0] = 0 and gamma[1] < 0 stay; without BatchNorm y itself), so
    potentials cross the threshold from the second step on and keep crossing it after every reset, and the final state
    always has a gradient (g_vT, g_iT), carried state or not."""
    inp = F.make_inputs(cs, seed_of(cs))
    g = torch.Generator().manual_seed(seed_of(cs) + 1)
    shape = (cs.B, cs.C, cs.H, cs.W)
    return inp._replace(gamma=1.5 * inp.gamma, bias=inp.bias + 0.8, y=inp.y if cs.bn is not None else inp.y + 0.8,
                        g_vT=torch.randn(shape, generator=g), g_iT=torch.randn(shape, generator=g))


# ------------------------------------------------------------------------------------------------------ reference
def run_ref(cs, inp, z, rule, v_th=1.0, dev="cpu"):
    """F.run_ref with the LIF of tests/lif_gradient_ref.py: ``z`` are the spikes to force ([T, B, C, H, W])."""
    y = inp.y.to(dev, D).requires_grad_()
    wrt = [y]
    gamma = bias = st = None
    if cs.bn is not None:
        gamma = inp.gamma.to(dev, D).requires_grad_()
        bias = inp.bias.to(dev, D).requires_grad_()
        wrt += [gamma, bias]
        x, st = L.batch_norm(y, gamma, bias, cs.bn == "train", 1e-5, 0.1, inp.rm.to(dev, D), inp.rv.to(dev, D))
    else:
        x = y * 1.0
    v0 = i0 = None
    if cs.state:
        v0 = inp.v0.to(dev, D).requires_grad_()
        i0 = inp.i0.to(dev, D).requires_grad_()
        wrt += [v0, i0]
    r = L.lif_scan(x, z.to(dev), v0, i0, rule[0], SLOPE[rule[0]], rule[1], v_th, L.V_RESET, cs.last_only)
    outs, gouts = [r.out, r.vT, r.iT], [inp.g_out.to(dev, D), inp.g_vT.to(dev, D), inp.g_iT.to(dev, D)]
    gr = torch.autograd.grad(outs, wrt + [x], gouts, allow_unused=True)
    names = ["dy"] + (["dgamma", "dbias"] if cs.bn is not None else []) + (["dv0", "di0"] if cs.state else [])
    grads = {k: v.detach() for k, v in zip(names, gr[:-1])}
    bn_st = None
    if st is not None:
        bn_st = R.BnStats(st.mean.detach(), st.var.detach(), st.xhat.detach(), st.invstd.detach(), st.running_mean,
                          st.running_var)
    return F.RefResult(r.out.detach(), r.vdec, r.vT.detach(), r.iT.detach(),
                       None if st is None else (st.running_mean if cs.bn == "train" else inp.rm.to(dev, D)),
                       None if st is None else (st.running_var if cs.bn == "train" else inp.rv.to(dev, D)),
                       grads, gr[-1].detach(), bn_st, None if gamma is None else gamma.detach(), None)


def reference_spikes(cs, inp, v_th=1.0):
    """The reference's own spike decisions on a row's inputs (what a test without a kernel forces)."""
    with torch.no_grad():
        y = inp.y.to(D)
        x = y
        if cs.bn is not None:
            x, _ = L.batch_norm(y, inp.gamma.to(D), inp.bias.to(D), cs.bn == "train", 1e-5, 0.1, inp.rm.to(D), inp.rv.to(D))
    return L.spikes_of(x, None if not cs.state else inp.v0.to(D), None if not cs.state else inp.i0.to(D), v_th)


def dy_distance(cs, ref_a, ref_b):
    """max over the groups of ||dy_a - dy_b|| / (TOL_STATE ||s||), s formed from ref_b: the very quantity F.check_grads
    bounds by 1 between the kernel and the reference."""
    rec = {}
    as_device = F.DevResult(None, None, None, None, None, None, {"dy": ref_a.grads["dy"]}, True)
    F.check_grads(cs, as_device, ref_b, [], rec, grads={"dy": ref_b.grads["dy"]})
    return rec["dy"]
