"""The fused Norm -> neuron scans (csrc/scan_fwd.hip, scan_bwd.hip, with the BatchNorm passes of bn_stats.hip and
bn_bwd.hip) against the float64 restatement of tests/norm_neuron_ref.py.

Every row of CASES calls ``functional.affine_neuron`` forward and backward and compares outputs, final state, running
statistics and every gradient with the reference.  Each row states the reverse-scan plan classes it is there for and
proves it through ``snn_affine_neuron_bwd_plan`` on this device's CU count; ``test_every_plan_class_is_reached`` checks
that the table reaches every class.  The production rows (B = 5, T = 32, TinyYolo's LIF layers at 240x304) run the
reference on the device in torch float64 and share it across their path variants.

Bounds (each derived where it is used):
* forward values: |d - r| <= 1e-5 (1 + |r|) elementwise; spikes exact except where |v_dec - v_th| <= 1e-5 (fp64), at most
  1e-4 of all spike decisions;
* gradients: norm-wise per group, ||d - r|| <= tol * ||s|| where s is the magnitude of the terms that form the gradient
  (cancellation in the BatchNorm backward must not loosen the bound: s is formed from absolute values), groups = each
  timestep and each 4-channel group for dy; per channel for dgamma / dbias.
The observed maxima (error / bound) per row are written as JSON to the file SNN_FP64_RECORD names, when it is set.
"""
import json
import os
import zlib
from typing import NamedTuple, Optional, Tuple

import pytest
import torch

from tests import norm_neuron_ref as R

pytestmark = pytest.mark.gpu

D = torch.float64
NAN_BITS = 0x7FC00000

# Gradient bounds.  Linear reverse scans (NONE, LI, LI+Tanh): each step rounds 2-4 fp32 operations (2^-24 each) inside a
# recurrence of gain <= 1 / (1 - 0.9) = 10 (the voltage leak), and the BatchNorm partial sums add <= rpb * NP + 6 <= 60
# fp32 terms per block: 10 * 4 * 6e-8 + 60 * 6e-8 = 6e-6 < 1e-5.
TOL_LINEAR = 1e-5
# State-dependent scans (LIF, SLI, Synapse): the backward coefficient is a function of the fp32 forward state.  LIF's
# SuperSpike factor s(u) = (alpha |u| + 1)^-2 has |s'/s| <= 2 alpha = 200; the fp32 potential carries the rounding of
# ~4 operations per step through the leak's gain of 10, 10 * 4 * 6e-8 = 2.4e-7 relative to |v| <= ~2: 200 * 4.8e-7 ~ 1e-4.
TOL_STATE = 1e-4
FWD_REL = 1e-5          # elementwise forward bound, |d - r| <= FWD_REL (1 + |r|): the derivation is the linear one above


def _tol(neuron):
    return TOL_LINEAR if neuron in (R.NONE, R.LI, R.LI_TANH) else TOL_STATE


class Case(NamedTuple):
    id: str
    neuron: int
    T: int
    B: int
    C: int
    H: int
    W: int
    bn: Optional[str] = "train"        # "train", "eval" (gamma / bias need no gradient), "eval_grad", None
    classes: Tuple[str, ...] = ()      # reverse-scan plan classes the row is there for
    variants: Tuple[str, ...] = ("default",)
    state: bool = False                # carried NeuronState(v0, i0) with g_vT / g_iT
    v0_scalar: bool = False            # LI's 0-dim initial v
    addend: bool = False
    y_off: Optional[int] = None        # y = channels [y_off, y_off + C) of a (C + 8)-channel buffer
    dest: bool = False                 # output into a Dest concat slice with NaN guard channels
    last_only: bool = False
    spikes_ok: bool = False
    sigma: float = 0.0
    special_gamma: bool = True         # gamma[0] = 0, gamma[1] < 0


CASES = [
    # ---- plan classes on small maps (reference on the host)
    Case("lif_c4_cvb1", R.LIF, 8, 2, 4, 7, 7, classes=("mode1", "vec4", "cvb1", "rpb1_partial")),
    Case("lif_c8_cvb2_state", R.LIF, 6, 2, 8, 9, 11, classes=("mode1", "cvb2"), state=True),
    Case("li_c16_cvb4_state0d", R.LI, 5, 2, 16, 6, 7, classes=("mode1", "cvb4"), state=True, v0_scalar=True),
    Case("litanh_c32_cvb8", R.LI_TANH, 7, 2, 32, 5, 9, classes=("mode1", "cvb8")),
    Case("none_c24_mode2", R.NONE, 6, 2, 24, 7, 8, classes=("mode2", "cvb_np2_lt64")),
    Case("sli_c36_mode2", R.SLI, 5, 2, 36, 6, 6, classes=("mode2", "cvb_np2_lt64")),
    Case("syn_c100_sigma0", R.SYNAPSE, 4, 1, 100, 7, 9, classes=("mode2", "cvb_np2_lt64")),
    Case("syn_c8_sigma07", R.SYNAPSE, 6, 2, 8, 8, 8, sigma=0.7),
    Case("lif_c3_vec1", R.LIF, 6, 2, 3, 9, 10, classes=("vec1", "mode2")),
    Case("li_c6_vec1_evalgrad", R.LI, 5, 2, 6, 7, 7, bn="eval_grad", classes=("vec1", "mode2")),
    Case("lif_c64_evalgrad", R.LIF, 6, 2, 64, 5, 6, bn="eval_grad", classes=("mode1", "cvb16")),
    Case("lif_c384_t4_idle_wave", R.LIF, 4, 1, 384, 10, 12, classes=("mode1", "cvb_np2_ge64")),
    Case("lif_c512_gy", R.LIF, 32, 1, 512, 6, 7, classes=("mode1", "gy>1")),
    Case("lif_nobn", R.LIF, 8, 2, 16, 6, 7, bn=None, classes=("mode0",)),
    Case("li_nobn_state", R.LI, 8, 2, 12, 6, 7, bn=None, classes=("mode0",), state=True),
    Case("lif_eval_scale_only", R.LIF, 6, 2, 16, 6, 7, bn="eval", classes=("mode0",)),
    Case("lif_t1", R.LIF, 1, 2, 16, 6, 7),
    Case("lif_t2", R.LIF, 2, 2, 16, 6, 7),
    Case("li_t2_nobn", R.LI, 2, 2, 8, 4, 5, bn=None),
    Case("lif_t70_segments", R.LIF, 70, 1, 16, 5, 6, variants=("default", "no_yfree")),
    Case("lif_t33_segments", R.LIF, 33, 1, 16, 5, 6),
    Case("lif_t70_segments_state", R.LIF, 70, 1, 8, 5, 6, state=True),
    Case("lif_addend", R.LIF, 6, 2, 16, 6, 7, addend=True),
    Case("li_addend_state", R.LI, 6, 2, 16, 6, 7, addend=True, state=True),
    Case("lif_y_slice_aligned", R.LIF, 6, 2, 16, 6, 7, y_off=4),
    Case("lif_y_slice_offset1", R.LIF, 6, 2, 16, 6, 7, y_off=1),
    Case("lif_y_slice_offset1_nobn", R.LIF, 6, 2, 16, 6, 7, bn=None, y_off=1),
    Case("syn_y_slice_offset1", R.SYNAPSE, 5, 2, 8, 5, 6, y_off=1),
    Case("lif_dest", R.LIF, 6, 2, 16, 6, 7, dest=True),
    Case("li_dest", R.LI, 6, 2, 12, 6, 7, dest=True),
    Case("lif_spikes_ok", R.LIF, 8, 2, 32, 6, 7, spikes_ok=True),
    Case("lif_rpb_gt1", R.LIF, 8, 4, 16, 90, 100, classes=("rpb>1_partial",), variants=("default", "no_yfree", "ckpt")),
    # ---- one launch over a long sequence (NONE is never segmented): all T slabs in LDS cap the channels per block
    Case("none_c64_t70", R.NONE, 70, 2, 64, 5, 6, classes=("mode1", "lds_capped", "cvb4", "gy>1")),
    Case("none_c100_t128", R.NONE, 128, 1, 100, 3, 4, classes=("mode2", "lds_capped")),
    # ---- TinyYolo's LIF layers at 240x304, B = 5, T = 32 (reference on the device)
    Case("prod_lif64_120x152", R.LIF, 32, 5, 64, 120, 152, classes=("mode1", "cvb16"),
         variants=("default", "no_yfree")),
    Case("prod_lif128_60x76", R.LIF, 32, 5, 128, 60, 76, classes=("mode1", "gy>1"), variants=("default", "ckpt")),
    Case("prod_lif256_30x38", R.LIF, 32, 5, 256, 30, 38, classes=("mode1", "gy>1", "rpb>1_partial"),
         variants=("default", "no_yfree", "wide", "ckpt")),
    Case("prod_lif256_15x19", R.LIF, 32, 5, 256, 15, 19, classes=("gy>1", "rpb1_partial"), variants=("default", "no_yfree")),
    Case("prod_litanh256_30x38_last", R.LI_TANH, 32, 5, 256, 30, 38, last_only=True, classes=("gy>1", "rpb>1_partial")),
]
REQUIRED_CLASSES = {"mode0", "mode1", "mode2", "vec1", "vec4", "cvb1", "cvb2", "cvb4", "cvb8", "cvb16", "cvb_np2_lt64",
                    "cvb_np2_ge64", "gy>1", "rpb1_partial", "rpb>1_partial", "lds_capped"}
_RECORD = {}


def _is_prod(cs):
    return cs.B * cs.T * cs.C * cs.H * cs.W > 5_000_000


@pytest.fixture(scope="module")
def HF(hip_lib):
    from snn_for_object_detection_amd import functional
    return functional


def _with_sums(cs):
    return cs.bn in ("train", "eval_grad")


def plan_of(HF, cs, variant="default", one_launch=False):
    """The plan of the (first segment's) reverse scan this row takes; ``one_launch``: of the scan over all T steps, which
    a SyncBatchNorm layer launches however long the sequence is."""
    from snn_for_object_detection_amd import _hip
    segmented = (not one_launch and _with_sums(cs) and cs.neuron != R.NONE and HF.SCAN_SEGMENT_T
                 and cs.T > HF.SCAN_SEGMENT_T)
    T = HF.SCAN_SEGMENT_T if segmented else cs.T
    flags = _hip.SCAN_WIDE_ADDRESSING if variant == "wide" else 0
    return HF.affine_neuron_bwd_plan(cs.neuron, T, cs.B * cs.H * cs.W, cs.C, cs.C, cs.C, _with_sums(cs), flags)


def plan_classes(pl):
    c = {f"mode{pl.mode}", f"vec{pl.vec}"}
    p2 = (pl.cvb & (pl.cvb - 1)) == 0
    if p2 and pl.cvb <= 16:
        c.add(f"cvb{pl.cvb}")
    elif not p2:
        c.add("cvb_np2_lt64" if pl.cvb < 64 else "cvb_np2_ge64")
    if pl.gy > 1:
        c.add("gy>1")
    # the slabs of all T steps did not leave room for min(C / vec, 256) channel groups per block: gy = ceil((C / vec) / cvb),
    # so cvb < C / vec is gy > 1
    if pl.gy > 1 and pl.cvb < 256:
        c.add("lds_capped")
    if pl.partial_row:
        c.add("rpb1_partial" if pl.rpb == 1 else "rpb>1_partial")
    return c


# ------------------------------------------------------------------------------------------------------ inputs
class Inputs(NamedTuple):
    y: torch.Tensor           # [T, B, C, H, W] fp32 (host)
    gamma: torch.Tensor
    bias: torch.Tensor
    rm: torch.Tensor
    rv: torch.Tensor
    v0: Optional[torch.Tensor]
    i0: Optional[torch.Tensor]
    addend: Optional[torch.Tensor]
    g_out: torch.Tensor
    g_vT: Optional[torch.Tensor]
    g_iT: Optional[torch.Tensor]


def make_inputs(cs, seed):
    g = torch.Generator().manual_seed(seed)
    T, B, C, H, W = cs.T, cs.B, cs.C, cs.H, cs.W
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    shift = 0.5 * rn(1, 1, C, 1, 1)
    y = 2.0 * rn(T, B, C, H, W) + shift
    gamma = 1.0 + 0.3 * rn(C)
    if cs.special_gamma and C >= 2:
        gamma[0], gamma[1] = 0.0, -0.7
    bias = 0.2 * rn(C)
    rm, rv = 0.3 * rn(C), 0.5 + torch.rand(C, generator=g)
    if cs.bn in ("eval", "eval_grad"):
        rm = rm + shift.flatten()
        rv = rv * 4.0
    v0 = i0 = None
    if cs.state:
        v0 = torch.tensor(0.3) if cs.v0_scalar else 0.5 * rn(B, C, H, W)
        i0 = rn(B, C, H, W)
    if cs.neuron == R.SYNAPSE:
        v0 = None
    addend = rn(T, B, C, H, W) if cs.addend else None
    g_out = rn(B, C, H, W) if cs.last_only else rn(T, B, C, H, W)
    g_out = g_out + 0.3   # a non-zero mean: a block dropped from the BatchNorm sums moves every dy of its channel
    g_vT = rn(B, C, H, W) if cs.state else None
    g_iT = rn(B, C, H, W) if cs.state and cs.neuron != R.SYNAPSE else None
    return Inputs(y, gamma, bias, rm, rv, v0, i0, addend, g_out, g_vT, g_iT)


def _cl(t, dev="cuda"):
    """Dense channels-last device copy of a logical [..., C, H, W] tensor."""
    nd = t.dim()
    perm = list(range(nd - 3)) + [nd - 2, nd - 1, nd - 3]
    inv = list(range(nd - 3)) + [nd - 1, nd - 3, nd - 2]
    return t.permute(perm).contiguous().to(dev).permute(inv)


# ------------------------------------------------------------------------------------------------------ device run
class DevResult(NamedTuple):
    out: torch.Tensor
    z: Optional[torch.Tensor]
    vT: Optional[torch.Tensor]
    iT: Optional[torch.Tensor]
    rm: Optional[torch.Tensor]
    rv: Optional[torch.Tensor]
    grads: dict
    guard_ok: bool


def batch_share(cs, inp, batch):
    """The row and its inputs restricted to the samples ``batch`` (a slice over B): one rank's share of the batch."""
    s0 = lambda t: None if t is None else t[batch]        # noqa: E731
    s1 = lambda t: None if t is None else t[:, batch]     # noqa: E731
    share = inp._replace(y=s1(inp.y), v0=inp.v0 if cs.v0_scalar else s0(inp.v0), i0=s0(inp.i0), addend=s1(inp.addend),
                         g_out=s0(inp.g_out) if cs.last_only else s1(inp.g_out), g_vT=s0(inp.g_vT), g_iT=s0(inp.g_iT))
    return cs._replace(B=len(range(*batch.indices(cs.B)))), share


def run_device(HF, cs, inp, variant, sync_group=None, batch=None):
    """``sync_group``: the layer is a SyncBatchNorm one over that process group; ``batch``: this rank's samples."""
    from snn_for_object_detection_amd import _hip
    from snn_for_object_detection_amd.layer_gen import HipBatchNorm2d
    with HF.levers(USE_SUMS_FROM_STATE=variant != "no_yfree", LIF_CHECKPOINT_BYTES=0 if variant == "ckpt" else None,
                   SCAN_FLAGS=_hip.SCAN_WIDE_ADDRESSING if variant == "wide" else 0):
        if batch is not None:
            cs, inp = batch_share(cs, inp, batch)
        T, B, C, H, W = cs.T, cs.B, cs.C, cs.H, cs.W
        bn = None
        if cs.bn is not None:
            bn = HipBatchNorm2d(C).cuda()
            with torch.no_grad():
                bn.weight.copy_(inp.gamma)
                bn.bias.copy_(inp.bias)
                bn.running_mean.copy_(inp.rm)
                bn.running_var.copy_(inp.rv)
            bn.train(cs.bn == "train")
            bn.weight.requires_grad_(cs.bn != "eval")
            bn.bias.requires_grad_(cs.bn != "eval")
            if sync_group is not None:
                bn._snn_sync_group = (sync_group,)
        if cs.y_off is None:
            y = _cl(inp.y)
        else:
            buf = torch.randn(T, B, H, W, C + 8, device="cuda")
            buf[..., cs.y_off:cs.y_off + C] = inp.y.permute(0, 1, 3, 4, 2).cuda()
            y = buf.permute(0, 1, 4, 2, 3)[:, :, cs.y_off:cs.y_off + C]
        y.requires_grad_()
        wrt = [y]
        if bn is not None and cs.bn != "eval":
            wrt += [bn.weight, bn.bias]
        state = None
        v0 = i0 = None
        if cs.state:
            if cs.neuron == R.SYNAPSE:
                raise AssertionError("no carried-state Synapse rows")
            v0 = inp.v0.cuda().requires_grad_() if cs.v0_scalar else _cl(inp.v0).requires_grad_()
            i0 = _cl(inp.i0).requires_grad_()
            state = HF.NeuronState(v0, i0)
            wrt += [v0, i0]
        addend = None
        if cs.addend:
            addend = _cl(inp.addend).requires_grad_()
            wrt.append(addend)
        dest = promise = None
        if cs.dest:
            promise = HF.ConcatPromise(C + 8)
            promise.buf = HF._new_cl((T, B), C + 8, H, W, y).fill_(float("nan"))
            dest = HF.Dest(promise, 4, C)
        prm = HF.neuron_params()
        prm.sigma = cs.sigma
        out, st = HF.affine_neuron(y, cs.neuron, state, bn=bn, params=prm, dest=dest, addend=addend,
                                   last_only=cs.last_only, spikes_ok=cs.spikes_ok)
        z = None
        if cs.neuron == R.LIF:
            thr = getattr(out, "_snn_spike_threshold", None)
            if cs.spikes_ok:
                assert thr is not None, "spikes_ok: the layer wrote a spike tensor"
                z = (out.detach() > thr).to(D)
            elif cs.addend:
                z = ((out.detach() - addend.detach()) > 0.5).to(D)   # out = z + addend, |addend| << 2^22
            else:
                z = out.detach().to(D)
                assert bool(((z == 0) | (z == 1)).all())
        outs, gouts = [out], [_cl(inp.g_out)]
        if cs.state:
            outs.append(st.v)
            gouts.append(_cl(inp.g_vT))
            if cs.neuron != R.SYNAPSE:
                outs.append(st.i)
                gouts.append(_cl(inp.g_iT))
        gr = torch.autograd.grad(outs, wrt, gouts, allow_unused=True)
        names = ["dy"] + (["dgamma", "dbias"] if (bn is not None and cs.bn != "eval") else []) + \
                (["dv0", "di0"] if cs.state else []) + (["daddend"] if cs.addend else [])
        torch.cuda.synchronize()
        grads = {k: (None if v is None else v.detach().to(D)) for k, v in zip(names, gr)}
        guard_ok = True
        if cs.dest:
            gb = promise.buf.detach().permute(0, 1, 3, 4, 2)
            bits = torch.cat([gb[..., :4], gb[..., 4 + C:]], -1).contiguous().view(torch.int32)
            guard_ok = bool((bits == NAN_BITS).all())
        res = DevResult(out.detach().to(D) if not cs.spikes_ok else z, z,
                        None if st is None else st[0].detach().to(D),
                        None if (st is None or cs.neuron == R.SYNAPSE) else st.i.detach().to(D),
                        None if bn is None else bn.running_mean.detach().to(D),
                        None if bn is None else bn.running_var.detach().to(D), grads, guard_ok)
        return res


# ------------------------------------------------------------------------------------------------------ reference
class RefResult(NamedTuple):
    out: torch.Tensor
    vdec: Optional[torch.Tensor]
    vT: Optional[torch.Tensor]
    iT: Optional[torch.Tensor]
    rm: Optional[torch.Tensor]
    rv: Optional[torch.Tensor]
    grads: dict
    gx: torch.Tensor               # gradient at the neuron input x
    bn: Optional[R.BnStats]
    gamma: Optional[torch.Tensor]
    excluded: Optional[torch.Tensor]   # [B, C, H, W] lanes kept out of the elementwise bounds


def run_ref(cs, inp, z_kernel, dev, alpha=R.ALPHA, unbiased_running=True):
    from snn_for_object_detection_amd import functional as HF
    prm = HF.neuron_params()
    y = inp.y.to(dev, D).requires_grad_()
    wrt = [y]
    gamma = bias = None
    st = None
    if cs.bn is not None:
        gamma = inp.gamma.to(dev, D).requires_grad_(cs.bn != "eval")
        bias = inp.bias.to(dev, D).requires_grad_(cs.bn != "eval")
        if cs.bn != "eval":
            wrt += [gamma, bias]
        x, st = R.batch_norm(y, gamma, bias, cs.bn == "train", 1e-5, 0.1, inp.rm.to(dev, D), inp.rv.to(dev, D),
                             unbiased_running)
    else:
        x = y * 1.0
    v0 = i0 = None
    if cs.state:
        v0 = inp.v0.to(dev, D).requires_grad_()
        i0 = inp.i0.to(dev, D).requires_grad_()
        wrt += [v0, i0]
    x_scale = None
    if cs.neuron == R.SYNAPSE:
        if st is not None:
            a = (gamma * st.invstd).detach()
            b = (bias[None, :] - st.mean * a).detach()
            x_scale = (y.detach() * a[:, None, :, None, None]).abs() + b[:, None, :, None, None].abs()
        else:
            x_scale = y.detach().abs()
    r = R.neuron_scan(x, cs.neuron, v0, i0, None if z_kernel is None else z_kernel.to(dev), alpha, cs.sigma,
                      float(prm.dt), x_scale, cs.last_only)
    out = r.out
    addend = None
    if cs.addend:
        addend = inp.addend.to(dev, D).requires_grad_()
        wrt.append(addend)
        out = out + addend
    outs, gouts = [out], [inp.g_out.to(dev, D)]
    if cs.state:
        outs.append(r.vT)
        gouts.append(inp.g_vT.to(dev, D))
        if cs.neuron != R.SYNAPSE:
            outs.append(r.iT)
            gouts.append(inp.g_iT.to(dev, D))
    gr = torch.autograd.grad(outs, wrt + [x], gouts, allow_unused=True)
    names = ["dy"] + (["dgamma", "dbias"] if (cs.bn is not None and cs.bn != "eval") else []) + \
            (["dv0", "di0"] if cs.state else []) + (["daddend"] if cs.addend else [])
    grads = {k: (None if v is None else v.detach()) for k, v in zip(names, gr[:-1])}
    gx = gr[-1] if gr[-1] is not None else torch.zeros_like(x)
    bn_st = None
    if st is not None:
        bn_st = R.BnStats(st.mean.detach(), st.var.detach(), st.xhat.detach(), st.invstd.detach(), st.running_mean,
                          st.running_var)
    return RefResult(out.detach(), r.vdec, None if r.vT is None else r.vT.detach(),
                     None if r.iT is None else r.iT.detach(),
                     None if st is None else (st.running_mean if cs.bn == "train" else inp.rm.to(dev, D)),
                     None if st is None else (st.running_var if cs.bn == "train" else inp.rv.to(dev, D)),
                     grads, gx.detach(), bn_st, None if gamma is None else gamma.detach(), r.near_zero)


# ------------------------------------------------------------------------------------------------------ checks
def _elementwise(name, d, r, keep, fails, rec):
    err = (d - r).abs()
    bound = FWD_REL * (1.0 + r.abs())
    if keep is not None:
        err = torch.where(keep, err, torch.zeros_like(err))
    ratio = float((err / bound).max())
    rec[name] = ratio
    if not ratio <= 1.0:
        fails.append(f"{name}: max |d - r| / (1e-5 (1 + |r|)) = {ratio:.3g}")


def _groupwise(name, d, r, scale, tol, dims_list, fails, rec):
    """||d - r|| <= tol * ||scale|| over every group; dims_list: the dims reduced for each grouping."""
    worst = 0.0
    for dims, label in dims_list:
        e = (d - r).square().sum(dim=dims).sqrt()
        s = scale.square().sum(dim=dims).sqrt()
        ratio = float((e / (tol * s + 1e-300)).max())
        worst = max(worst, ratio)
        if not ratio <= 1.0:
            fails.append(f"{name} per {label}: max ||d - r|| / ({tol:g} ||s||) = {ratio:.3g}")
    rec[name] = worst


def _quad_groups(t):
    """[T, B, C, H, W] -> [T, B, C/4 groups, 4, H, W] view, channels padded to a multiple of 4."""
    T, B, C, H, W = t.shape
    pad = (-C) % 4
    if pad:
        t = torch.cat([t, torch.zeros(T, B, pad, H, W, dtype=t.dtype, device=t.device)], 2)
    return t.reshape(T, B, (C + pad) // 4, 4, H, W)


def check_forward(cs, dev_res, ref, fails, rec):
    keep = None
    if ref.excluded is not None:
        keep = (~ref.excluded).to(dev_res.out.device)
        rec["excluded_lanes"] = int(ref.excluded.sum())
    if cs.neuron == R.LIF:
        z = dev_res.z
        vd = ref.vdec.to(z.device)
        mism = z != (vd > R.V_TH).to(D)
        near = (vd - R.V_TH).abs() <= 1e-5
        rec["spike_flips"] = int(mism.sum())
        if bool((mism & ~near).any()):
            fails.append(f"spikes: {int((mism & ~near).sum())} decisions differ away from the threshold")
        if mism.float().mean().item() > 1e-4:
            fails.append(f"spikes: {mism.float().mean().item():.3g} of the decisions flipped")
    else:
        out_keep = None if keep is None else (keep if cs.last_only else keep.expand_as(ref.out))
        _elementwise("out", dev_res.out, ref.out.to(dev_res.out.device), out_keep, fails, rec)
    if ref.vT is not None and dev_res.vT is not None:
        _elementwise("vT", dev_res.vT, ref.vT.to(dev_res.vT.device), keep, fails, rec)
    if ref.iT is not None and dev_res.iT is not None:
        _elementwise("iT", dev_res.iT, ref.iT.to(dev_res.iT.device), keep, fails, rec)
    if ref.rm is not None:
        # running statistics: variance in double from fp32 y, T fp32 updates of relative 2^-24 each: << 1e-5
        _elementwise("running_mean", dev_res.rm, ref.rm.to(dev_res.rm.device), None, fails, rec)
        _elementwise("running_var", dev_res.rv, ref.rv.to(dev_res.rv.device), None, fails, rec)
    if not dev_res.guard_ok:
        fails.append("dest: a guard channel of the concat buffer changed")


def check_grads(cs, dev_res, ref, fails, rec, grads=None):
    g_ref = ref.grads if grads is None else grads
    tol = _tol(cs.neuron)
    dv = dev_res.grads["dy"].device
    gx = ref.gx.to(dv)
    keep = None if ref.excluded is None else (~ref.excluded).to(dv).to(D)
    # magnitude of the terms that form dy
    if cs.bn == "train":
        xh, inv = ref.bn.xhat.to(dv), ref.bn.invstd.to(dv)
        ag = ref.gamma.to(dv).abs()[None, :] * inv
        m1 = gx.abs().mean(dim=(1, 3, 4))
        m2 = (gx * xh).abs().mean(dim=(1, 3, 4))
        e = lambda a: a[:, None, :, None, None]   # noqa: E731
        s_dy = e(ag) * (gx.abs() + e(m1) + xh.abs() * e(m2))
    elif cs.bn in ("eval", "eval_grad"):
        inv = ref.bn.invstd.to(dv)
        s_dy = (ref.gamma.to(dv).abs()[None, :] * inv)[:, None, :, None, None] * gx.abs()
    else:
        s_dy = gx.abs()
    d_dy, r_dy = dev_res.grads["dy"], g_ref["dy"].to(dv)
    if keep is not None:
        d_dy, r_dy = d_dy * keep, r_dy * keep
    _groupwise("dy", _quad_groups(d_dy), _quad_groups(r_dy), _quad_groups(s_dy), tol,
               [((1, 2, 3, 4, 5), "timestep"), ((0, 1, 3, 4, 5), "4-channel group")], fails, rec)
    if "dgamma" in g_ref:
        xh = ref.bn.xhat.to(dv)
        for name, terms in (("dgamma", gx * xh), ("dbias", gx)):
            s = terms.abs().sum(dim=(0, 1, 3, 4))
            if keep is not None:   # an excluded lane may differ by its whole contribution
                s = s + 2.0 * (terms.abs() * (1.0 - keep)).sum(dim=(0, 1, 3, 4))
            err = (dev_res.grads[name] - g_ref[name].to(dv)).abs()
            ratio = float((err / (tol * s + 1e-300)).max())
            rec[name] = ratio
            if not ratio <= 1.0:
                c = int((err / (tol * s + 1e-300)).argmax())
                fails.append(f"{name}: max |d - r| / ({tol:g} sum|terms|) = {ratio:.3g} at channel {c}")
    for name in ("dv0", "di0"):
        if name in g_ref and g_ref[name] is not None:
            r = g_ref[name].to(dv)
            d = dev_res.grads[name]
            e = float((d - r).norm() / (tol * r.norm() + 1e-300))
            rec[name] = e
            if not e <= 1.0:
                fails.append(f"{name}: ||d - r|| / ({tol:g} ||r||) = {e:.3g}")
    if "daddend" in g_ref:
        if not torch.equal(dev_res.grads["daddend"], g_ref["daddend"].to(dv)):
            fails.append("daddend: the shortcut's gradient is not g_out")


def _record(cs, variant, rec):
    _RECORD[f"{cs.id}/{variant}"] = rec
    path = os.environ.get("SNN_FP64_RECORD")
    if path:
        rows = {}
        if os.path.exists(path):   # (another test module's rows: tests/test_gpu_syncbn_fp64.py records through here too)
            with open(path) as f:
                rows = json.load(f)
        rows.update(_RECORD)
        with open(path, "w") as f:
            json.dump(rows, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("cs", CASES, ids=[c.id for c in CASES])
def test_norm_neuron_against_fp64(HF, cs):
    pl = plan_of(HF, cs)
    got = plan_classes(pl)
    assert set(cs.classes) <= got, (cs.id, pl, got)
    inp = make_inputs(cs, seed=zlib.crc32(cs.id.encode()) % 10007)
    dev = "cuda" if _is_prod(cs) else "cpu"
    ref = None
    z0 = None
    for variant in cs.variants:
        if variant == "wide":
            assert plan_of(HF, cs, "wide").buf == 0
        res = run_device(HF, cs, inp, variant)
        if ref is None:
            z0 = res.z
            ref = run_ref(cs, inp, None if z0 is None else z0, dev)
        elif z0 is not None:
            assert torch.equal(res.z, z0), f"{variant}: the spikes differ from the first variant's"
        fails, rec = [], {"plan": list(pl)}
        check_forward(cs, res, ref, fails, rec)
        check_grads(cs, res, ref, fails, rec)
        _record(cs, variant, rec)
        assert not fails, f"{cs.id} [{variant}]:\n  " + "\n  ".join(fails)
    del ref
    torch.cuda.empty_cache()


def test_every_plan_class_is_reached(HF):
    """Every reverse-scan plan class the table is for is reached on this device's CU count."""
    seen = set()
    for cs in CASES:
        got = plan_classes(plan_of(HF, cs))
        assert set(cs.classes) <= got, (cs.id, got)
        seen |= got
    assert REQUIRED_CLASSES <= seen, REQUIRED_CLASSES - seen


# ------------------------------------------------------------------------------------------------------ negative controls
# Each check family must fail against a deliberately wrong reference.
def _small_case(cs_id):
    return next(c for c in CASES if c.id == cs_id)


@pytest.mark.parametrize("cs_id, families", [("lif_c512_gy", ("dy per", "dgamma", "dbias")),
                                              ("lif_rpb_gt1", ("dgamma", "dbias"))])
def test_control_bn_sums_without_the_last_block(HF, cs_id, families):
    """dy / dgamma / dbias from BatchNorm sums that omit the pixel rows of the last block: must fail.  (On the 282-block
    row one block of 2 x 64 pixels moves dy by ~1e-5 of its terms: the per-channel parameter gradients see it.)"""
    cs = _small_case(cs_id)
    pl = plan_of(HF, cs)
    assert pl.gx > 1
    inp = make_inputs(cs, seed=zlib.crc32(cs.id.encode()) % 10007)
    res = run_device(HF, cs, inp, "default")
    ref = run_ref(cs, inp, res.z, "cpu")
    M = cs.B * cs.H * cs.W
    first_dropped = (pl.gx - 1) * pl.rpb * (256 // pl.cvb)
    keep = (torch.arange(M) < first_dropped).reshape(cs.B, cs.H, cs.W)
    dy, s1, s2 = R.bn_train_dy(ref.gx, ref.bn.xhat, ref.bn.invstd, ref.gamma, M, keep)
    # the closed form with every pixel agrees with autograd: the control differs from the reference only by the block
    dy_all, _, _ = R.bn_train_dy(ref.gx, ref.bn.xhat, ref.bn.invstd, ref.gamma, M)
    assert float((dy_all - ref.grads["dy"]).norm() / ref.grads["dy"].norm()) < 1e-12
    wrong = dict(ref.grads, dy=dy, dgamma=s2.sum(0), dbias=s1.sum(0))
    fails = []
    check_grads(cs, res, ref, fails, {}, grads=wrong)
    for fam in families:
        assert any(f.startswith(fam) for f in fails), (fam, fails)


def test_control_superspike_alpha_99(HF):
    """The LIF gradients of a reference whose SuperSpike has alpha = 99: must fail."""
    cs = _small_case("lif_c8_cvb2_state")
    inp = make_inputs(cs, seed=zlib.crc32(cs.id.encode()) % 10007)
    res = run_device(HF, cs, inp, "default")
    ref = run_ref(cs, inp, res.z, "cpu", alpha=99.0)
    fails = []
    check_grads(cs, res, ref, fails, {})
    assert any(f.startswith(("dy per", "dv0", "di0")) for f in fails), fails


def test_control_biased_running_variance(HF):
    """Running statistics of a reference that updates with the biased variance: must fail."""
    cs = _small_case("lif_c4_cvb1")
    inp = make_inputs(cs, seed=zlib.crc32(cs.id.encode()) % 10007)
    res = run_device(HF, cs, inp, "default")
    ref = run_ref(cs, inp, res.z, "cpu", unbiased_running=False)
    fails = []
    check_forward(cs, res, ref, fails, {})
    assert any(f.startswith("running_var") for f in fails) and not any(f.startswith("running_mean") for f in fails), fails
