"""The implicit-GEMM convolutions, one row per plan class, against fp64 per element.

k_conv_gather (forward / data gradient; csrc/conv_gather.hip), k_conv_wgrad_pipe / k_conv_wgrad (weight gradient) and the
slab reducers (k_wgrad_reduce, k_wgrad_reduce_once, k_wgrad_reduce4) of csrc/conv_wgrad.hip through the C ABI.  Every row
* names the plan classes it exists for and asserts them through the host-only queries snn_conv2d_gather_plan /
  snn_conv2d_wgrad_plan with this device's CU count (it is in the row's messages) and the alignment facts of the very
  buffers it passes; test_every_gemm_plan_class_is_reached fails when the tables no longer cover REQUIRED_CLASSES;
* writes into a NaN-filled slice of a wider buffer whose guard channels and guard pixels must come back bit for bit
  (weight gradient: dw inside a guarded flat buffer, the workspace NaN-filled and exactly splitk * n floats between guards);
* checks every element against torch's fp64 CPU convolution, |out - ref| <= (PREC_TOL + ACC_TOL) * mag (tests/conv_ref.py),
  and that the bound rejects a reference with one channel, one tap or one split's pixels dropped (_teeth);
* runs again on EXACT operands - x, dy small integers, w = k * 2^-6 with |k| <= 31 - where every product and partial sum is
  exact in every arithmetic mode: outputs, BatchNorm partials and reduced weight gradients must equal fp64 bit for bit, for
  accumulate = 0 and 1.
Each row prints its largest error / bound ratio (RATIO lines, -s) and, when SNN_FP64_RECORD names a file, writes the
ratios of the run there as JSON.  Spike-operand and bf16-storage numerics stay in test_gpu_siblings.py / test_gpu_bf16_storage.py.
"""
import ctypes
import json
import os

import pytest
import torch

from tests.conv_ref import ACC_TOL, PREC_TOL, TINY, _check, _dgrad_ref, _fwd_ref, _teeth, _wgrad_ref
from tests.fp64_buffers import GATHER_KEYS, GUARD, SENT, WGRAD_PLAN_KEYS, Buf, _exact_operands, _exact_weights, _random, _st

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H_(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from snn_for_object_detection_amd import _hip
    return _hip


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _prec(_hip, name):
    return {"fp32": _hip.PREC_FP32, "bf16x3": _hip.PREC_BF16X3, "bf16x6": _hip.PREC_BF16X6, "fp16x3": _hip.PREC_FP16X3,
            "bf16x1": _hip.PREC_BF16X1}[name]


_RECORD = {}


def _ratio(tag, out, ref, mag, tol, **extra):
    r = float(((out - ref).abs() / (tol * mag + TINY)).max())
    print(f"RATIO {tag} {r:.4g}" + "".join(f" {k}={v}" for k, v in extra.items()))
    _RECORD[tag] = dict(ratio=r, num_cu=_num_cu(), **extra)
    if os.environ.get("SNN_FP64_RECORD"):
        with open(os.environ["SNN_FP64_RECORD"], "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)
    return r


def _a16(ptr):
    return ptr % 16 == 0


def _gather_align(x, w, y, adds, split):
    """align_bits of snn_conv2d_gather_plan from the pointers and strides the call gets (include/snn_hip.h)."""
    b = (1 if _a16(x.ptr) else 0) | (2 if x.ptr % 8 == 0 else 0) | (4 if _a16(w.data_ptr()) else 0)
    b |= (8 if _a16(y.ptr) else 0) | (16 if y.ptr % 8 == 0 else 0)
    for i, (ptr, ld) in enumerate(adds):
        b |= (32 << (2 * i) if _a16(ptr) and ld % 4 == 0 else 0) | (64 << (2 * i) if ptr % 8 == 0 and ld % 4 == 0 else 0)
    return b | (512 if split is not None and _a16(split.data_ptr()) else 0)


# ---------------------------------------------------------------------------------------------------- k_conv_gather
# id, kind, N, H, W, Cin, Cout, KH, KW, stride, pad, arithmetic modes, options, plan classes the row exists for.
# options: x = (channel offset, pixel stride) of the gathered tensor, y = the same of the produced one, w_off = float offset
# of the weight matrix (1: not 16-byte aligned), adds = number of addends, inplace = the destination is its own addend,
# split = also with the pre-split weight image (bit-identical), fps = frames per timestep of the BatchNorm partials
FWD_MODES = ("fp16x3", "bf16x6", "fp32", "bf16x1")
BWD_MODES = ("bf16x3", "fp32", "bf16x1")
GATHER_ROWS = [
    ("fwd-scalar-co27-small", "fwd", 1, 5, 7, 3, 27, 3, 3, 1, 1, FWD_MODES, dict(),
     {"loader0", "bn32", "co%4", "M<128", "out_scalar", "idle"}),
    ("fwd-scalar-unaligned-w", "fwd", 2, 6, 8, 32, 32, 1, 1, 1, 0, ("fp16x3",), dict(w_off=1, adds=1),
     {"loader0", "bn32", "out_vec"}),
    ("fwd-vec-7x7-co36", "fwd", 2, 9, 11, 32, 36, 7, 7, 1, 3, FWD_MODES, dict(y=(4, 44)),
     {"loader1", "bn64", "7x7", "out_vec"}),
    ("fwd-vec-co130-cin12", "fwd", 2, 8, 9, 12, 130, 3, 3, 1, 1, ("fp16x3", "fp32"), dict(adds=1),
     {"loader1", "bn128", "co%4", "ntiles_partial", "out_scalar"}),
    ("fwd-fast-1x1-co132-M768", "fwd", 3, 16, 16, 64, 132, 1, 1, 1, 0, FWD_MODES, dict(split=True),
     {"loader2", "loader3", "bn128", "ntiles_partial", "M%128", "idle", "1x1", "out_vec"}),
    ("fwd-fast-s2-co256-bn", "fwd", 6, 37, 45, 32, 256, 3, 3, 2, 1, ("fp16x3", "bf16x1"), dict(split=True, fps=2),
     {"loader2", "loader3", "bn128", "ntiles_full", "mtiles_per_xcd>1", "3x3s2", "bn_straddle"}),
    ("fwd-fast-5x3-co64", "fwd", 2, 10, 12, 32, 64, 5, 3, 1, 1, ("fp16x3", "bf16x6"), dict(x=(4, 40)),
     {"loader2", "bn64", "nonsquare"}),
    ("fwd-fast-5x5-co38", "fwd", 2, 9, 9, 32, 38, 5, 5, 1, 2, ("fp16x3",), dict(adds=1),
     {"loader2", "bn64", "5x5", "co%4"}),
    ("fwd-bn-multiple-T3", "fwd", 6, 8, 16, 32, 64, 1, 1, 1, 0, ("fp16x3",), dict(fps=2), {"bn_multiple"}),
    ("fwd-bn-T1", "fwd", 3, 8, 15, 32, 32, 1, 1, 1, 0, ("fp16x3",), dict(fps=3), {"bn_T1"}),
    ("fwd-bn-short-step", "fwd", 3, 5, 7, 32, 32, 1, 1, 1, 0, ("fp16x3",), dict(fps=1), {"bn_none"}),
    ("dgrad-s2-3x3-odd", "dgrad", 2, 13, 17, 64, 32, 3, 3, 2, 1, BWD_MODES, dict(adds=2, split=True),
     {"loader2", "loader3", "bn64", "phases4", "adds2"}),
    ("dgrad-1x1-s2-pad0", "dgrad", 2, 7, 9, 38, 64, 1, 1, 2, 0, BWD_MODES, dict(adds=2),
     {"phase_without_tap", "bn64", "co%4", "adds2"}),
    ("dgrad-1x1-s2-pad0-plain", "dgrad", 2, 7, 9, 32, 32, 1, 1, 2, 0, ("bf16x3",), dict(), {"phase_without_tap", "bn32"}),
    ("dgrad-s3-5x5-inplace", "dgrad", 2, 10, 11, 27, 12, 5, 5, 3, 2, BWD_MODES, dict(inplace=True),
     {"loader1", "phases9", "inplace", "co%4", "out_scalar"}),
    ("dgrad-stride-above-H", "dgrad", 3, 2, 9, 32, 32, 3, 3, 3, 1, ("bf16x3",), dict(adds=1), {"stride>H"}),
    ("dgrad-7x7-vec-co132", "dgrad", 1, 9, 10, 132, 32, 7, 7, 1, 3, ("bf16x3", "fp32"), dict(adds=1),
     {"loader1", "7x7", "bn128", "ntiles_partial"}),
]


def gather_plan(_hip, mode, N, H, W, Cin, Cout, KH, KW, s, pad, ld_in, ld_out, align, split, add, add2, fps, prec, phase=0):
    Ho, Wo = (H + 2 * pad - KH) // s + 1, (W + 2 * pad - KW) // s + 1
    out = (ctypes.c_int * 17)()
    rc = _hip.query("snn_conv2d_gather_plan", mode, N, H, W, Cin, Ho, Wo, Cout, KH, KW, s, pad, ld_in, ld_out, align, split, add,
                    add2, fps, prec, phase, ctypes.addressof(out))
    assert rc == 0, "snn_conv2d_gather_plan refuses the row"
    return dict(zip(GATHER_KEYS, out))


def _gather_classes(plans, kind, KH, KW, s, H, opt, M):
    """The plan classes a call shows (plans: one per launch)."""
    c = set()
    for p in plans:
        c |= {f"loader{p['loader']}", f"bn{p['bn']}", "out_vec" if p["out_vec"] else "out_scalar"}
        if p["idle"]:
            c.add("idle")
        if p["mtiles_per_xcd"] > 1:
            c.add("mtiles_per_xcd>1")
        if p["ktot"] == 0:
            c.add("phase_without_tap")
    p = plans[0]
    oc = p["_oc"]
    if oc % 4:
        c.add("co%4")
    if p["ntiles"] > 1:
        c.add("ntiles_full" if oc % p["bn"] == 0 else "ntiles_partial")
    if kind == "fwd":
        c.add("M<128" if M < 128 else "M%128" if M % 128 == 0 else "M_partial")
        if p["bn_chunks"]:
            rows, T = opt["fps"] * p["ohc"] * p["owc"], M // (opt["fps"] * p["ohc"] * p["owc"])
            c.add("bn_T1" if T == 1 else "bn_multiple" if rows % 128 == 0 else "bn_straddle" if T >= 3 else "bn_T2")
        elif opt.get("fps"):
            c.add("bn_none")
    else:
        c.add(f"phases{len(plans)}")
        if s > H:
            c.add("stride>H")
        if opt.get("inplace"):
            c.add("inplace")
        if opt.get("adds") == 2:
            c.add("adds2")
    c.add({(1, 1): "1x1", (5, 5): "5x5", (7, 7): "7x7"}.get((KH, KW), "nonsquare" if KH != KW else "3x3s2" if s == 2 else "3x3"))
    return c


def _run_gather(_hip, kind, x, w, geom, prec, opt, *, split=False, adds=(), part_fill=None):
    """One snn_conv2d_fwd / snn_conv2d_dgrad call into guarded buffers.  x: the gathered tensor (dy for a data gradient);
    w [Cout,KH,KW,Cin].  Returns (out fp64 CPU, plans, per-(t, c) sums or None, partials buffer or None)."""
    N, H, W, Cin, Cout, KH, KW, s, pad = geom
    Ho, Wo = (H + 2 * pad - KH) // s + 1, (W + 2 * pad - KW) // s + 1
    x_off, x_ld = opt.get("x", (0, None))
    y_off, y_ld = opt.get("y", (0, None))
    X = Buf(x.shape, x_off, x_ld, values=x)
    oshape = (N, Ho, Wo, Cout) if kind == "fwd" else (N, H, W, Cin)
    wm = w if kind == "fwd" else w.permute(3, 1, 2, 0)                 # [Cin][KH][KW][Cout]: the transposed weights
    w_off = opt.get("w_off", 0)
    wbuf = torch.full((wm.numel() + 8,), SENT, device="cuda")
    wdev = wbuf[4 + w_off:4 + w_off + wm.numel()]
    wdev.copy_(wm.contiguous().reshape(-1))
    img = None
    if split:
        img = torch.empty(wm.numel(), device="cuda")
        _hip.call("snn_weight_presplit", wdev.data_ptr(), img.data_ptr(), wm.numel(),
                  _hip.PREC_FP16X3 if kind == "fwd" else _hip.PREC_BF16X3, _st())
    if opt.get("inplace"):
        Y = Buf(oshape, y_off, y_ld, values=adds[0])
        A, a_ptrs = [], [(Y.ptr, Y.ld)]
    else:
        Y = Buf(oshape, y_off, y_ld, fill=float("nan"))
        A = [Buf(oshape, 4 * i, oshape[3] + 8, values=a) for i, a in enumerate(adds)]
        a_ptrs = [(a.ptr, a.ld) for a in A]
    a_args = []
    for i in range(2):
        a_args += list(a_ptrs[i]) if i < len(a_ptrs) else [None, 0]
    align = _gather_align(X, wdev, Y, a_ptrs, img)
    fps = opt.get("fps", 0)
    mode = 0 if kind == "fwd" else 1
    q = (mode, N, H, W, Cin, Cout, KH, KW, s, pad, X.ld, Y.ld, align, int(split), int(len(a_ptrs) > 0), int(len(a_ptrs) > 1), fps, prec)
    plans = [gather_plan(_hip, *q)]
    plans += [gather_plan(_hip, *q, phase=ph) for ph in range(1, plans[0]["nphases"])]
    for p in plans:
        p["_oc"] = oshape[3]
    part = lay = sums = None
    if kind == "fwd":
        if fps:
            n_part = _hip.query("snn_conv2d_fwd_bn_partial_size", N, fps, Ho, Wo, Cout)
            part = torch.full((n_part,), part_fill if part_fill is not None else float("nan"), dtype=torch.float64, device="cuda")
            lay = (ctypes.c_int * 2)()
        _hip.call("snn_conv2d_fwd", X.ptr, X.ld, wdev.data_ptr(), img.data_ptr() if split else None, Y.ptr, Y.ld, N, H, W, Cin,
                  Ho, Wo, Cout, KH, KW, s, pad, a_args[0], a_args[1], part.data_ptr() if fps else None, fps, lay, prec, _st())
        if fps:
            assert (lay[0], lay[1]) == (plans[0]["bn_chunks"], plans[0]["bn_rows"]), (lay[0], lay[1], plans[0])
            if lay[0]:
                sums = torch.empty(N // fps, Cout, 2, dtype=torch.float64, device="cuda")
                _hip.call("snn_bn_stats_reduce", part.data_ptr(), lay[0], lay[1], N // fps, fps * Ho * Wo, Cout, sums.data_ptr(), _st())
    else:
        _hip.call("snn_conv2d_dgrad", X.ptr, X.ld, wdev.data_ptr(), img.data_ptr() if split else None, Y.ptr, Y.ld, N, H, W, Cin,
                  Ho, Wo, Cout, KH, KW, s, pad, *a_args, prec, _st())
    torch.cuda.synchronize()
    assert X.guards_intact(whole=True) and all(a.guards_intact(whole=True) for a in A), "an input changed"
    assert Y.guards_intact(), "the convolution wrote outside its output slice"
    wb = wbuf.cpu()
    assert bool((wb[:4 + w_off] == SENT).all()) and bool((wb[4 + w_off + wm.numel():] == SENT).all())
    return Y.value(), plans, (None if sums is None else sums.cpu()), part


@pytest.mark.parametrize("row", GATHER_ROWS, ids=[r[0] for r in GATHER_ROWS])
def test_gather_row_against_fp64(H_, row):
    _hip = H_
    rid, kind, N, H, W, Cin, Cout, KH, KW, s, pad, modes, opt, want_classes = row
    Ho, Wo = (H + 2 * pad - KH) // s + 1, (W + 2 * pad - KW) // s + 1
    geom = (N, H, W, Cin, Cout, KH, KW, s, pad)
    xshape = (N, H, W, Cin) if kind == "fwd" else (N, Ho, Wo, Cout)
    oshape = (N, Ho, Wo, Cout) if kind == "fwd" else (N, H, W, Cin)
    nadd = 1 if opt.get("inplace") else opt.get("adds", 0)
    seed = N * 1000 + H * 10 + W + Cin
    seen = set()
    for name in modes:
        prec = _prec(_hip, name)
        for exact in (False, True):
            if exact:
                x, w = _exact_operands(xshape, seed), _exact_weights((Cout, KH, KW, Cin), seed + 1)
                adds = [_exact_operands(oshape, seed + 2 + i, lim=8) for i in range(nadd)]
            else:
                x, w = _random(xshape, seed), _random((Cout, KH, KW, Cin), seed + 1, (KH * KW * Cin) ** -0.5)
                adds = [_random(oshape, seed + 2 + i) for i in range(nadd)]
            xd, wd = x.double(), w.double()
            if kind == "fwd":
                ref, mag = _fwd_ref(xd, wd, s, pad), _fwd_ref(xd.abs(), wd.abs(), s, pad)
            else:
                ref, mag = _dgrad_ref(xd, wd, H, W, s, pad), _dgrad_ref(xd.abs(), wd.abs(), H, W, s, pad)
            want = ref + sum(a.double() for a in adds) if adds else ref
            amag = sum(a.double().abs() for a in adds) if adds else None
            out, plans, sums, part = _run_gather(_hip, kind, x, w, geom, prec, opt, adds=adds, part_fill=12345.0)
            what = f"{rid} {name} {'exact' if exact else 'random'} ({_num_cu()} CUs) plans {plans}"
            seen |= _gather_classes(plans, kind, KH, KW, s, H, opt, N * Ho * Wo)
            if opt.get("split") and name in ("fp16x3", "bf16x3"):
                out2, plans2, sums2, _ = _run_gather(_hip, kind, x, w, geom, prec, opt, split=True, adds=adds)
                seen |= {f"loader{p['loader']}" for p in plans2}
                assert torch.equal(out2, out), f"{what}: the pre-split weight image changes bits"
                assert sums is None or torch.equal(sums2, sums), f"{what}: pre-split image, BatchNorm partials"
            if kind == "dgrad" and any(p["ktot"] == 0 for p in plans):
                dead = mag == 0                              # pixels no tap reaches: exactly (0 + addend) + addend2 in fp32
                a32 = torch.zeros(oshape)
                for a in adds:
                    a32 = a32 + a
                assert bool(dead.any()) and torch.equal(out[dead], a32.double()[dead]), f"{what}: tapless pixels are not the addends"
            if opt.get("fps"):
                if plans[0]["bn_chunks"] == 0:
                    assert bool((part == 12345.0).all()), f"{what}: bn_layout[0] == 0 but the partials buffer was written"
                else:
                    yt = (ref if exact else out).reshape(N // opt["fps"], -1, Cout)
                    ws = torch.stack([yt.sum(1), (yt * yt).sum(1)], -1)
                    if exact:
                        assert torch.equal(sums, ws), f"{what}: BatchNorm partials differ from the fp64 sums"
                    else:
                        scale = torch.stack([yt.abs().sum(1), (yt * yt).sum(1)], -1)
                        assert bool(((sums - ws).abs() <= 1e-12 * scale + 1e-30).all()), f"{what}: BatchNorm partials"
            if exact:
                assert torch.equal(out, want), f"{what}: {int((out != want).sum())} elements differ from fp64"
                continue
            _check(what, out, want, mag, name, extra_mag=amag)
            _ratio(f"k_conv_gather {kind} {name} {rid}", out, want, mag + (amag if adds else 0), PREC_TOL[name] + ACC_TOL)
            if name != "bf16x1":   # (one channel / tap of many is below the bf16 x 1 bound)
                c = x.shape[3] // 2                                      # one gathered channel dropped
                if kind == "fwd":
                    drop = _fwd_ref(xd[..., c:c + 1], wd[..., c:c + 1], s, pad)
                else:
                    drop = _dgrad_ref(xd[..., c:c + 1], wd[c:c + 1], H, W, s, pad)
                _teeth(what, out, want - drop, mag + (amag if adds else 0), name)
                wt = wd.clone()
                wt[:, KH - 1, KW - 1] = 0                                # the last tap dropped
                wrong = _fwd_ref(xd, wt, s, pad) if kind == "fwd" else _dgrad_ref(xd, wt, H, W, s, pad)
                _teeth(what, out, wrong + (want - ref), mag + (amag if adds else 0), name)
                if kind == "dgrad" and len(plans) > 1:                   # one stride phase's launch skipped: only the addends
                    ph = next(i for i, p in enumerate(plans) if p["ktot"] > 0)
                    npw = min(s, W)
                    wrong = want.clone()
                    wrong[:, ph // npw::s, ph % npw::s] = (want - ref)[:, ph // npw::s, ph % npw::s]
                    _teeth(what, out, wrong, mag + (amag if adds else 0), name)
    assert want_classes <= seen, f"{rid} ({_num_cu()} CUs): the row no longer reaches {want_classes - seen}; it shows {seen}"


# ---------------------------------------------------------------------------------------------------- weight gradient
# id, N, H, W, Cin, Cout, k, stride, arithmetic modes, options, plan classes the row exists for (asserted at this device's
# CU count; the shapes are the smallest a host-side search over snn_conv2d_wgrad_plan found for 256 CUs).
# options: dw_off = float offsets of dw inside the flat buffer to run (1..3: the scalar reducer), x = (offset, stride).
WGRAD_ROWS = [
    ("tile0-128x128", 1, 5, 7, 68, 68, 1, 2, BWD_MODES, dict(), {"tile0", "stage32", "splitk1", "kernel0", "kernel1"}),
    ("tile1-64x256-5x5", 1, 5, 7, 20, 36, 5, 1, BWD_MODES, dict(), {"tile1", "stage32", "splitk1"}),
    ("tile2-32x256", 1, 5, 7, 132, 4, 1, 2, ("bf16x3", "fp32"), dict(), {"tile2", "stage32"}),
    ("tile3-128x64", 1, 5, 7, 4, 68, 1, 2, ("bf16x3", "fp32"), dict(), {"tile3", "stage32"}),
    ("tile4-64x64", 1, 5, 7, 4, 4, 1, 2, ("bf16x3", "fp32"), dict(), {"tile4", "stage64"}),
    ("tile5-32x128", 1, 5, 7, 68, 4, 1, 2, BWD_MODES, dict(), {"tile5", "stage64"}),
    ("scalar-odd-channels", 2, 9, 11, 3, 27, 3, 1, ("bf16x3", "fp32"), dict(), {"kernel2"}),
    ("scalar-unaligned-x", 2, 9, 11, 32, 36, 1, 1, ("bf16x3",), dict(x=(1, 36)), {"kernel2"}),
    # the 32-pixel-stage tiles with several splits of several stages and a short last split (the steady-state loop)
    ("tile0-splitk3", 2, 30, 38, 20, 68, 3, 2, BWD_MODES, dict(), {"tile0:multisplit", "stage32", "splitk2-7", "tiles>1"}),
    ("tile1-splitk9-5x5", 2, 30, 38, 20, 36, 5, 1, BWD_MODES, dict(),
     {"tile1:multisplit", "stage32", "splitk8-31!%8", "tiles>1", "tails:once2"}),
    ("tile1-splitk32-empty", 3, 45, 61, 256, 36, 1, 1, ("bf16x3",), dict(), {"tile1:multisplit", "stage32", "splitk>=32", "empty"}),
    ("tile1-gen1-256-36-8x10", 160, 8, 10, 256, 36, 1, 1, ("bf16x3",), dict(), {"tile1:multisplit", "stage32", "splitk>=32", "empty"}),
    ("tile2-splitk3-3x3s2", 2, 30, 38, 100, 4, 3, 2, BWD_MODES, dict(), {"tile2:multisplit", "stage32", "splitk2-7", "tiles>1"}),
    ("tile2-splitk32-empty", 3, 45, 61, 132, 4, 1, 1, ("bf16x3",), dict(), {"tile2:multisplit", "stage32", "splitk>=32", "empty"}),
    ("tile3-splitk9", 2, 30, 38, 4, 68, 1, 1, BWD_MODES, dict(), {"tile3:multisplit", "stage32", "splitk8-31!%8", "tails:once2"}),
    ("tile3-splitk32-empty", 3, 45, 61, 4, 68, 1, 1, ("bf16x3",), dict(), {"tile3:multisplit", "stage32", "splitk>=32", "empty"}),
    ("splitk3-once1", 2, 30, 38, 4, 132, 1, 2, BWD_MODES, dict(dw_off=(0, 1)), {"splitk2-7", "once1", "scalar1", "tiles>1"}),
    ("splitk9-once2-tails", 3, 45, 61, 4, 132, 1, 2, BWD_MODES, dict(dw_off=(0, 2)),
     {"splitk8-31!%8", "once2", "scalar4", "tails:once2", "tiles>1"}),
    ("splitk8-3x3s2-empty", 3, 45, 61, 260, 132, 3, 2, ("bf16x3",), dict(), {"splitk8-31%8", "once2", "empty", "tiles>1", "row_split"}),
    ("splitk18-once4-tails", 4, 30, 38, 4, 4, 1, 1, ("bf16x3", "fp32"), dict(dw_off=(0, 3)), {"once4", "tails:once4", "scalar4"}),
    ("splitk32-once8-empty", 3, 45, 61, 4, 132, 1, 1, ("bf16x3",), dict(), {"splitk>=32", "once8", "empty", "tiles>1"}),
    ("splitk96-once16", 8, 100, 128, 4, 4, 1, 2, ("bf16x3",), dict(dw_off=(0, 1)), {"splitk>=32", "once16", "scalar16", "empty"}),
    ("splitk400-scalar64", 8, 100, 128, 4, 4, 1, 1, ("bf16x3",), dict(dw_off=(1,)), {"scalar64", "idle_group"}),
    ("splitk800-reduce4", 16, 100, 128, 132, 4, 1, 1, ("fp32",), dict(), {"reduce4x2", "kernel1"}),
    ("last-split-one-pixel", 1, 1, 769, 4, 132, 1, 1, BWD_MODES, dict(), {"last1px"}),
    ("last-split-one-stage", 1, 1, 832, 4, 132, 1, 1, ("bf16x3",), dict(), {"last1stage"}),
    ("halo-slabs", 1, 310, 517, 32, 32, 3, 1, ("bf16x3",), dict(dw_off=(0, 1)), {"kernel3"}),
    # slab counts that are no multiple of 4, of KG or of the rows per group: the `r + 4 <= r1` tails and a shorter last
    # group of every reducer.  The implicit GEMM plans whole groups of 8 slabs from 32 on, so the counts above 31 come
    # from the event-frame row kernel (one slab per block, as many blocks as output rows): the reducer is common code.
    ("event-frame-51-slabs", 3, 17, 23, 2, 16, 3, 1, ("bf16x3",), dict(dw_off=(0, 3)),
     {"kernel4", "once8", "tails:once8", "scalar4", "tails:scalar4"}),
    ("event-frame-101-slabs", 1, 101, 9, 2, 4, 3, 1, ("bf16x3",), dict(dw_off=(0, 1)),
     {"kernel4", "once16", "tails:once16", "scalar16", "tails:scalar16", "idle_group"}),
    ("event-frame-933-slabs", 3, 311, 40, 2, 4, 3, 1, ("bf16x3",), dict(dw_off=(0, 2)),
     {"kernel4", "reduce4x2", "tails:reduce4x2", "scalar64", "tails:scalar64"}),
]


def wgrad_plan(_hip, N, H, W, Cin, Cout, k, s, pad, ldx, lddy, align, prec):
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    out = (ctypes.c_int * 18)()
    rc = _hip.query("snn_conv2d_wgrad_plan", N, H, W, Cin, Ho, Wo, Cout, k, k, s, pad, ldx, lddy, align, prec, 0, 0,
                    ctypes.addressof(out))
    assert rc == 0, "snn_conv2d_wgrad_plan refuses the row"
    p = dict(zip(WGRAD_PLAN_KEYS, out))
    out2 = (ctypes.c_int * 18)()
    _hip.query("snn_conv2d_wgrad_plan", N, H, W, Cin, Ho, Wo, Cout, k, k, s, pad, ldx, lddy, align, prec, 0, _num_cu(),
               ctypes.addressof(out2))
    assert list(out) == list(out2), "num_cu = 0 does not plan for this device"
    return p


def _wgrad_classes(p, Wo):
    c = {f"kernel{p['kernel']}"}
    sk = p["splitk"]
    red = {0: "scalar", 1: "once", 2: "reduce4x", 3: "reduce4x"}[p["reducer"]] + str(p["kg"] if p["reducer"] < 2 else 4 - p["reducer"])
    c.add(red)
    launched = p["kg"] if p["reducer"] < 2 else p["groups"]
    if launched > p["groups"]:
        c.add("idle_group")
    # the scalar tail of the 4-row loop runs, the last group is shorter, and the slab count is no multiple of 4 or of KG
    # (two passes: nor is the number of group heads the second pass adds)
    if p["per"] % 4 and sk % p["per"] and sk % 4 and (p["kg"] == 1 or sk % p["kg"]) and (p["reducer"] != 2 or p["groups"] % 4):
        c.add(f"tails:{red}")
    if p["kernel"] > 2:
        return c
    c |= {f"tile{p['tile']}", f"stage{p['stage']}"}
    if p["kernel"] == 0 and sk > 1 and p["pps"] >= 3 * p["stage"] and p["last_pix"] < p["pps"]:
        c.add(f"tile{p['tile']}:multisplit")                            # pipelined, several stages per split, a short last split
    c.add("splitk1" if sk == 1 else "splitk2-7" if sk < 8 else "splitk>=32" if sk >= 32 else
          "splitk8-31%8" if sk % 8 == 0 else "splitk8-31!%8")
    if p["tiles_m"] * p["tiles_n"] > 1:
        c.add("tiles>1")
    if p["empty"]:
        c.add("empty")
    if sk > 1 and not p["empty"] and p["last_pix"] == 1:
        c.add("last1px")
    if sk > 1 and not p["empty"] and p["last_pix"] == p["stage"] < p["pps"]:
        c.add("last1stage")
    if sk > 1 and p["pps"] % Wo:
        c.add("row_split")
    return c


def _run_wgrad(_hip, x, dy, k, s, pad, prec, opt, *, dw_off=0, old=None):
    """snn_conv2d_wgrad into a guarded flat buffer at float offset dw_off, workspace exactly splitk * n floats between guards."""
    N, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    x_off, x_ld = opt.get("x", (0, None))
    X, DY = Buf(x.shape, x_off, x_ld, values=x), Buf(dy.shape, values=dy)
    n = Cout * k * k * Cin
    flat = torch.full((n + 12,), SENT, device="cuda")
    lo = 4 + dw_off
    flat[lo:lo + n] = old.reshape(-1).cuda() if old is not None else float("nan")
    before = flat.clone()
    dwv = flat[lo:lo + n]
    align = (1 if _a16(X.ptr) else 0) | (2 if X.ptr % 8 == 0 else 0) | (8 if _a16(DY.ptr) else 0) | (16 if DY.ptr % 8 == 0 else 0)
    p = wgrad_plan(_hip, N, H, W, Cin, Cout, k, s, pad, X.ld, DY.ld, align | (32 if _a16(dwv.data_ptr()) else 0), prec)
    splitk = p["splitk"]
    assert splitk == _hip.query("snn_conv2d_wgrad_splitk", N, H, W, Cin, Ho, Wo, Cout, k, k, s, pad, prec)
    wsb = torch.full((splitk * n + 2 * GUARD,), SENT, device="cuda")
    ws = wsb[GUARD:GUARD + splitk * n]
    ws.fill_(float("nan"))                                               # a slab nobody writes poisons dw
    assert _a16(ws.data_ptr())
    _hip.call("snn_conv2d_wgrad", X.ptr, X.ld, DY.ptr, DY.ld, dwv.data_ptr(), N, H, W, Cin, Ho, Wo, Cout, k, k, s, pad,
              int(old is not None), ws.data_ptr(), splitk, prec, _st())
    torch.cuda.synchronize()
    assert X.guards_intact(whole=True) and DY.guards_intact(whole=True)
    a, b = flat.view(torch.int32), before.view(torch.int32)
    assert torch.equal(a[:lo], b[:lo]) and torch.equal(a[lo + n:], b[lo + n:]), "snn_conv2d_wgrad wrote outside dw"
    g = wsb.cpu()
    assert bool((g[:GUARD] == SENT).all()) and bool((g[GUARD + splitk * n:] == SENT).all()), "wrote outside the workspace"
    return dwv.double().cpu().reshape(Cout, k, k, Cin), p


@pytest.mark.parametrize("row", WGRAD_ROWS, ids=[r[0] for r in WGRAD_ROWS])
def test_wgrad_row_against_fp64(H_, row):
    _hip = H_
    rid, N, H, W, Cin, Cout, k, s, modes, opt, want_classes = row
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    seed = N * 100 + H + W + Cin
    x, dy = _random((N, H, W, Cin), seed), _random((N, Ho, Wo, Cout), seed + 1)
    xi, dyi = _exact_operands((N, H, W, Cin), seed, lim=3), _exact_operands((N, Ho, Wo, Cout), seed + 1, lim=3)
    xd, dyd = x.double(), dy.double()
    ref, mag = _wgrad_ref(xd, dyd, k, k, s, pad), _wgrad_ref(xd.abs(), dyd.abs(), k, k, s, pad)
    refi = _wgrad_ref(xi.double(), dyi.double(), k, k, s, pad)
    assert float(refi.abs().max()) < 2 ** 24
    old = _random((Cout, k, k, Cin), seed + 2)
    oldi = _exact_operands((Cout, k, k, Cin), seed + 3) * 0.25
    seen = set()
    for name in modes:
        prec = _prec(_hip, name)
        for off in opt.get("dw_off", (0,)):
            out, p = _run_wgrad(_hip, x, dy, k, s, pad, prec, opt, dw_off=off)
            what = f"{rid} {name} dw+{off} ({N * Ho * Wo} px, {_num_cu()} CUs) plan {p}"
            seen |= _wgrad_classes(p, Wo)
            _check(what, out, ref, mag, name)
            _ratio(f"wgrad {name} {rid} dw+{off}", out, ref, mag, PREC_TOL[name] + ACC_TOL, splitk=p["splitk"], reducer=p["reducer"],
                   kg=p["kg"], chain=(p["pps"] // max(p["stage"], 1) if p["stage"] else 0) + p["per"] + p["kg"])
            if name != "bf16x1" and p["kernel"] <= 2 and p["splitk"] > 1:
                # the pixels of the last split that owns any dropped (flat pixel order: image, row, column)
                z0 = (p["splitk"] - p["empty"] - 1) * p["pps"]
                dz = dyd.clone().reshape(-1, Cout)
                part = torch.zeros_like(dz)
                part[z0:] = dz[z0:]
                drop = _wgrad_ref(xd, part.reshape(dyd.shape), k, k, s, pad)
                if float((drop.abs() / (mag + TINY)).max()) > 4 * (PREC_TOL[name] + ACC_TOL):
                    _teeth(what, out, ref - drop, mag, name)
            if name != "bf16x1":
                c = Cin // 2                                             # one input channel's gradient dropped
                wrong = ref.clone()
                wrong[..., c] = 0
                _teeth(what, out, wrong, mag, name)
            out, _ = _run_wgrad(_hip, x, dy, k, s, pad, prec, opt, dw_off=off, old=old)
            _check(f"{what} accumulate", out, ref + old.double(), mag, name, extra_mag=old.double().abs())
            out, _ = _run_wgrad(_hip, xi, dyi, k, s, pad, prec, opt, dw_off=off)
            assert torch.equal(out, refi), f"{what} exact: {int((out != refi).sum())} elements differ from fp64"
            out, _ = _run_wgrad(_hip, xi, dyi, k, s, pad, prec, opt, dw_off=off, old=oldi)
            assert torch.equal(out, refi + oldi.double()), f"{what} exact, accumulate: {int((out != refi + oldi.double()).sum())} differ"
    assert want_classes <= seen, f"{rid} ({_num_cu()} CUs): the row no longer reaches {want_classes - seen}; it shows {seen}"


# ---------------------------------------------------------------------------------------------------- production shapes
# GEN1 B = 5, T = 32 (N = 160): each once, fp64 on the device with torch (an independent implementation; the CPU takes
# minutes for these).  id, Cin, Cout, k, stride, H, W
# then: forward plan (loader, channel tile), data-gradient loaders of the phases, weight-gradient classes
PROD_ROWS = [
    ("neck-768-256-30x38", 768, 256, 1, 1, 30, 38, (2, 128), {2}, {"kernel0", "tile0", "stage32", "tile0:multisplit", "splitk>=32", "once4"}),
    ("down-64-128-s2-120x152", 64, 128, 3, 2, 120, 152, (2, 128), {2}, {"kernel3"}),
    ("head-256-27-30x38", 256, 27, 1, 1, 30, 38, (2, 32), {0}, {"kernel2", "tile2", "stage32", "splitk>=32", "empty", "once16"}),
]


@pytest.mark.parametrize("row", PROD_ROWS, ids=[r[0] for r in PROD_ROWS])
def test_production_shape_against_fp64(H_, row):
    _hip = H_
    rid, Cin, Cout, k, s, H, W, fwd_plan, dgrad_loaders, wgrad_classes = row
    N, pad = 160, k // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    import torch.nn.functional as F
    x, w, dy = _random((N, H, W, Cin), 1), _random((Cout, k, k, Cin), 2, (k * k * Cin) ** -0.5), _random((N, Ho, Wo, Cout), 3)
    xc, wc, dyc = (t.cuda().double() for t in (x, w, dy))
    nchw = lambda t: t.permute(0, 3, 1, 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    opt = {}
    # forward
    ref = nhwc(F.conv2d(nchw(xc), nchw(wc), stride=s, padding=pad)).cpu()
    mag = nhwc(F.conv2d(nchw(xc.abs()), nchw(wc.abs()), stride=s, padding=pad)).cpu()
    out, plans, _, _ = _run_gather(_hip, "fwd", x, w, (N, H, W, Cin, Cout, k, k, s, pad), _hip.PREC_FP16X3, opt)
    assert (plans[0]["loader"], plans[0]["bn"]) == fwd_plan and plans[0]["out_vec"] == (Cout % 4 == 0), (rid, _num_cu(), plans)
    _check(f"{rid} fwd {plans}", out, ref, mag, "fp16x3")
    _ratio(f"k_conv_gather fwd fp16x3 prod-{rid}", out, ref, mag, PREC_TOL["fp16x3"] + ACC_TOL)
    # data gradient
    gi = lambda a, b: nhwc(torch.nn.grad.conv2d_input((N, Cin, H, W), nchw(b), nchw(a), stride=s, padding=pad)).cpu()
    ref, mag = gi(dyc, wc), gi(dyc.abs(), wc.abs())
    out, plans, _, _ = _run_gather(_hip, "dgrad", dy, w, (N, H, W, Cin, Cout, k, k, s, pad), _hip.PREC_BF16X3, opt)
    assert {p["loader"] for p in plans} == dgrad_loaders and len(plans) == s * s, (rid, _num_cu(), plans)
    _check(f"{rid} dgrad {plans}", out, ref, mag, "bf16x3")
    _ratio(f"k_conv_gather dgrad bf16x3 prod-{rid}", out, ref, mag, PREC_TOL["bf16x3"] + ACC_TOL)
    # weight gradient
    gw = lambda a, b: torch.nn.grad.conv2d_weight(nchw(a), (Cout, Cin, k, k), nchw(b), stride=s, padding=pad).permute(0, 2, 3, 1).cpu()
    ref, mag = gw(xc, dyc), gw(xc.abs(), dyc.abs())
    del xc, wc, dyc
    out, p = _run_wgrad(_hip, x, dy, k, s, pad, _hip.PREC_BF16X3, opt)
    assert wgrad_classes <= _wgrad_classes(p, Wo), f"{rid} ({_num_cu()} CUs): {wgrad_classes - _wgrad_classes(p, Wo)} not in plan {p}"
    chain = (p["pps"] // p["stage"] if p["stage"] else 0) + p["per"] + p["kg"]   # longest sequential fp32 chain of the plan
    _ratio(f"wgrad bf16x3 prod-{rid}", out, ref, mag, PREC_TOL["bf16x3"] + ACC_TOL, splitk=p["splitk"], chain=chain,
           kernel=p["kernel"])
    _check(f"{rid} wgrad plan {p}", out, ref, mag, "bf16x3")


# ---------------------------------------------------------------------------------------------------- coverage
REQUIRED_CLASSES = {
    "gather": {"loader0", "loader1", "loader2", "loader3", "bn32", "bn64", "bn128", "ntiles_full", "ntiles_partial", "co%4",
               "out_vec", "out_scalar", "M<128", "M%128", "idle", "mtiles_per_xcd>1", "1x1", "3x3s2", "5x5", "7x7",
               "nonsquare", "phases4", "phases9", "phase_without_tap", "stride>H", "adds2", "inplace", "bn_straddle",
               "bn_multiple", "bn_T1", "bn_none"},
    "wgrad": {"kernel0", "kernel1", "kernel2", "kernel3", "kernel4", "tile0", "tile1", "tile2", "tile3", "tile4", "tile5",
              "stage32", "stage64", "splitk1", "splitk2-7", "splitk8-31%8", "splitk8-31!%8", "splitk>=32", "tiles>1", "empty",
              "last1px", "last1stage", "row_split", "once1", "once2", "once4", "once8", "once16", "reduce4x2", "scalar1",
              "scalar4", "scalar16", "scalar64", "idle_group", "tile0:multisplit", "tile1:multisplit", "tile2:multisplit",
              "tile3:multisplit", "tails:once2", "tails:once4", "tails:once8", "tails:once16", "tails:reduce4x2", "tails:scalar4",
              "tails:scalar16", "tails:scalar64"},
}


def test_every_gemm_plan_class_is_reached():
    """The tables' declared classes (each row asserts its own through the plan queries) cover the required ones."""
    got = set().union(*(r[-1] for r in GATHER_ROWS))
    assert REQUIRED_CLASSES["gather"] <= got, REQUIRED_CLASSES["gather"] - got
    got = set().union(*(r[-1] for r in WGRAD_ROWS))
    assert REQUIRED_CLASSES["wgrad"] <= got, REQUIRED_CLASSES["wgrad"] - got
