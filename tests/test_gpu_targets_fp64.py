"""The training-target kernels - snn_roi_assign (csrc/targets.hip) and snn_det_loss_fwd / _bwd (csrc/det_loss.hip) -
against the references of tests/targets_ref.py, at the edges of their launch geometry and of their arithmetic.

Both entry points are called through the C ABI (``_hip.call``) on buffers pre-filled with NaN (0x7F bytes for integer
buffers) with a guard region of the same fill behind every output and behind the workspace, and through ``roi.RoI`` /
``functional.detection_loss``, which must return the same bits.

Assignment (an integer decision on fp32 IoUs): classes, masks and the offset columns 10 * dxy / wh equal the fp32
reference bit for bit; the columns 5 * log(eps + wh / wh_a) go through the device logf and are bounded against the fp32
reference as the golden-vector test bounds them and against the fp64 offsets of the same assignment.

Loss: elementwise against the fp64 closed form; every bound is derived where it is used.  u = 2^-24 is the unit roundoff
of fp32.  The observed maxima (error / bound) per case are merged as JSON into the file SNN_FP64_RECORD names, when set.
"""
import json
import os

import pytest
import torch

from tests import targets_ref as TR

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 64                      # guard elements behind every buffer
ROI_CASES = TR.roi_cases()
_RECORD = {}
_REF = {}


@pytest.fixture(scope="module")
def hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from snn_for_object_detection_amd import _hip
    return _hip


def _st():
    return torch.cuda.current_stream().cuda_stream


def _record(key, rec):
    _RECORD[key] = rec
    path = os.environ.get("SNN_FP64_RECORD")
    if path:
        merged = {}
        if os.path.exists(path):
            try:
                with open(path) as f:
                    merged = json.load(f)
            except ValueError:
                merged = {}
        merged.update(_RECORD)
        with open(path, "w") as f:
            json.dump(merged, f, indent=1, sort_keys=True)


class Guarded:
    """n elements pre-filled with NaN (floating) or 0x7F bytes (integer), and GUARD more of the same behind them."""

    def __init__(self, n, dtype):
        fill = float("nan") if dtype.is_floating_point else (0x7F if dtype == torch.uint8 else 0x7F7F7F7F7F7F7F7F)
        self.n = n
        self.buf = torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")
        self.fill_bytes = self.buf[n:].clone().view(torch.uint8)
        self.ptr = self.buf.data_ptr()

    def out(self, *shape):
        return self.buf[:self.n].reshape(*shape).cpu()

    def guard_intact(self):
        return torch.equal(self.buf[self.n:].view(torch.uint8), self.fill_bytes)

    def untouched(self):
        n = min(self.n, GUARD)
        return self.guard_intact() and torch.equal(self.buf[:n].view(torch.uint8),
                                                   self.fill_bytes[:n * self.buf.element_size()])


# ====================================================================================================== assignment
def _roi_ref(cs):
    if cs.id not in _REF:
        _REF[cs.id] = TR.roi_assign_ref(cs.anchors, cs.labels, cs.thr)
    return _REF[cs.id]


def run_roi_abi(hip, anchors, labels, thr):
    """snn_roi_assign through the C ABI on guarded buffers -> (offset, mask, cls) on the host."""
    anchors, labels = anchors.cuda().contiguous(), labels.cuda().contiguous()
    B, N, _ = labels.shape
    A = anchors.shape[0]
    ws = Guarded(hip.query("snn_roi_workspace_size", B, A, N), torch.uint8)
    off, mask, cls = Guarded(B * A * 4, torch.float32), Guarded(B * A * 4, torch.float32), Guarded(B * A, torch.int64)
    hip.call("snn_roi_assign", anchors.data_ptr(), labels.data_ptr(), B, A, N, float(thr), ws.ptr, off.ptr, mask.ptr,
             cls.ptr, _st())
    torch.cuda.synchronize()
    for name, g in (("workspace", ws), ("offset", off), ("mask", mask), ("class", cls)):
        assert g.guard_intact(), f"the guard behind the {name} buffer changed"
    return off.out(B, A, 4), mask.out(B, A, 4), cls.out(B, A)


def check_roi(ref, off, mask, cls, rec):
    assert cls.dtype == torch.int64 and torch.equal(cls, ref.classes)
    assert torch.equal(mask, ref.masks)
    assert torch.equal(off[..., :2], ref.offsets[..., :2])                         # 10 * dxy / wh: the same roundings
    assert torch.allclose(off, ref.offsets, rtol=3e-7, atol=1e-6)                   # 5 * log(...): the device logf
    # against fp64: the operands sit on the 1/64 grid, so centres, sizes and 10 * (difference) are exact and columns
    # 0 / 1 round once, in the division: u |r|.
    err = (off.double() - ref.offsets64).abs()
    r64 = ref.offsets64.abs()
    xy = float((err[..., :2] / (U * r64[..., :2] + 1e-300)).max())
    # Columns 2 / 3, 5 * logf(eps + tw / aw), round four times: the division and the add of eps each move the argument
    # of the logarithm by <= u relative, that is log by <= u absolute, 5 (u + u) after the multiplication; logf is
    # within 1 ulp = 2 u of its result and the multiplication by 5 within u: u (10 + 3 |r|).  (4 u (1 + |r|), one u per
    # rounding relative to the result, does not hold near r = 0, where the roundings of the ARGUMENT count five-fold:
    # the reference's own fp32 arithmetic is at 1.5 times that bound on these cases.)
    wh = float((err[..., 2:] / (U * (10.0 + 3.0 * r64[..., 2:]))).max())
    rec["offset_xy_vs_fp64"], rec["offset_wh_vs_fp64"] = xy, wh
    assert xy <= 1.0, f"offsets 0 / 1: max |d - r64| / (u |r64|) = {xy:.3g}"
    assert wh <= 1.0, f"offsets 2 / 3: max |d - r64| / (u (10 + 3 |r64|)) = {wh:.3g}"


@pytest.mark.parametrize("cs", ROI_CASES, ids=[c.id for c in ROI_CASES])
def test_roi_assign_against_the_reference(hip, cs):
    from snn_for_object_detection_amd.roi import RoI
    ref = _roi_ref(cs)
    if cs.check is not None:
        cs.check(ref)                                   # the edge the case is there for is reached by the reference
    off, mask, cls = run_roi_abi(hip, cs.anchors, cs.labels, cs.thr)
    rec = {"A": cs.anchors.shape[0], "N": cs.labels.shape[1], "B": cs.labels.shape[0]}
    check_roi(ref, off, mask, cls, rec)
    _record(f"roi/{cs.id}", rec)
    o2, m2, c2 = RoI(cs.thr)(cs.anchors.cuda(), cs.labels.cuda())
    assert c2.dtype == torch.int64 and torch.equal(c2.cpu(), cls) and torch.equal(m2.cpu(), mask)
    assert torch.equal(o2.cpu().view(torch.int32), off.view(torch.int32))


def test_roi_assign_sample_is_independent_of_its_batch(hip):
    """Every sample of the B = 4 case equals its own B = 1 call bit for bit (per-sample workspace offsets)."""
    cs = next(c for c in ROI_CASES if c.id == "batch4")
    off, mask, cls = run_roi_abi(hip, cs.anchors, cs.labels, cs.thr)
    ref = _roi_ref(cs)
    assert [r[2] for r in ref.rounds[1]] == list(range(7))          # the all-padding sample claims anchors 0 .. 6
    for b in range(cs.labels.shape[0]):
        o1, m1, c1 = run_roi_abi(hip, cs.anchors, cs.labels[b:b + 1], cs.thr)
        assert torch.equal(c1[0], cls[b]) and torch.equal(m1[0], mask[b]), b
        assert torch.equal(o1[0].view(torch.int32), off[b].view(torch.int32)), b


def test_roi_assign_refusals(hip):
    """Host-side refusals: nothing is launched, the outputs keep their fill."""
    A, N = 8, 2
    anchors = TR.grid_boxes(A + 1, torch.Generator().manual_seed(1)).cuda()
    labels = torch.zeros(1, N, 5, device="cuda")
    ws, off, mask = Guarded(1024, torch.uint8), Guarded(A * 4 + 4, torch.float32), Guarded(A * 4, torch.float32)
    cls = Guarded(A, torch.int64)
    good = [anchors.data_ptr(), labels.data_ptr(), 1, A, N, 0.5, ws.ptr, off.ptr, mask.ptr, cls.ptr, _st()]

    def refused(**kw):
        args = list(good)
        for k, v in kw.items():
            args[int(k[1:])] = v
        with pytest.raises(RuntimeError, match="snn_roi_assign"):
            hip.call("snn_roi_assign", *args)

    for i in (0, 1, 6, 7, 8, 9):
        refused(**{f"a{i}": None})                       # null pointers
    refused(a3=1 << 16, a4=1 << 15)                      # A * N = 2^31
    refused(a3=(1 << 31) - 1, a4=1)
    refused(a2=0)
    refused(a3=0)
    refused(a4=0)
    refused(a0=anchors.data_ptr() + 4)                   # boxes are read and written as float4
    refused(a7=off.ptr + 4)
    refused(a8=mask.ptr + 4)
    refused(a6=ws.ptr + 4)
    torch.cuda.synchronize()
    assert ws.untouched() and off.untouched() and mask.untouched() and cls.untouched()
    hip.call("snn_roi_assign", *good)                    # the same arguments unchanged are accepted
    torch.cuda.synchronize()


# ====================================================================================================== loss
LOSS_SHAPES = [(1, 2), (255, 3), (256, 3), (257, 3), (1025, 8), (40_635, 3), (5000, 64), (1_048_576 + 300, 2)]
LOSS_CONDS = ("base", "g_ratio", "no_pos", "no_neg", "big_logits")


class LossOut:
    pass


def run_loss_abi(hip, inputs):
    logits, bbox, offset, mask, labels, ratio, g_loss = inputs
    R, K = logits.shape
    d = [t.cuda().contiguous() for t in (logits, bbox, offset, mask, labels)]
    ws = Guarded(hip.query("snn_det_loss_workspace_size", R), torch.uint8)
    stats, loss = Guarded(5, torch.float64), Guarded(1, torch.float32)
    gl, gb = Guarded(R * K, torch.float32), Guarded(R * 4, torch.float32)
    g = torch.tensor([g_loss], dtype=torch.float32, device="cuda")
    ptrs = [t.data_ptr() for t in d]
    hip.call("snn_det_loss_fwd", *ptrs, R, K, float(ratio), ws.ptr, stats.ptr, loss.ptr, _st())
    hip.call("snn_det_loss_bwd", *ptrs, R, K, float(ratio), stats.ptr, g.data_ptr(), gl.ptr, gb.ptr, _st())
    torch.cuda.synchronize()
    for name, b in (("workspace", ws), ("stats", stats), ("loss", loss), ("g_logits", gl), ("g_bbox", gb)):
        assert b.guard_intact(), f"the guard behind the {name} buffer changed"
    o = LossOut()
    o.stats, o.loss, o.g_logits, o.g_bbox = stats.out(5), loss.out(1)[0], gl.out(R, K), gb.out(R, 4)
    o.device_inputs = d
    return o


def check_loss(K, ref, o, fails, rec):
    # ---- counts: integers below 2^53 accumulated in fp64
    if float(o.stats[1]) != float(ref.stats[1]) or float(o.stats[3]) != float(ref.stats[3]):
        fails.append(f"counts {o.stats[1]}, {o.stats[3]} != {ref.stats[1]}, {ref.stats[3]}")
    # ---- sums.  Per row se = sum of K expf (1 ulp = 2 u each, the rounded argument x - mx adds t e^-t u <= 0.37 u of
    # se) accumulated in fp32 ((K - 1) u): (K + 1.4) u relative, which is the absolute error of log(se); logf adds 2 u
    # of its result, x[y] - mx and the final subtraction u each: <= (K + 1.4) u + 4 u CE per row, below (K + 8) u of
    # the sum as long as the mean CE of the group is O(1); the rows are then added in fp64.  The L1 sum rounds once
    # per element (the products with a 0 / 1 mask are exact).
    for i, name in ((0, "ce_pos"), (2, "ce_neg"), (4, "l1")):
        r, d = float(ref.stats[i]), float(o.stats[i])
        if r == 0.0:
            ratio = 0.0 if d == 0.0 else float("inf")
        else:
            ratio = abs(d - r) / ((K + 8) * U * abs(r))
        rec[name] = ratio
        if not ratio <= 1.0:
            fails.append(f"stats[{i}] ({name}): |d - r| / ((K + 8) u |r|) = {ratio:.3g}")
    # ---- loss: the three quotients are rounded to fp32 and combined by two multiplications and two additions of
    # positive terms; bounded at 2^-22 of the reference
    d = float(o.loss)
    if ref.loss != ref.loss:
        if d == d:
            fails.append(f"loss {d} where the reference is NaN")
    else:
        ratio = abs(d - ref.loss) / (2.0 ** -22 * abs(ref.loss))
        rec["loss"] = ratio
        if not ratio <= 1.0:
            fails.append(f"loss: |d - r| / (2^-22 |r|) = {ratio:.3g} ({d} vs {ref.loss})")
    # ---- g_logits = w (p - onehot), elementwise.  w: ratio (or 1 - ratio, one more rounding) times g, divided by the
    # count: <= 3 u.  p = expf / se: 2 u + 0.4 u + (K + 1.4) u + u; the subtraction and the product u each:
    # (K + 9.8) u of |w| since |p - onehot| <= 1, below (K + 8) 2 u.
    if not bool(torch.isfinite(o.g_logits).all()):
        fails.append(f"g_logits: {int((~torch.isfinite(o.g_logits)).sum())} non-finite entries")
    err = (o.g_logits.double() - ref.g_logits).abs()
    bound = (K + 8) * 2 * U * ref.w.abs()[:, None]
    ratio = float((err / bound).max())
    rec["g_logits"] = ratio
    if not ratio <= 1.0:
        r = int((err / bound).max(dim=1).values.argmax())
        fails.append(f"g_logits: max |d - r| / ((K + 8) 2^-23 |w|) = {ratio:.3g} at row {r}")
    # ---- g_bbox = w_l1 sign(.) mask with w_l1 = g / (4 R): 4 R is exact (R < 2^22), one division
    err = (o.g_bbox.double() - ref.g_bbox).abs()
    ratio = float(err.max() / (2 * U * abs(ref.w_l1)))
    rec["g_bbox"] = ratio
    if not ratio <= 1.0:
        fails.append(f"g_bbox: max |d - r| / (2^-23 |w_l1|) = {ratio:.3g}")
    if not torch.equal(torch.sign(o.g_bbox.double()), torch.sign(ref.g_bbox)):
        bad = int((torch.sign(o.g_bbox.double()) != torch.sign(ref.g_bbox)).sum())
        fails.append(f"g_bbox: sign / zero pattern differs at {bad} entries")


@pytest.mark.parametrize("cond", LOSS_CONDS)
@pytest.mark.parametrize("rows,K", LOSS_SHAPES, ids=[f"{r}x{k}" for r, k in LOSS_SHAPES])
def test_det_loss_against_fp64(hip, rows, K, cond):
    """Every shape under every condition: g_loss in {1, -2.5} with ratio in {0.04, 0.5}; no positives (loss NaN on both
    sides, gradients of the negatives finite and equal to the reference); no negatives; logits shifted / scaled to a row
    maximum of +-80; every case carries rows with bbox * mask == offset * mask (gradient exactly 0) and class 0 with
    mask 1."""
    from snn_for_object_detection_amd import functional as HF
    inputs = TR.loss_inputs(rows, K, cond, seed=rows * 131 + K)
    logits, bbox, offset, mask, labels, ratio, g_loss = inputs
    ref = TR.det_loss_ref(*inputs)
    diff = bbox.double() * mask.double() - offset.double() * mask.double()
    assert bool((diff == 0).any())
    if cond == "no_pos":
        assert ref.loss != ref.loss and int(ref.stats[1]) == 0 and bool(torch.isfinite(ref.g_logits).all())
    if cond == "no_neg":
        assert int(ref.stats[3]) == 0
    if cond == "big_logits":
        assert float(logits.max(dim=1).values.abs().min()) >= 79.9
    o = run_loss_abi(hip, inputs)
    fails, rec = [], {}
    check_loss(K, ref, o, fails, rec)
    _record(f"loss/{rows}x{K}/{cond}", rec)
    assert not fails, f"{rows}x{K} [{cond}]:\n  " + "\n  ".join(fails)
    # ---- the same through functional.detection_loss: the same bits
    lg, bb, of, mk, lb = o.device_inputs
    lg, bb = lg.clone().requires_grad_(), bb.clone().requires_grad_()
    loss = HF.detection_loss(lg.view(1, rows, K), bb.view(1, rows, 4), of.view(1, rows, 4), mk.view(1, rows, 4),
                             lb.view(1, rows), ratio)
    (loss * g_loss).backward()
    assert torch.equal(loss.detach().cpu().reshape(1).view(torch.int32), o.loss.reshape(1).view(torch.int32))
    assert torch.equal(lg.grad.cpu(), o.g_logits) and torch.equal(bb.grad.cpu(), o.g_bbox)


def test_det_loss_of_well_classified_rows_with_large_logits(hip):
    """Regression: -log_softmax(x)[y] must not be formed as (mx + log(se)) - x[y], which rounds at the size of mx = 80
    (2^-18 = 3.8e-6) while the value is log(1 + e^-d) = 0.3 ... 0.7.  Three positive and three negative rows, each
    labelled with its maximum."""
    logits = torch.tensor([[80.0, 80.0], [79.0, 80.0], [79.5, 80.0], [-80.0, -80.0], [-80.0, -81.0], [-80.0, -80.5]])
    labels = torch.tensor([1, 1, 1, 0, 0, 0])
    z = torch.zeros(6, 4)
    ref = TR.det_loss_ref(logits, z, z, z, labels, 0.5)
    o = run_loss_abi(hip, (logits, z, z, z, labels, 0.5, 1.0))
    fails = []
    check_loss(2, ref, o, fails, {})
    assert not fails, fails


def test_det_loss_refusals(hip):
    """Host-side refusals of both entry points: nothing is launched, the outputs keep their fill."""
    R, K = 16, 3
    inputs = TR.loss_inputs(R, K, "base", seed=5)
    d = [t.cuda().contiguous() for t in inputs[:5]]
    spare = torch.zeros(R * 4 + 4, device="cuda")
    ws = Guarded(hip.query("snn_det_loss_workspace_size", R), torch.uint8)
    stats, loss = Guarded(5, torch.float64), Guarded(1, torch.float32)
    gl, gb = Guarded(R * 65, torch.float32), Guarded(R * 4 + 4, torch.float32)
    g = torch.ones(1, device="cuda")
    ok_stats = torch.ones(5, dtype=torch.float64, device="cuda")
    ptrs = [t.data_ptr() for t in d]
    fwd = ptrs + [R, K, 0.04, ws.ptr, stats.ptr, loss.ptr, _st()]
    bwd = ptrs + [R, K, 0.04, ok_stats.data_ptr(), g.data_ptr(), gl.ptr, gb.ptr, _st()]

    def refused(name, good, **kw):
        args = list(good)
        for k, v in kw.items():
            args[int(k[1:])] = v
        with pytest.raises(RuntimeError, match=name):
            hip.call(name, *args)

    for name, good, ptr_args in (("snn_det_loss_fwd", fwd, (0, 1, 2, 3, 4, 8, 9, 10)),
                                 ("snn_det_loss_bwd", bwd, (0, 1, 2, 3, 4, 8, 9, 10, 11))):
        for i in ptr_args:
            refused(name, good, **{f"a{i}": None})                      # null pointers
        refused(name, good, a6=1)                                       # K = 1: no class next to the background
        refused(name, good, a6=65)                                      # K above the kernel's 64
        refused(name, good, a5=0)                                       # rows = 0
        for i in (1, 2, 3):                                             # box tensors are read as float4
            refused(name, good, **{f"a{i}": spare.data_ptr() + 4})
    refused("snn_det_loss_bwd", bwd, a11=gb.ptr + 4)
    torch.cuda.synchronize()
    assert ws.untouched() and stats.untouched() and loss.untouched() and gl.untouched() and gb.untouched()


def test_detection_loss_refuses_targets_that_are_not_fp32_device_tensors(hip):
    """functional.detection_loss hands raw pointers to the kernel: offsets / masks on the host or in another dtype are
    refused on the host (RuntimeError) instead of being read as device addresses."""
    from snn_for_object_detection_amd import functional as HF
    R, K = 16, 3
    logits, bbox, offset, mask, labels, ratio, _ = TR.loss_inputs(R, K, "base", seed=6)
    lg, bb, of, mk, lb = (t.cuda().view(1, R, -1) for t in (logits, bbox, offset, mask, labels.view(R, 1)))
    lb = lb.view(1, R)
    HF.detection_loss(lg, bb, of, mk, lb, ratio)
    for bad_of, bad_mk in ((of.cpu(), mk), (of.double(), mk), (of, mk.cpu()), (of, mk.double()), (of, mk.bool()),
                           (of.half(), mk)):
        with pytest.raises(RuntimeError):
            HF.detection_loss(lg, bb, bad_of, bad_mk, lb, ratio)
    with pytest.raises(RuntimeError):
        HF.detection_loss(lg, bb, of, mk, lb.cpu(), ratio)
    with pytest.raises(RuntimeError):
        HF.detection_loss(lg, bb, of, mk[:, :R - 1], lb, ratio)
    torch.cuda.synchronize()
