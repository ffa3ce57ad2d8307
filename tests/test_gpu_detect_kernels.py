"""The detection tail of csrc/detect.hip kernel by kernel, through the C ABI on guarded buffers, against the restatement
of tests/detect_ref.py (which tests/test_detect_ref_host.py holds against the goldens, the host path and the oracle).

Every output buffer is pre-filled (NaN for floats, 0x7F bytes for integers) and stands between two guards of the same
fill that must come back bit for bit; what a kernel has no reason to write must still hold the fill.  Inputs are built by
hand (boxes, order, seg; flags and ranks from the restatement), so each kernel is tested alone.

NMS and assembly run on EXACT inputs: boxes on the grid k * 2^-6 in [0, 8), where every difference, product and sum of
iou_of is exact in float32 and its one division is correctly rounded on both sides - kept sets, ranks and output rows
are compared with torch.equal, no tolerance, no row left out.  (That the device division is correctly rounded is hipcc's
default and is the premise of these rows, not something they measure: a mismatch at an exact quotient is a finding.)

Decode: classes and confidences bit for bit; boxes bit for bit against the float32 restatement on exact inputs (size
offsets 0), and against the fp64 restatement on general inputs within k * u * mag, u = 2^-24,
mag = |acx| + |off * aw / 10| + 0.5 * w * (1 + |off_wh / 5|).  Counting the float32 roundings of decode_box, each of them
relative to the term it rounds:
  off * aw / 10 : aw, the product, the division, the sum with acx, the corner's own sum          -> 5
  acx           : its own sum (the halving is exact), the sum with the offset term, the corner   -> 3
  0.5 * w       : aw, the product with aw, the corner (the halving is exact)                     -> 3
                  expf itself, E ulp = 2 E u relative                                            -> 2 E
                  the rounding of off_wh / 5 moves the exponential by u |off_wh / 5| relative    -> the factor in mag
so k = max(5, 3 + 2 E) (+ 0.01 for the second-order terms).  E: no document on the build machine states the accuracy of
the device expf, so it is measured here against fp64 on the very size offsets of the general rows (an anchor
[-1, -1, 1, 1] with centre offsets 0 makes the decoded corner expf(off / 5) itself, exactly) and EXPF_ULP is twice the
measured maximum: 0.734 ulp on the MI355X (over the 504 arguments of row 255-K9; 0.51 .. 0.73 on the other rows), so
E = 1.5 and k = 6.  The test asserts that the measurement stays below E.  The largest error / bound ratio of every row is
printed (RATIO lines, -s) and merged as JSON into the file SNN_FP64_RECORD names, when it is set.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import detect_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 64                       # guard elements on both sides of every output (64 floats = 256 bytes: alignment is kept)
EXPF_ULP = 1.5                   # twice the measured maximum error (0.734 ulp) of the device expf, rounded up
K_DECODE = max(5.0, 3.0 + 2.0 * EXPF_ULP) + 0.01
INT_FILL = 0x7F7F7F7F
_RECORD = {}


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


def same(a, b):
    """torch.equal with NaN equal to NaN."""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


class Out:
    """n elements between two guards of GUARD elements, all pre-filled: NaN (float32), 0x7F bytes (int32, uint8).
    ``skew`` moves the payload by that many elements (a pointer that is not 16-byte aligned)."""

    def __init__(self, n, dtype, skew=0):
        fill = float("nan") if dtype.is_floating_point else (0x7F if dtype == torch.uint8 else INT_FILL)
        self.n, self.lo = n, GUARD + skew
        self.buf = torch.full((2 * GUARD + skew + n,), fill, dtype=dtype, device="cuda")
        self.before = self.buf.clone().view(torch.uint8)
        self.ptr = self.buf[self.lo:].data_ptr()

    def host(self, *shape):
        t = self.buf[self.lo:self.lo + self.n].cpu()
        return t.reshape(*shape) if shape else t

    def guards_intact(self):
        e = self.buf.element_size()
        now = self.buf.view(torch.uint8)
        return torch.equal(now[:self.lo * e], self.before[:self.lo * e]) and \
            torch.equal(now[(self.lo + self.n) * e:], self.before[(self.lo + self.n) * e:])

    def untouched(self):
        return torch.equal(self.buf.view(torch.uint8), self.before)


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


# =================================================================================================================== NMS
NMS_NAMES = R.NMS_CASE_NAMES      # the cases themselves are built when a test asks for them


def check_nms(name, outs, exp):
    """kept / nkept / kept_flag / kept_rank of the device against the restatement's: written entries equal, every other
    entry still the fill, every guard intact."""
    kept, nkept, flag, rank = outs
    e_kept, e_nkept, e_flag, e_rank = exp
    for what, o in zip(("kept", "nkept", "kept_flag", "kept_rank"), outs):
        assert o.guards_intact(), f"{name}: a guard of {what} changed"
    assert torch.equal(nkept.host().long(), torch.from_numpy(e_nkept.reshape(-1))), f"{name}: nkept"
    want_kept = torch.from_numpy(np.where(e_kept == R.FILL, INT_FILL, e_kept))
    assert torch.equal(kept.host().long(), want_kept), f"{name}: kept ids, or an entry past lo + nkept was written"
    assert torch.equal(flag.host().long(), torch.from_numpy(np.where(e_flag, 1, 0x7F))), f"{name}: kept_flag"
    assert torch.equal(rank.host().long(), torch.from_numpy(np.where(e_flag, e_rank, INT_FILL))), f"{name}: kept_rank"


@pytest.mark.parametrize("name", NMS_NAMES)
def test_nms_sorted(hip, name):
    case = R.nms_case(name)
    A, C = case.A, case.C
    boxes, order, seg = dev(case.boxes, torch.float32), dev(case.order, torch.int32), dev(case.seg, torch.int32)
    outs = (Out(A, torch.int32), Out(C, torch.int32), Out(A, torch.uint8), Out(A, torch.int32))
    hip.call("snn_nms_sorted", boxes.data_ptr(), order.data_ptr(), seg.data_ptr(), C, float(case.thr),
             *(o.ptr for o in outs), _st())
    torch.cuda.synchronize()
    check_nms(case.name, outs, case.expected())


@pytest.mark.parametrize("i", range(len(NMS_NAMES)), ids=NMS_NAMES)
def test_nms_sorted_batched(hip, i):
    """The case as frame i % 3 of three, between two other inputs made from it; with C = 1024 its own frame carries
    malformed seg rows (decreasing, above A, negative): those classes report nkept = 0 and write nothing."""
    case, pos = R.nms_case(NMS_NAMES[i]), i % 3
    A, C = case.A, case.C
    b, o, s, bad = R.batched_frames(case, pos)
    exp = R.nms_sorted_batched(b, o, s, 3, A, case.thr)
    boxes, order, seg = dev(b, torch.float32), dev(o, torch.int32), dev(s, torch.int32)
    outs = (Out(3 * A, torch.int32), Out(3 * C, torch.int32), Out(3 * A, torch.uint8), Out(3 * A, torch.int32))
    hip.call("snn_nms_sorted_batched", boxes.data_ptr(), order.data_ptr(), seg.data_ptr(), 3, A, C, float(case.thr),
             *(o_.ptr for o_ in outs), _st())
    torch.cuda.synchronize()
    check_nms(case.name, outs, exp)
    # the case's own frame is the single-frame result (but for the classes whose seg rows are malformed)
    single = case.expected()
    live = np.ones(C, bool)
    live[list(bad)] = False
    got = outs[1].host(3, C)[pos].numpy()
    assert np.array_equal(got[live], single[1][live]) and not got[~live].any()


# ============================================================================================================== assemble
ASSEMBLE_RUNS = [(A, 3, names) for A in R.ASSEMBLE_SIZES for names in (R.PATTERNS[:3], R.PATTERNS[3:])]
ASSEMBLE_RUNS += [(257, 1, R.PATTERNS[:3]), (257, 1024, R.PATTERNS[3:]), (513, 1024, R.PATTERNS[:3])]


def assemble_args(A, C, names):
    conf, cls, boxes, nkept, flag, rank = R.assemble_input(A, C, names)
    want = R.assemble(conf, cls, boxes, nkept, flag, rank, R.POS_THRESHOLD)
    args = (dev(conf, torch.float32), dev(cls, torch.int32), dev(boxes, torch.float32), dev(nkept, torch.int32),
            dev(flag, torch.uint8), dev(rank, torch.int32))
    return args, want


@pytest.mark.parametrize("A,C,names", ASSEMBLE_RUNS, ids=[f"A{a}-C{c}-{n[0]}" for a, c, n in ASSEMBLE_RUNS])
def test_detect_assemble(hip, A, C, names):
    """Three frames with three kept patterns: every output position is written (the class column of a NaN-filled out
    holds no NaN; A rows onto A positions: exactly once) with the restatement's row - weak rows, conf == pos_threshold
    and NaN confidences among them.  One KEPT row of every frame that keeps any has a NaN confidence: NaN is not weak, so
    it keeps its class and its NaN (a not-kept row says nothing here: it has class -1 and NaN either way)."""
    args, want = assemble_args(A, C, names)
    out = Out(3 * A * 6, torch.float32)
    hip.call("snn_detect_assemble", *(a.data_ptr() for a in args), 3, A, C, R.POS_THRESHOLD, out.ptr, _st())
    torch.cuda.synchronize()
    assert out.guards_intact()
    got = out.host(3, A, 6)
    assert not torch.isnan(got[..., 0]).any() and not torch.isnan(got[..., 2:]).any(), "an output row was not written"
    assert same(got, want)
    conf, cls, _, nkept, flag, rank = R.assemble_input(A, C, names)
    for n in range(3):
        kept_nan = np.flatnonzero(flag[n] & np.isnan(conf[n]))
        assert len(kept_nan) == (1 if flag[n].any() else 0)
        for a in kept_nan:
            row = got[n, R.assemble_positions(cls[n], nkept[n], flag[n], rank[n])[a]]
            assert float(row[0]) == float(cls[n, a]) >= 0 and torch.isnan(row[1]), "a kept NaN confidence counted as weak"


def test_detect_assemble_refuses_1025_classes(hip, hip_lib):
    args, _ = assemble_args(65, 3, R.PATTERNS[:3])
    out = Out(3 * 65 * 6, torch.float32)
    rc = hip_lib.snn_detect_assemble(*(a.data_ptr() for a in args), 3, 65, 1025, R.POS_THRESHOLD, out.ptr, _st())
    torch.cuda.synchronize()
    assert rc != 0 and b"snn_detect_assemble" in hip_lib.snn_last_error() and out.untouched()


# ================================================================================================================ decode
DECODE_SHAPES = [((A,), K) for A in (1, 255, 256, 257) for K in (2, 3, 9)] + [((3, 257), K) for K in (2, 3, 9)]
DECODE_IDS = ["x".join(map(str, s)) + f"-K{k}" for s, k in DECODE_SHAPES]


def run_decode(hip, prob, offsets, anchors, skew=0):
    """snn_detect_decode for [A, K], snn_detect_decode_batched for [N, A, K] -> conf, cls, boxes on the host."""
    A, K = prob.shape[-2:]
    rows = prob.numel() // K
    p, o, a = prob.cuda().contiguous(), offsets.cuda().contiguous(), anchors.cuda().contiguous()
    conf, cls, boxes = Out(rows, torch.float32), Out(rows, torch.int32), Out(rows * 4, torch.float32, skew=skew)
    if prob.dim() == 2:
        hip.call("snn_detect_decode", p.data_ptr(), o.data_ptr(), a.data_ptr(), A, K, conf.ptr, cls.ptr, boxes.ptr, _st())
    else:
        hip.call("snn_detect_decode_batched", p.data_ptr(), o.data_ptr(), a.data_ptr(), prob.shape[0], A, K, conf.ptr,
                 cls.ptr, boxes.ptr, _st())
    torch.cuda.synchronize()
    assert conf.guards_intact() and cls.guards_intact() and boxes.guards_intact()
    shape = prob.shape[:-1]
    return conf.host(*shape), cls.host(*shape), boxes.host(*shape, 4)


def check_argmax(prob, conf, cls):
    want_conf, want_cls = R.argmax_first(prob)
    assert torch.equal(cls, want_cls)
    nan = torch.isnan(want_conf)
    assert torch.equal(torch.isnan(conf), nan)
    assert torch.equal(conf[~nan].view(torch.int32), want_conf[~nan].view(torch.int32))      # the bits: -0 is -0


@pytest.mark.parametrize("shape,K", DECODE_SHAPES, ids=DECODE_IDS)
def test_decode_exact(hip, shape, K):
    """Dyadic anchors, size offsets 0: classes, confidences and boxes equal the float32 restatement bit for bit - the
    argmax table (ties, all equal, NaN rows, +0 / -0) in the first rows of the last frame.  The batched form uses the
    anchor row % A; the boxes pointer of the decode entry points needs no alignment (skew 1)."""
    A = shape[-1]
    prob, off, anchors = R.decode_probs(shape, K, seed=A + K), R.exact_offsets(shape, seed=A), R.dyadic_anchors(A, seed=A)
    _, _, want = R.decode(prob, off, anchors, torch.float32)
    assert not torch.isnan(want).any() and float(want[want != 0].abs().min()) > 2.0 ** -100
    for skew in (0, 1):
        conf, cls, boxes = run_decode(hip, prob, off, anchors, skew=skew)
        check_argmax(prob, conf, cls)
        assert torch.equal(boxes, want), f"skew {skew}"
    if len(shape) == 2:          # a frame's rows do not depend on the frames around it
        conf1, cls1, boxes1 = run_decode(hip, prob[1], off[1], anchors)
        assert same(conf1, conf[1]) and torch.equal(cls1, cls[1]) and torch.equal(boxes1, boxes[1])


def measure_expf(hip, offsets):
    """Largest error, in ulps of the result, of the device expf on fl32(off / 5) for the size offsets of ``offsets``."""
    off = offsets.reshape(-1, 4).clone()
    off[:, :2] = 0
    anchors = torch.tensor([[-1.0, -1.0, 1.0, 1.0]]).repeat(off.shape[0], 1)
    prob = torch.zeros(off.shape[0], 2)
    _, _, boxes = run_decode(hip, prob, off, anchors)
    arg = (off[:, 2:] / 5).double()                              # the float32 quotient the kernel forms
    ref = torch.exp(arg)
    ok = torch.isfinite(ref) & (ref > 2.0 ** -120) & (ref < 2.0 ** 120)
    got = boxes[:, 2:].double()
    ulp = torch.from_numpy(np.spacing(ref.float().numpy())).double()
    return float(((got - ref).abs() / ulp)[ok].max()), int(ok.sum())


def decode_bound(offsets, anchors):
    """mag of the module docstring, per coordinate, in fp64."""
    off = offsets.double()
    anc = anchors.double()
    centre = torch.stack(((anc[:, 0] + anc[:, 2]) / 2, (anc[:, 1] + anc[:, 3]) / 2), dim=-1)
    size = torch.stack((anc[:, 2] - anc[:, 0], anc[:, 3] - anc[:, 1]), dim=-1)
    wh = torch.exp(off[..., 2:] / 5) * size
    mag = centre.abs() + (off[..., :2] * size / 10).abs() + 0.5 * wh * (1 + (off[..., 2:] / 5).abs())
    return torch.cat((mag, mag), dim=-1)


def decode_ratio(boxes, ref, mag):
    """max |boxes - ref| / (k u mag) over the coordinates whose yardstick is finite; the others must be equal."""
    fin = torch.isfinite(ref)
    assert torch.equal(boxes.double()[~fin], ref[~fin]), "an infinite coordinate of the yardstick is not met"
    return float(((boxes.double() - ref).abs()[fin] / (K_DECODE * U * mag[fin])).max())


@pytest.mark.parametrize("shape,K", DECODE_SHAPES[2::3], ids=DECODE_IDS[2::3])
def test_decode_general_against_fp64(hip, shape, K):
    A = shape[-1]
    prob, anchors = R.decode_probs(shape, K, seed=A), R.random_anchors(A, seed=A)
    off = R.general_offsets(shape, seed=A)
    measured, count = measure_expf(hip, off)
    print(f"EXPF {DECODE_IDS[DECODE_SHAPES.index((shape, K))]} max error {measured:.4g} ulp over {count} arguments")
    conf, cls, boxes = run_decode(hip, prob, off, anchors)
    check_argmax(prob, conf, cls)

    def ref(**kw):
        if len(shape) == 1:
            return R.decode_boxes(off, anchors, torch.float64, **kw)
        return torch.stack([R.decode_boxes(o, anchors, torch.float64, **kw) for o in off])

    mag = decode_bound(off, anchors)
    ratio = decode_ratio(boxes, ref(), mag)
    tag = "decode/" + DECODE_IDS[DECODE_SHAPES.index((shape, K))]
    print(f"RATIO {tag} {ratio:.4g} (k = {K_DECODE}, EXPF_ULP = {EXPF_ULP})")
    _record(tag, dict(ratio=ratio, k=K_DECODE, expf_ulp_measured=measured, expf_ulp_bound=EXPF_ULP, arguments=count))
    assert measured <= EXPF_ULP, "the device expf is less accurate than the bound was derived for"
    assert ratio <= 1.0
    if A > 1:
        # teeth: the bound rejects a divisor of 8 in the centre offset and the anchor of the next row
        fin = torch.isfinite(ref())
        for kw in (dict(ten=8.0), dict(shift=1)):
            wrong = ref(**kw)
            assert float(((boxes.double() - wrong).abs()[fin] / (K_DECODE * U * mag[fin])).max()) > 1.0, kw


# ============================================================================================================== pipeline
def device_paths(box, prob, off, anchors, thr, pos):
    p, o, a = prob.cuda(), off.cuda(), anchors.cuda()
    yield "per-frame", box._multibox_detection_device(p, o, a, thr, pos).cpu()
    yield "batched", box.multibox_detection_batched(p, o, a, thr, pos).cpu()
    yield "public", box.multibox_detection(p, o, a, thr, pos).cpu()
    yield "public, one frame", torch.cat([box.multibox_detection(p[n:n + 1], o[n:n + 1], a, thr, pos).cpu()
                                          for n in range(p.shape[0])])


def test_pipeline_exact_inputs_equal_the_restatement(hip):
    """Anchors on the grid, offsets 0, probabilities on a 1/8 grid: large groups of equal confidence in every class,
    candidates in anchor order; every device path equals the restatement row for row."""
    from snn_for_object_detection_amd import box
    prob, off, anchors = R.pipeline_exact(3, 300, 4)
    for thr, pos in ((0.5, 0.25), (0.1, 0.009999999)):
        want = R.detect(prob, off, anchors, thr, pos)
        kept = int((want[..., 0] >= 0).sum())
        assert 30 < kept < 600
        for name, got in device_paths(box, prob, off, anchors, thr, pos):
            assert torch.equal(got, want), (name, thr, pos)


def test_pipeline_random_inputs_equal_the_restatement_on_the_device_boxes(hip):
    """Random anchors, offsets and softmax probabilities: the restatement's NMS and assembly run on the boxes the device
    decoded (their IoUs round, but every operation rounds the same way on both sides)."""
    from snn_for_object_detection_amd import box
    prob, off, anchors = R.pipeline_random(3, 700, 4)
    _, _, boxes = run_decode(hip, prob, off, anchors)
    for thr, pos in ((0.45, 0.3), (0.1, 0.009999999)):
        want = R.detect(prob, off, anchors, thr, pos, boxes=boxes)
        kept = int((want[..., 0] >= 0).sum())
        assert 30 < kept < 2000
        for name, got in device_paths(box, prob, off, anchors, thr, pos):
            assert torch.equal(got, want), (name, thr, pos)


@pytest.mark.parametrize("rows", [(17,), (0, 5, 150, 299), tuple(range(300))], ids=["one", "several", "all"])
def test_pipeline_nan_rows(hip, rows):
    """NaN probability rows in the middle frame of three: they come out as not-kept background rows in anchor order
    (class -1, confidence NaN, their decoded box), and every other row is what it is with a plain background row in
    their place."""
    from snn_for_object_detection_amd import box
    prob, off, anchors = R.pipeline_exact(3, 300, 4, seed=1)
    prob[1, list(rows)] = float("nan")
    clean = prob.clone()
    clean[1, list(rows)] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    want = R.detect(prob, off, anchors, 0.5, 0.25)
    want_clean = R.detect(clean, off, anchors, 0.5, 0.25)
    assert int(torch.isnan(want).sum()) == len(rows) and torch.equal(torch.nan_to_num(want, nan=1.0), want_clean)
    for (name, got), (_, got_clean) in zip(device_paths(box, prob, off, anchors, 0.5, 0.25),
                                           device_paths(box, clean, off, anchors, 0.5, 0.25)):
        assert not torch.isnan(got[..., 0]).any() and not torch.isnan(got[..., 2:]).any(), name
        assert same(got, want), name
        assert torch.equal(torch.nan_to_num(got, nan=1.0), got_clean), name
    # what the parent's key relied on, observed: where the device sort puts a NaN key
    key = torch.tensor([3.0, float("nan"), 1.0, 2.0], dtype=torch.float64).cuda()
    last = int(torch.argsort(key, stable=True)[-1]) == 1
    print(f"PREMISE device argsort places a NaN key last: {last}")
    _record("premise/device_argsort_nan_last", dict(observed=last))


# ============================================================================================================== refusals
HUGE_N, HUGE_A = 65536, 32768          # N * A = 2^31, above the documented 2^31 - 256


def _refusal_cases():
    """name, entry point, variants: for each, the valid call's arguments with one of them made unacceptable."""
    case = R.edge_case("half")
    A, C = case.A, case.C
    boxes, order, seg = dev(case.boxes, torch.float32), dev(case.order, torch.int32), dev(case.seg, torch.int32)
    skewed = torch.zeros(4 * A + 1, device="cuda")[1:]            # boxes misaligned by 4 bytes
    outs = lambda n: [Out(n * A, torch.int32), Out(n * C, torch.int32), Out(n * A, torch.uint8), Out(n * A, torch.int32)]
    # ---- snn_nms_sorted(boxes, order, seg, C, thr, kept, nkept, flag, rank, stream)
    o = outs(1)
    base = [boxes.data_ptr(), order.data_ptr(), seg.data_ptr(), C, 0.5] + [x.ptr for x in o] + [_st()]
    edits = {"null pointer": (1, None), "null output": (6, None), "misaligned boxes": (0, skewed.data_ptr()),
             "class count 0": (3, 0), "class count 65536": (3, 65536)}
    yield "snn_nms_sorted", base, edits, o
    # ---- snn_nms_sorted_batched(boxes, order, seg, N, A, C, thr, kept, nkept, flag, rank, stream)
    o = outs(1)
    base = [boxes.data_ptr(), order.data_ptr(), seg.data_ptr(), 1, A, C, 0.5] + [x.ptr for x in o] + [_st()]
    edits = {"null pointer": (2, None), "null output": (10, None), "misaligned boxes": (0, skewed.data_ptr()),
             "class count 0": (5, 0), "class count 65536": (5, 65536), "N * A above the limit": ((3, 4), (HUGE_N, HUGE_A))}
    yield "snn_nms_sorted_batched", base, edits, o
    # ---- snn_detect_assemble(conf, cls, boxes, nkept, flag, rank, N, A, C, pos, out, stream)
    args, _ = assemble_args(65, 3, R.PATTERNS[:3])
    out = Out(3 * 65 * 6, torch.float32)
    out_skew = Out(3 * 65 * 6, torch.float32, skew=1)
    skewed = torch.zeros(3 * 65 * 4 + 1, device="cuda")[1:]
    base = [a.data_ptr() for a in args] + [3, 65, 3, 0.25, out.ptr, _st()]
    edits = {"null pointer": (0, None), "null output": (10, None), "misaligned boxes": (2, skewed.data_ptr()),
             "misaligned out": (10, out_skew.ptr), "class count 0": (8, 0), "class count 65536": (8, 65536),
             "N * A above the limit": ((6, 7), (HUGE_N, HUGE_A))}
    yield "snn_detect_assemble", base, edits, [out, out_skew]
    # ---- snn_detect_decode(prob, offsets, anchors, A, K, conf, cls, boxes, stream): K = classes + background
    prob, off, anc = (torch.zeros(8, 3).cuda(), torch.zeros(8, 4).cuda(), R.dyadic_anchors(8).cuda())
    o = [Out(8, torch.float32), Out(8, torch.int32), Out(32, torch.float32)]
    base = [prob.data_ptr(), off.data_ptr(), anc.data_ptr(), 8, 3] + [x.ptr for x in o] + [_st()]
    edits = {"null pointer": (2, None), "null output": (7, None), "class count 0": (4, 1), "no column": (4, 0),
             "no anchor": (3, 0)}
    yield "snn_detect_decode", base, edits, o
    # ---- snn_detect_decode_batched(prob, offsets, anchors, N, A, K, conf, cls, boxes, stream)
    o = [Out(8, torch.float32), Out(8, torch.int32), Out(32, torch.float32)]
    base = [prob.data_ptr(), off.data_ptr(), anc.data_ptr(), 1, 8, 3] + [x.ptr for x in o] + [_st()]
    edits = {"null pointer": (0, None), "null output": (6, None), "class count 0": (5, 1),
             "N * A above the limit": ((3, 4), (HUGE_N, HUGE_A))}
    yield "snn_detect_decode_batched", base, edits, o
    del boxes, order, seg, prob, off, anc, args


def test_entry_points_refuse_bad_arguments(hip, hip_lib):
    """Null pointers, misaligned boxes, class counts 0 and 65536 and N * A above the documented limit: a nonzero return
    in front of any launch, snn_last_error names the entry point, and the outputs hold their fill.  (The decode entry
    points accept any K > 1 and any boxes alignment - test_decode_exact runs them misaligned.)"""
    seen = 0
    for name, base, edits, outs in _refusal_cases():
        fn = getattr(hip_lib, name)
        for what, (at, value) in edits.items():
            args = list(base)
            if isinstance(at, tuple):
                for i, v in zip(at, value):
                    args[i] = v
            else:
                args[at] = value
            rc = fn(*args)
            torch.cuda.synchronize()
            assert rc != 0, (name, what)
            assert name.encode() + b":" in hip_lib.snn_last_error(), (name, what, hip_lib.snn_last_error())
            assert all(o.untouched() for o in outs), (name, what)
            seen += 1
        assert fn(*base) == 0, name                                # the arguments the variants start from are accepted
        torch.cuda.synchronize()
        assert not all(o.untouched() for o in outs), name
    assert seen == 5 + 6 + 7 + 5 + 4
