"""Keeps the restatement of the detection tail (tests/detect_ref.py) honest, without a device: against the reference
goldens, against the host path and the oracle on tie-free inputs, and input builder by input builder - the crafted
inputs of tests/test_gpu_detect_kernels.py must reach the edges they are named after on the restatement alone.  The
NaN-row case runs the ordering helper of box.py (``detection_order``) on CPU tensors."""
import numpy as np
import pytest
import torch

from tests import detect_ref as R
from tests.test_gpu_detect import _npz, _rows_equal_up_to_ties

NMS_THR, POS_THR = 0.1, 0.009999999


def same(a, b):
    """torch.equal with NaN equal to NaN."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


# ------------------------------------------------------------------------------------- goldens, host path, oracle
@pytest.mark.parametrize("fixture,anchor_key", [("detect_nms.npz", None), ("detect_nms_mid.npz", "anchors")])
def test_detect_meets_the_reference_goldens(fixture, anchor_key):
    g = _npz(fixture)
    anchors = torch.from_numpy(g[anchor_key] if anchor_key else _npz("detect_anchors.npz")["anchors_tiny"])
    probs, offs, ref = (torch.from_numpy(g[k]) for k in ("probs", "offsets", "detections"))
    _rows_equal_up_to_ties(R.detect(probs, offs, anchors, NMS_THR, POS_THR), ref)


@pytest.mark.parametrize("A,K,thr,pos", [(300, 3, 0.1, POS_THR), (700, 5, 0.45, 0.5)])
def test_detect_equals_host_path_and_oracle_on_tie_free_inputs(A, K, thr, pos):
    from oracle import detect as OD
    from snn_for_object_detection_amd import box
    prob, offs, anchors = R.pipeline_random(2, A, K, seed=A)
    conf = prob.max(2).values
    for n in range(2):
        assert conf[n].unique().numel() == A, "the input has two equal confidences"
    got = R.detect(prob, offs, anchors, thr, pos)
    kept = int((got[..., 0] >= 0).sum())
    assert 10 < kept < 2 * A - 10, kept                                       # NMS keeps some and suppresses some
    assert torch.equal(got, box.multibox_detection(prob.clone(), offs.clone(), anchors, thr, pos))
    assert torch.equal(got, OD.multibox_detection(prob.clone(), offs.clone(), anchors, thr, pos))


# ------------------------------------------------------------------------------------------------ the NMS builders
def _ious(case, i, js):
    return R.iou_f32(case.boxes[case.order[i]], case.boxes[case.order[js]])


def test_grid_ious_are_the_stated_exact_values():
    f = np.float32
    assert R.iou_f32(R.cell(3), R.cell(4)) == 0 and R.iou_f32(R.cell(3), R.cell(35)) == 0      # neighbours touch
    assert R.iou_f32(R.cell(3), R.cell(3, dx=1)) == f(15) / f(17)
    assert R.iou_f32(R.cell(3), R.cell(3, shrink=1)) == f(15) / f(16)
    assert R.iou_f32(R.P_BOX, R.Q_BOX) == f(0.5)
    a, b, c = R._triple(2.0, 0.0)
    assert R.iou_f32(a, b) == f(3) / f(5) == R.iou_f32(b, c) and R.iou_f32(a, c) == f(1) / f(3)
    assert f(R.HALF_BELOW) < f(0.5) and f(R.HALF_BELOW) == f(0.5) - f(2.0 ** -25)
    # every crafted box but the degenerate ones lies on the grid inside [0, 8): exact differences, products and sums
    for case in R.nms_cases():
        if case.name == "degenerate":
            continue
        b = case.boxes.astype(np.float64) * 64
        assert np.all(b == np.round(b)) and b.min() >= 0 and b.max() <= 512, case.name
        assert np.all(b[:, 2] - b[:, 0] >= 1) and np.all(b[:, 3] - b[:, 1] >= 1), case.name


@pytest.mark.parametrize("name", R.NMS_CASE_NAMES)
def test_nms_builders_give_the_intended_counts(name):
    case = R.nms_case(name)
    kept, nkept, flag, rank = case.expected()
    assert list(nkept) == case.note["nkept"]
    assert sorted(case.order) == list(range(case.A)) and case.seg[-1] == case.A     # order is a permutation of the rows
    assert not np.array_equal(case.order, np.arange(case.A)) or case.A < 3         # ... and not the identity
    assert flag.sum() == nkept.sum() and not flag[case.order[:case.seg[0]]].any()   # no background row is kept
    for c in range(case.C):
        lo, n = int(case.seg[c]), int(nkept[c])
        assert list(rank[kept[lo:lo + n]]) == list(range(n))
        assert np.all(kept[lo + n:case.seg[c + 1]] == R.FILL)


def test_count_cases_alternate_through_the_chunk_boundaries():
    for n in (255, 256, 257, 511, 512, 513):
        case = R.count_case(n)
        _, nkept, flag, _ = case.expected()
        members = case.order[case.seg[1]:case.seg[2]]
        assert len(members) == n and nkept[1] == (n + 1) // 2 and n - nkept[1] == n // 2
        assert list(flag[members]) == [i % 2 == 0 for i in range(n)]            # so 255 | 256 and 511 | 512 differ


@pytest.mark.parametrize("m", [257, 513])
def test_tile_case_probes_meet_exactly_one_kept_box_in_an_earlier_chunk(m):
    case = R.tile_case(m)
    kept, nkept, flag, rank = case.expected()
    start, probes = case.note["start"], case.note["probes"]
    assert start % 256 == 0 and start >= m and probes == [t for t in (0, 255, 256, 257, 511, 512) if t < m]
    assert nkept[0] == m + 1 and list(kept[1:1 + m]) == list(case.order[1:1 + m])     # the m cells, in order
    first = 1                                                                          # (one background row in front)
    for i, t in enumerate(probes):
        at = first + start + i
        iou = _ious(case, at, np.arange(first, first + m))
        assert iou[t] == np.float32(15) / np.float32(16) and np.count_nonzero(iou) == 1   # kept box t and no other
        assert not flag[case.order[at]]
        assert (at - first) // 256 > t // 256                                          # t lies in an earlier chunk
    free = first + start + len(probes)
    assert np.count_nonzero(_ious(case, free, np.arange(first, first + m))) == 0
    assert flag[case.order[free]] and rank[case.order[free]] == m
    fillers = case.order[first + m:first + start]
    assert len(fillers) == start - m and not flag[fillers].any()


def test_greedy_case_is_not_transitive_across_mask_words_and_chunks():
    case = R.greedy_case()
    _, nkept, flag, _ = case.expected()
    assert sorted(v[1:] for v in case.note["triples"].values()) == [(63, 64), (127, 128), (191, 192), (254, 255), (261, 262)]
    thr = np.float32(case.thr)
    for a, b, c in case.note["triples"].values():
        ia, ib, ic = (case.order[x] for x in (a, b, c))
        assert flag[ia] and not flag[ib] and flag[ic]
        assert R.iou_f32(case.boxes[ia], case.boxes[ib]) > thr and R.iou_f32(case.boxes[ib], case.boxes[ic]) > thr
        others = np.array([x for x in range(case.A) if x not in (b, c)])
        assert np.all(_ious(case, c, others) <= thr)                # B alone would suppress C
        assert np.count_nonzero(_ious(case, b, others) > thr) == 1  # A alone suppresses B
    a, b, c = case.note["triples"][4]
    assert a < 256 <= b < c


def test_edge_and_degenerate_cases_say_what_their_names_say():
    for name, (thr, want) in R.EDGE_ROWS.items():
        case = R.edge_case(name)
        assert case.thr is thr
        kept, nkept, flag, _ = case.expected()
        assert list(nkept) == want
        ids = case.order[case.seg[4]:case.seg[5]]
        assert list(ids) == sorted(ids) and kept[case.seg[4]] == ids.min()       # equal confidences: the lowest anchor
    case = R.degenerate_case()
    _, nkept, flag, _ = case.expected()
    seg, o, b = case.seg, case.order, case.boxes
    assert np.isnan(R.iou_f32(b[o[seg[0]]], b[o[seg[0] + 1]]))                   # 0 / 0
    assert R.iou_f32(b[o[seg[1]]], b[o[seg[1] + 1]]) == 0
    assert R.iou_f32(b[o[seg[2] + 1]], b[o[seg[2] + 2]]) == 0 and np.signbit(R.iou_f32(b[o[seg[2] + 1]], b[o[seg[2] + 2]]))
    assert R.iou_f32(b[o[seg[3]]], b[o[seg[3] + 1]]) == 0 and np.isnan(R.iou_f32(b[o[seg[3]]], b[o[seg[3] + 2]]))
    assert np.isnan(R.iou_f32(b[o[seg[4]]], b[o[seg[4] + 1]])) and np.isnan(R.iou_f32(b[o[seg[5]]], b[o[seg[5] + 1]]))
    assert [list(flag[o[seg[c]:seg[c + 1]]]) for c in range(6)] == [
        [True, False], [True, True], [True, True, True], [True, True, False], [True, False, True], [True, False]]


def test_batched_frames_place_the_case_and_disable_only_the_malformed_classes():
    case = R.many_classes_case()
    A, C = case.A, case.C
    for pos in range(3):
        boxes, order, seg, bad = R.batched_frames(case, pos)
        assert bad == (300, 301, 302, 700, 701)
        assert seg[pos][301] < seg[pos][300] and seg[pos][302] > A and seg[pos][701] < 0
        kept, nkept, flag, rank = R.nms_sorted_batched(boxes, order, seg, 3, A, case.thr)
        want = np.array(case.note["nkept"])
        live = np.ones(C, bool)
        live[list(bad)] = False
        assert np.all(nkept[pos][~live] == 0) and np.array_equal(nkept[pos][live], want[live])
        good = case.expected()
        members = np.concatenate([case.order[case.seg[c]:case.seg[c + 1]] for c in bad])
        assert not flag[pos * A + members].any() and good[2][members].any()     # their members: kept before, not now
        rest = np.setdiff1d(np.arange(A), members)
        assert np.array_equal(flag[pos * A + rest], good[2][rest])               # every other class as without them
        # the segments that remain valid do not overlap (no two blocks write the same entries)
        ranges = sorted((lo, hi) for lo, hi in zip(seg[pos][:-1], seg[pos][1:]) if 0 <= lo <= hi <= A)
        assert all(x[1] <= y[0] for x, y in zip(ranges, ranges[1:]))
    small = R.edge_case("half")
    for pos in range(3):
        boxes, order, seg, bad = R.batched_frames(small, pos)
        _, nkept, flag, _ = R.nms_sorted_batched(boxes, order, seg, 3, small.A, small.thr)
        assert bad == () and list(nkept[pos]) == small.note["nkept"]
        assert np.array_equal(flag[pos * small.A:(pos + 1) * small.A], small.expected()[2])
        others = [n for n in range(3) if n != pos]                               # the neighbours are other inputs
        assert not np.array_equal(order[others[0] * small.A:][:small.A] - others[0] * small.A, small.order)
        assert not np.array_equal(boxes[others[1] * small.A:][:small.A], small.boxes, equal_nan=True)


# -------------------------------------------------------------------------------------------- the assemble builders
@pytest.mark.parametrize("A", R.ASSEMBLE_SIZES)
def test_assemble_builder_gives_the_pattern_and_a_permutation(A):
    for C, names in ((3, R.PATTERNS[:3]), (3, R.PATTERNS[3:]), (1, R.PATTERNS[:3]), (1024, R.PATTERNS[3:])):
        conf, cls, boxes, nkept, flag, rank = R.assemble_input(A, C, names)
        out = R.assemble(conf, cls, boxes, nkept, flag, rank, R.POS_THRESHOLD)
        for n, name in enumerate(names):
            assert np.array_equal(flag[n], R.pattern(name, A)), (name, A)
            assert sorted(R.assemble_positions(cls[n], nkept[n], flag[n], rank[n])) == list(range(A))
            assert not torch.isnan(out[n, :, 0]).any() and not torch.isnan(out[n, :, 2:]).any()
            k = int(flag[n].sum())
            assert torch.all(out[n, k:, 0] == -1)
            # kept rows come class by class; weak ones (confidence 1/8) keep their slot with class -1 and 7/8
            weak = flag[n] & (conf[n] < np.float32(0.25))
            pos = np.array(R.assemble_positions(cls[n], nkept[n], flag[n], rank[n]))
            assert torch.all(out[n, pos[weak], 0] == -1) and torch.all(out[n, pos[weak], 1] == 0.875)
            edge = flag[n] & (conf[n] == np.float32(0.25))
            assert torch.all(out[n, pos[edge], 0] == torch.from_numpy(cls[n][edge]).float())
            assert torch.all(out[n, pos[edge], 1] == 0.25)
            nan = np.isnan(conf[n])
            assert torch.isnan(out[n, pos[nan], 1]).all() and int(torch.isnan(out[n, :, 1]).sum()) == int(nan.sum())
            # a KEPT row with a NaN confidence is not weak: it keeps its class (a weak row would get -1)
            kept_nan = flag[n] & nan
            assert int(kept_nan.sum()) == (1 if k else 0)
            assert torch.equal(out[n, pos[kept_nan], 0], torch.from_numpy(cls[n][kept_nan]).float())
            assert np.all(cls[n][kept_nan] >= 0)
    conf, cls, _, _, flag, _ = R.assemble_input(513, 3, R.PATTERNS[:3])
    assert (flag[2] & (conf[2] < 0.25)).any() and (flag[2] & (conf[2] == 0.25)).any() and np.isnan(conf[2]).any()
    assert (~flag[2] & (cls[2] >= 0)).any() and (~flag[2] & (conf[2] < 0.25) & (cls[2] < 0)).any()


# ---------------------------------------------------------------------------------------------- the decode builders
@pytest.mark.parametrize("K", [2, 3, 9])
def test_argmax_table_rows(K):
    conf, cls = R.argmax_first(R.argmax_table(K))
    for i, (name, _, want_cls, want_conf) in enumerate(R.ARGMAX_ROWS):
        assert int(cls[i]) == want_cls, name
        got, want = conf[i:i + 1].view(torch.int32), torch.tensor([want_conf], dtype=torch.float32).view(torch.int32)
        assert torch.equal(got, want) or (np.isnan(want_conf) and torch.isnan(conf[i])), name      # the bits: -0 is -0
    if K >= 3:
        assert int(cls[-1]) == 1 and float(conf[-1]) == 0.5          # a NaN in front of the maximum is passed over


def test_decode_exact_inputs_are_exact_and_general_ones_are_not_degenerate():
    anchors = R.dyadic_anchors(257)
    off = R.exact_offsets((3, 257))
    _, _, b32 = R.decode(R.decode_probs((3, 257), 3), off, anchors, torch.float32)
    _, _, b64 = R.decode(R.decode_probs((3, 257), 3), off, anchors, torch.float64)
    # only the division by ten rounds: float32 is within one rounding of fp64, and nothing is subnormal
    assert float(((b32.double() - b64).abs() / b64.abs().clamp(min=1.0)).max()) <= 2.0 ** -22
    assert float(b32[b32 != 0].abs().min()) > 2.0 ** -100
    g = R.general_offsets((3, 257))
    _, _, big = R.decode(R.decode_probs((3, 257), 3), g, R.random_anchors(257), torch.float64)
    assert torch.isinf(big[0, 1, 0]) and torch.isinf(big[0, 2, 3]) and big[0, 3, 0] == big[0, 3, 2]


# ------------------------------------------------------------------------------------------------------ the NaN row
def parent_order(conf, cls, K):
    """The ordering expression both device paths held before ``detection_order``: the confidence enters the key as it
    is, so a NaN confidence gives a NaN key, which sorts behind every class."""
    key = (cls + 1).double() * 2.0 - conf.double()
    order = torch.argsort(key, stable=True).to(torch.int32)
    counts = (cls.unsqueeze(1) + 1 == torch.arange(K, dtype=torch.int32).unsqueeze(0)).sum(0)
    return order, torch.cumsum(counts, 0).to(torch.int32)


def tail_with(order_fn, prob, offs, anchors, thr, pos):
    """One frame through the restatement's decode, NMS and assembly with ``order_fn`` between them: the device paths'
    plumbing on CPU tensors."""
    conf, cls, boxes = R.decode(prob, offs, anchors)
    order, seg = order_fn(conf, cls, prob.shape[-1])
    _, nkept, flag, rank = R.nms_sorted(boxes.numpy(), order.numpy(), seg.numpy(), thr)
    if flag[(cls < 0).numpy()].any():
        return None, order, seg, cls, flag                      # a background row was kept: there is no row for it
    out = R.assemble(conf[None], cls[None], boxes[None], nkept, flag, np.where(flag, rank, 0), pos)[0]
    return out, order, seg, cls, flag


def nan_rows_case(rows, A=40, K=3, seed=3):
    prob, offs, anchors = R.pipeline_random(1, A, K, seed=seed)
    prob = prob[0].clone()
    prob[list(rows)] = float("nan")
    return prob, offs[0], anchors


@pytest.mark.parametrize("rows", [(17,), (0, 5, 39), tuple(range(40))], ids=["one", "several", "all"])
def test_nan_rows_stay_in_the_background_band(rows):
    from snn_for_object_detection_amd import box
    prob, offs, anchors = nan_rows_case(rows)
    want = R.detect(prob[None], offs[None], anchors, NMS_THR, POS_THR)[0]
    host = box.multibox_detection(prob[None].clone(), offs[None].clone(), anchors, NMS_THR, POS_THR)[0]
    assert same(want, host)                                     # the host path ignores such a row
    got, order, seg, cls, _ = tail_with(box.detection_order, prob, offs, anchors, NMS_THR, POS_THR)
    assert order.dtype == torch.int32 and seg.dtype == torch.int32
    bounds = [0] + [int(s) for s in seg]
    for k in range(3):                                          # every segment holds the rows of its class, all of them
        assert sorted(order[bounds[k]:bounds[k + 1]].tolist()) == torch.nonzero(cls == k - 1).flatten().tolist()
    assert same(got, want)
    # every clean row is as it is with a plain background row in the NaN row's place
    clean = prob.clone()
    clean[list(rows)] = torch.tensor([1.0, 0.0, 0.0])
    ref = R.detect(clean[None], offs[None], anchors, NMS_THR, POS_THR)[0]
    assert torch.equal(torch.isnan(want[:, 1]), ref[:, 1] == 1.0) and int(torch.isnan(want).sum()) == len(rows)
    assert torch.equal(want[:, [0, 2, 3, 4, 5]], ref[:, [0, 2, 3, 4, 5]])
    assert torch.equal(torch.nan_to_num(want[:, 1], nan=1.0), ref[:, 1])
    nan_out = torch.nonzero(torch.isnan(want[:, 1])).flatten()
    assert torch.all(want[nan_out, 0] == -1)
    _, _, boxes = R.decode(prob, offs, anchors)
    assert torch.equal(want[nan_out, 2:], boxes[list(rows)])    # not kept, in anchor order


def test_nan_row_breaks_the_parent_ordering():
    """The defect this helper replaces, pinned: with the confidence itself in the key, one NaN row moves every class
    segment one entry early - class 0 loses its best member and the NaN row is 'kept' in the last class."""
    from snn_for_object_detection_amd import box
    prob, offs, anchors = nan_rows_case((17,))
    want = R.detect(prob[None], offs[None], anchors, NMS_THR, POS_THR)[0]
    bad, order, seg, cls, flag = tail_with(parent_order, prob, offs, anchors, NMS_THR, POS_THR)
    assert int(order[-1]) == 17                                 # the NaN key sorts last, behind every class
    assert int(cls[order[int(seg[0]) - 1]]) == 0                # so the best of class 0 stands in the background segment
    assert int(seg[-1]) == 40 and int(seg[-2]) < 40             # and the NaN row is a candidate of the last class
    assert bad is None or not same(bad, want)                   # (bad is None: it was even kept)
    best0 = int(order[int(seg[0]) - 1])
    assert not flag[best0] and torch.any((want[:, 0] == 0) & (want[:, 1] == prob[best0].max()))
    # on inputs without NaN the two expressions give the same order and segments
    clean, offs, anchors = R.pipeline_random(1, 40, 3, seed=3)
    conf, cls, _ = R.decode(clean[0], offs[0], anchors)
    for a, b in zip(parent_order(conf, cls, 3), box.detection_order(conf, cls, 3)):
        assert torch.equal(a, b)
    # ... and on N frames the helper returns row ids, frame by frame what it returns for the frame alone
    prob2 = torch.stack((prob, clean[0]))
    conf2, cls2, _ = R.decode(prob2, torch.stack((offs[0], offs[0])), anchors)
    order2, seg2 = box.detection_order(conf2, cls2, 3)
    for n in range(2):
        o, s = box.detection_order(conf2[n], cls2[n], 3)
        assert torch.equal(order2[n], o + n * 40) and torch.equal(seg2[n], s)
