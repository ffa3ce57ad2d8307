"""Hand-derived cases that pin tests/coco_map_ref.py (the fp64 restatement of COCO bbox mAP the device metric is checked
against).  Host only.  Each case states its derivation; ``CASES`` is reused by tests/test_gpu_map.py.

Notation: AP at one IoU threshold = mean over the 101 recall thresholds r of the interpolated precision q[r].  A lone
true positive has precision 1 / (1 + 2^-52), which is 1 - 2^-52: "1" below, to 1e-12.  N50 = 51 recall thresholds of
torch.linspace(0, 1, 101) are <= 0.5 (the table's entry 50 is 0.5 exactly).
"""
import numpy as np
import pytest
import torch

from tests.coco_map_ref import REC_THRESHOLDS, evaluate

N50 = 51
FAR = [0.875, 0.875, 0.9375, 0.9375]   # overlaps none of the ground-truth boxes below


def strip(k):
    """Ground-truth box k of a row of disjoint boxes (width 1/32, gaps of 1/32)."""
    return [k * 0.0625, 0.0, k * 0.0625 + 0.03125, 0.03125]


def det(c, s, b):
    return [float(c), float(s)] + list(b)


def gt(c, b):
    return [float(c)] + list(b)


def _cases():
    cases = {}
    # exact match: IoU 1 at every threshold, one TP, rc = [1], pr = [1] -> q = 1 everywhere, recall 1
    cases["exact"] = dict(images=[([det(0, 0.9, strip(3))], [gt(0, strip(3))])], C=1,
                          expect=dict(map=1.0, map_50=1.0, map_75=1.0, mar_1=1.0, mar_10=1.0, mar_100=1.0))
    # FP (0.9) above TP (0.8), one gt: tp = [0, 1], fp = [1, 1] -> rc = [0, 1], pr = [0, 1/2] -> after the running max
    # [1/2, 1/2]: q = 1/2 for every r; maxDet 1 keeps only the FP -> recall 0, maxDet 10 recall 1
    cases["fp_above_tp"] = dict(
        images=[([det(0, 0.9, FAR), det(0, 0.8, strip(0))], [gt(0, strip(0))])], C=1,
        expect=dict(map=0.5, map_50=0.5, map_75=0.5, mar_1=0.0, mar_10=1.0, mar_100=1.0))
    # IoU exactly 0.5: w, h = .5, .5 vs .5, .25 -> inter .125, union .25 + .125 - .125 = .25 -> 0.5 = the first threshold,
    # which matches (>=); fl32(0.55) and above do not.  map_50 = 1, map_75 = 0, map = (1 + 9 * 0) / 10
    cases["iou_half"] = dict(images=[([det(0, 0.7, [0, 0, .5, .5])], [gt(0, [0, 0, .5, .25])])], C=1,
                             expect=dict(map=0.1, map_50=1.0, map_75=0.0, mar_100=0.1))
    # equal-IoU tie: g0 = y [0, .75], g1 = y [.25, 1]; d0 = y [.25, .75] has IoU .5 / .75 = 2/3 with both (the same
    # expression, bit-equal) and takes the LATER row g1; d1 = y [.5, 1] has IoU 2/3 with g1 and .25 / 1 with g0, so at
    # t <= 0.65 it finds g1 taken and is a FP: tp = [1, 1], fp = [0, 1], rc = [.5, .5], pr = [1, .5] -> q = 1 for the
    # N50 thresholds r <= .5, else 0.  (Ties to the earlier row would give d0 -> g0, d1 -> g1: AP 1.)  At t >= 0.7 both
    # are FPs (2/3 < t): AP 0.  map = 4 * N50 / 101 / 10, recall .5 at the first four thresholds
    cases["tie_later_gt"] = dict(
        images=[([det(0, 0.9, [0, .25, 1, .75]), det(0, 0.8, [0, .5, 1, 1])],
                 [gt(0, [0, 0, 1, .75]), gt(0, [0, .25, 1, 1])])], C=1,
        expect=dict(map_50=N50 / 101, map=4 * N50 / 101 / 10, map_75=0.0, mar_100=4 * 0.5 / 10),
        masks=[[0b1111 | 1 << 31, 1 << 31]])
    # greedy order: d0 (0.9, IoU .625) takes the gt at t in {.5, .55, .6} although d1 (0.8, IoU 1) fits better: there
    # d1 is a FP after a TP -> rc = [1, 1], pr = [1, .5] -> AP 1.  At the 7 thresholds above .625 d0 is a FP and d1
    # takes the gt: rc = [0, 1], pr = [0, .5] -> AP .5.  map = (3 + 3.5) / 10; maxDet 1 keeps d0 only -> mar_1 = .3
    cases["greedy_order"] = dict(
        images=[([det(0, 0.9, [0, 0, 1, .625]), det(0, 0.8, [0, 0, 1, 1])], [gt(0, [0, 0, 1, 1])])], C=1,
        expect=dict(map=0.65, map_50=1.0, map_75=0.5, mar_1=0.3, mar_10=1.0, mar_100=1.0),
        masks=[[0b111 | 1 << 31, (0b1111111 << 3) | 1 << 31]])
    # truncation: 150 FPs by descending score, the exact box at rank 101 (index 100) is cut before matching: no TP
    dets = [det(0, 1 - k / 1000, strip(0) if k == 100 else FAR) for k in range(150)]
    cases["truncation"] = dict(images=[(dets, [gt(0, strip(0))])], C=1,
                               expect=dict(map=0.0, map_50=0.0, mar_1=0.0, mar_10=0.0, mar_100=0.0))
    # the same 150 with the exact box at rank 100 (index 99): kept, the 100th record -> rc reaches 1 at pr = 1/100
    dets = [det(0, 1 - k / 1000, strip(0) if k == 99 else FAR) for k in range(150)]
    cases["truncation_kept"] = dict(images=[(dets, [gt(0, strip(0))])], C=1,
                                    expect=dict(map=0.01, mar_10=0.0, mar_100=1.0))
    # 12 exact matches: maxDet m keeps min(m, 12) TPs of 12 gts -> recall 1/12, 10/12, 1 at every threshold
    cases["mar_ladder"] = dict(
        images=[([det(0, 0.9 - k / 64, strip(k)) for k in range(12)], [gt(0, strip(k)) for k in range(12)])], C=1,
        expect=dict(map=1.0, mar_1=1 / 12, mar_10=10 / 12, mar_100=1.0))
    # class 1 has a detection but no gt: npig = 0 -> left out of every mean, so class 0's exact match gives 1
    cases["class_without_gt"] = dict(
        images=[([det(0, 0.9, strip(1)), det(1, 0.95, strip(4))], [gt(0, strip(1))])], C=2,
        expect=dict(map=1.0, map_50=1.0, mar_1=1.0, mar_100=1.0))
    # no ground truth at all: no valid class -> -1 everywhere
    cases["no_gt"] = dict(images=[([det(0, 0.9, strip(1))], [])], C=2,
                          expect=dict(map=-1.0, map_50=-1.0, map_75=-1.0, mar_1=-1.0, mar_10=-1.0, mar_100=-1.0))
    # cross-image tie at score .5: image 0's FP stays before image 1's TP -> tp = [0, 1], fp = [1, 1], rc = [0, .5],
    # pr = [0, .5] -> [.5, .5]: q = .5 for the N50 thresholds <= .5
    cases["cross_image_tie"] = dict(
        images=[([det(0, 0.5, FAR)], [gt(0, strip(0))]), ([det(0, 0.5, strip(2))], [gt(0, strip(2))])], C=1,
        expect=dict(map=0.5 * N50 / 101, mar_1=0.5, mar_100=0.5))
    # ... and with the images swapped the TP comes first: rc = [.5, .5], pr = [1, .5] -> q = 1 for r <= .5
    cases["cross_image_tie_swapped"] = dict(
        images=[([det(0, 0.5, strip(2))], [gt(0, strip(2))]), ([det(0, 0.5, FAR)], [gt(0, strip(0))])], C=1,
        expect=dict(map=N50 / 101, mar_100=0.5))
    # an image with gt and no detection still counts: npig = 2, one TP -> rc = [.5], q = 1 for r <= .5, recall .5
    cases["gt_without_dets"] = dict(
        images=[([det(0, 0.9, strip(0))], [gt(0, strip(0))]), ([], [gt(0, strip(5))])], C=1,
        expect=dict(map=N50 / 101, mar_1=0.5, mar_100=0.5), npig=[2])
    # the two recall tables of rule 7: 20 gts, TP x 11, FP, TP (IoU 1)
    dets = [det(0, 0.99 - k / 100, strip(k)) for k in range(11)] + [det(0, 0.87, FAR), det(0, 0.86, strip(11))]
    two = [(dets, [gt(0, strip(k)) for k in range(20)])]
    cases["table_torch"] = dict(images=two, C=1, expect=dict(map=0.5902513328255903, map_50=0.5902513328255903))
    cases["table_numpy"] = dict(images=two, C=1, kw=dict(rec_thresholds=np.linspace(0.0, 1.0, 101).tolist()),
                                expect=dict(map=0.6001523229246001))
    return cases


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_hand_case(name):
    case = CASES[name]
    got, rec = evaluate(case["images"], case["C"], **case.get("kw", {}))
    for k, v in case["expect"].items():
        assert got[k] == pytest.approx(v, abs=1e-12), (k, got[k], v)
    if "masks" in case:
        for i, want in enumerate(case["masks"]):
            assert rec["mask"][i, 0, :len(want)].tolist() == want
    if "npig" in case:
        assert rec["npig"].tolist() == case["npig"]


def test_recall_table_is_torch_linspace():
    """0.55 is fl32(0.55) and entry 50 of the recall table is 0.5 exactly (what N50 relies on); numpy's table differs
    in 89 of the k/n, n <= 50, that land on a threshold (rule 7)."""
    from tests.coco_map_ref import IOU_THRESHOLDS
    assert IOU_THRESHOLDS[1] == 0.550000011920929
    assert REC_THRESHOLDS[50] == 0.5 and sum(r <= 0.5 for r in REC_THRESHOLDS) == N50
    rt, rn = np.array(REC_THRESHOLDS), np.linspace(0.0, 1.0, 101)
    diff = sum(int(np.searchsorted(rt, k / n) != np.searchsorted(rn, k / n)) for n in range(1, 51) for k in range(n + 1))
    assert diff == 89


def test_torch_linspace_default_matches_metric():
    pytest.importorskip("snn_for_object_detection_amd")
    from snn_for_object_detection_amd.metrics import MeanAveragePrecision
    from tests.coco_map_ref import IOU_THRESHOLDS
    m = MeanAveragePrecision(2)
    assert m.iou_thresholds == IOU_THRESHOLDS and m.rec_thresholds == REC_THRESHOLDS
    assert m.max_detection_thresholds == [1, 10, 100]
    assert torch.linspace(0.0, 1.0, 101).tolist() == REC_THRESHOLDS


def test_iou_matrix_is_the_scalar_form_bit_for_bit():
    """The vectorised IoU of the restatement against the scalar bbIou on random boxes, shared edges and disjoint pairs."""
    from tests.coco_map_ref import bb_iou, iou_matrix
    rng = np.random.default_rng(5)
    lo = rng.random((40, 2)) * 0.8
    boxes = np.concatenate([lo, lo + 0.01 + rng.random((40, 2)) * 0.3], axis=1).astype(np.float32)
    boxes[:8] = np.round(boxes[:8] * 8) / 8          # dyadic corners: shared edges and exact ratios
    m = iou_matrix(boxes[:20], boxes[20:])
    for a in range(20):
        for b in range(20):
            assert m[a, b] == bb_iou(boxes[a], boxes[20 + b])
    assert (m == 0).any() and (m > 0).any()

