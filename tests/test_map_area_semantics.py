"""Hand-derived cases that pin tests/coco_area_ref.py (the fp64 restatement of COCO mAP with area ranges, per-class
output and the box-size filter).  Host only.  ``AREA_CASES`` and ``area_set`` are reused by tests/test_gpu_map_areas.py.

Every case lives on a 256 x 256 image with boxes on the 1/256 grid, so every coordinate, side and pixel area is exact
in fp32.  ``px(x, y, w, h)`` is the box with its corner at pixel (x, y).  Notation as in tests/test_map_semantics.py: AP
at one IoU threshold = mean over the 101 recall thresholds of the interpolated precision; a lone true positive has
precision 1 - 2^-52 ("1", to 1e-12); the IoU thresholds are .5, .55, ..., .95; ranges small [0, 1024], medium
[1024, 9216], large [9216, 1e10] in pixel area, both ends inclusive.
"""
import functools

import numpy as np
import pytest

from tests.coco_area_ref import evaluate as evaluate_areas
from tests.coco_map_ref import evaluate
from tests.test_map_semantics import CASES, N50, det, gt

SIZE = (256, 256)


def px(x, y, w, h):
    return [x / 256, y / 256, (x + w) / 256, (y + h) / 256]


def _cases():
    cases = {}
    # edge: one 32 x 32 gt, area 1024 = 32^2 exactly: inside small (<= 1024) AND inside medium (>= 1024), outside large.
    # The exact detection (same area) is a TP in both: AP 1.  large has npig = 0: no valid class, -1.
    cases["edge"] = dict(
        images=[([det(0, 0.9, px(10, 10, 32, 32))], [gt(0, px(10, 10, 32, 32))])], C=1,
        expect=dict(map=1.0, map_small=1.0, mar_small=1.0, map_medium=1.0, mar_medium=1.0, map_large=-1.0, mar_large=-1.0),
        npig_area=[[1], [1], [0]])
    # in-range detection on an ignored gt.  A = 34 x 34 (area 1156: medium), B = 16 x 16 (256: small).  d0 = 30 x 30
    # (900: small) lies inside A: IoU 900 / 1156 = .7785, i.e. >= t for the six t <= .75; d1 = B exactly.
    #  small: A ignored, B counts (npig 1).  t <= .75: d0 finds no non-ignored row (IoU 0 with B), takes the ignored A
    #   and is ignored; d1 is a TP: tp = [0, 1], fp = [0, 0] -> pr = [0, 1] -> [1, 1]: AP 1.  t >= .8: d0 is unmatched
    #   and its own area 900 is inside small: a FP above the TP: pr = [0, .5] -> AP .5.  map_small = (6 + 4 * .5) / 10
    #   = .8, recall 1 at every t.  (Dropping ignored gts instead of ignoring the detection: d0 a FP at every t, .5.)
    #  medium: A counts, B ignored (npig 1).  t <= .75: d0 takes A, TP; d1 takes the ignored B and is ignored: AP 1,
    #   recall 1.  t >= .8: d0 unmatched with area 900 < 1024 outside medium: ignored; d1 ignored: no tp, no fp: AP 0,
    #   recall 0.  map_medium = mar_medium = .6.  large: no gt, -1.
    #  all: t <= .75 both TPs: AP 1; t >= .8 FP then TP of 2 gts: rc = [0, .5], pr = [0, .5] -> q = .5 for the N50
    #   thresholds <= .5: map = (6 + 4 * .5 * N50 / 101) / 10
    cases["ignored_gt"] = dict(
        images=[([det(0, 0.9, px(2, 2, 30, 30)), det(0, 0.8, px(100, 100, 16, 16))],
                 [gt(0, px(0, 0, 34, 34)), gt(0, px(100, 100, 16, 16))])], C=1,
        expect=dict(map_small=0.8, mar_small=1.0, map_medium=0.6, mar_medium=0.6, map_large=-1.0,
                    map=(6 + 4 * 0.5 * N50 / 101) / 10),
        npig_area=[[1], [1], [0]])
    # non-ignored beats better ignored.  d = 32 x 32 (1024: small and medium); A = 36 x 32 (1152: medium only) with IoU
    # 1024 / 1152 = .888..; B = 32 x 20 (640: small) with IoU 640 / 1024 = .625.
    #  small: B counts, A ignored.  t in {.5, .55, .6}: B qualifies, and d takes it although the ignored A overlaps
    #   better: TP, AP 1.  t in {.65 .. .85}: only the ignored A qualifies: d ignored, AP 0.  t in {.9, .95}: unmatched,
    #   area inside small: FP, AP 0.  map_small = .3 (taking the best row regardless of the flag would give 0)
    #  medium: A counts: TP for the eight t <= .85; above unmatched and inside medium: FP.  map_medium = .8
    cases["non_ignored_first"] = dict(
        images=[([det(0, 0.9, px(0, 0, 32, 32))], [gt(0, px(0, 0, 36, 32)), gt(0, px(0, 0, 32, 20))])], C=1,
        expect=dict(map_small=0.3, mar_small=0.3, map_medium=0.8, mar_medium=0.8, map_large=-1.0),
        preferred=1)
    # filter: gts 8 x 40, 16 x 16, 9 x 50 (disjoint); dets = the first two exactly.  Unfiltered: npig 3, two TPs:
    # rc = [1/3, 2/3], pr = [1, 1] -> q = 1 for the 67 thresholds .00 .. .66: map = 67 / 101
    three = [gt(0, px(0, 0, 8, 40)), gt(0, px(50, 0, 16, 16)), gt(0, px(100, 0, 9, 50))]
    two = [det(0, 0.9, px(0, 0, 8, 40)), det(0, 0.8, px(50, 0, 16, 16))]
    cases["unfiltered"] = dict(images=[(two, three)], C=1, expect=dict(map=67 / 101, mar_100=2 / 3), npig=[3], used=2)
    # ... with min_box_side = 10 the 8- and 9-wide rows go, ground truth and detection alike: one gt, one TP, map 1
    cases["min_side"] = dict(images=[(two, three)], C=1, kw=dict(min_box_side=10.0), expect=dict(map=1.0, mar_1=1.0),
                             npig=[1], used=1)
    # min_box_diag = 20 with min_box_side = 10: 12 x 12 passes the side test (12 >= 10) and fails the diagonal
    # (288 < 400); 12 x 16 is exactly on the diagonal (144 + 256 = 400, not < 400: kept); 10 x 30 exactly on the side
    # (10 < 10 is false: kept).  Detections are exact copies: two gts, two TPs, map 1
    rows = [px(0, 0, 12, 12), px(50, 0, 12, 16), px(100, 0, 10, 30)]
    diag = ([det(0, 0.9 - k / 10, b) for k, b in enumerate(rows)], [gt(0, b) for b in rows])
    cases["min_diag"] = dict(images=[diag], C=1, kw=dict(min_box_diag=20.0, min_box_side=10.0),
                             expect=dict(map=1.0, mar_100=1.0), npig=[2], used=2)
    # ... a hair past each boundary the row on it goes too
    cases["min_diag_past"] = dict(images=[diag], C=1, kw=dict(min_box_diag=20.0 + 2.0 ** -20, min_box_side=10.0),
                                  expect=dict(map=1.0), npig=[1], used=1)
    cases["min_side_past"] = dict(images=[diag], C=1, kw=dict(min_box_diag=20.0, min_box_side=10.0 + 2.0 ** -20),
                                  expect=dict(map=1.0), npig=[1], used=1)
    # per class: class 0 an exact match (AP 1, AR 1), class 1 a gt and a far detection (AP 0, AR 0), class 2 no gt (-1)
    cases["per_class"] = dict(
        images=[([det(0, 0.9, px(0, 0, 40, 40)), det(1, 0.8, px(200, 200, 20, 20)), det(2, 0.7, px(0, 0, 40, 40))],
                 [gt(0, px(0, 0, 40, 40)), gt(1, px(100, 0, 20, 20))])], C=3,
        expect=dict(map=0.5, mar_100=0.5), per_class=([1.0, 0.0, -1.0], [1.0, 0.0, -1.0]))
    return cases


AREA_CASES = _cases()


@functools.lru_cache(maxsize=None)
def case_reference(name):
    case = AREA_CASES[name]
    return evaluate_areas(case["images"], case["C"], SIZE, **case.get("kw", {}))


@pytest.mark.parametrize("name", sorted(AREA_CASES))
def test_restatement_hand_case(name):
    case = AREA_CASES[name]
    got, rec = case_reference(name)
    for k, v in case["expect"].items():
        assert got[k] == pytest.approx(v, abs=1e-12), (k, got[k], v)
    if "npig_area" in case:
        assert rec["npig_area"].tolist() == case["npig_area"]
    if "npig" in case:
        assert rec["npig"].tolist() == case["npig"]
    if "used" in case:
        assert int(((rec["mask"] >> 31) & 1).sum()) == case["used"]
    if "preferred" in case:
        assert rec["preferred"] == case["preferred"]
    if "per_class" in case:
        assert got["map_per_class"] == pytest.approx(case["per_class"][0], abs=1e-12)
        assert got["mar_per_class"] == pytest.approx(case["per_class"][1], abs=1e-12)


def test_ignored_gt_masks():
    """The masks behind the "ignored_gt" case, bit t per threshold: t = 0..5 are the thresholds <= .75."""
    _, rec = case_reference("ignored_gt")
    low, high = 0b0000111111, 0b1111000000
    assert rec["matched"][0, 0, 0, :2].tolist() == [low, low | high]       # small: d0 on the ignored A; d1 on B
    assert rec["ignored"][0, 0, 0, :2].tolist() == [low, 0]
    assert rec["matched"][0, 0, 1, :2].tolist() == [low, low | high]       # medium: d0 on A; d1 on the ignored B
    assert rec["ignored"][0, 0, 1, :2].tolist() == [high, low | high]      # d0 unmatched and too small above .75
    assert rec["matched"][0, 0, 2, :2].tolist() == [low, low | high]       # large: both gts ignored, matched as before,
    assert rec["ignored"][0, 0, 2, :2].tolist() == [low | high] * 2        # ignored through them or as out of range


def area_set(seed, n_images, C, image_size=(240, 304), max_gt=40, max_det=300):
    """Ground truth with sides from a few pixels to more than half the frame (so that all three ranges occur),
    overlapping freely, with interleaved padding rows; detections partly jittered ground truth, partly random, some of
    class -1; scores on a grid of 1/16 so that ties within and across images are common.  Sides are strictly positive."""
    rng = np.random.default_rng(seed)
    images = []
    for _ in range(n_images):
        ng = int(rng.integers(0, max_gt + 1))
        side = 0.02 + rng.random((ng, 2)) ** 2 * 0.6
        lo = rng.random((ng, 2)) * (1 - side)
        cls = rng.integers(0, C, (ng, 1))
        for k in range(ng // 3):             # a third are grown copies of the row before them (same corner and class):
            side[3 * k + 1] = np.minimum(side[3 * k] * (1.1 + rng.random(2) * 0.5), 1 - lo[3 * k])   # pairs that
            lo[3 * k + 1], cls[3 * k + 1] = lo[3 * k], cls[3 * k]      # overlap well and often straddle a range's end
        boxes = np.concatenate([lo, lo + side], axis=1)
        gts = np.concatenate([cls, boxes], axis=1)
        for _ in range(int(rng.integers(0, 4))):
            gts = np.insert(gts, int(rng.integers(0, len(gts) + 1)), [-1, .1, .1, .2, .2], axis=0)
        nd = int(rng.integers(0, max_det + 1))
        side = 0.02 + rng.random((nd, 2)) ** 2 * 0.6
        lo = rng.random((nd, 2)) * (1 - side)
        dets = np.zeros((nd, 6))
        dets[:, 2:] = np.concatenate([lo, lo + side], axis=1)
        dets[:, 0] = rng.integers(0, C, nd)
        if ng:
            jit = rng.random(nd) < 0.6
            src = rng.integers(0, ng, nd)
            dets[jit, 2:] = boxes[src[jit]] + rng.normal(0, 0.01, (int(jit.sum()), 4)) * (rng.random((int(jit.sum()), 1)) < 0.8)
            dets[jit, 0] = np.where(rng.random(int(jit.sum())) < 0.9, gts[gts[:, 0] >= 0][src[jit], 0], dets[jit, 0])
        dets[:, 4:] = np.maximum(dets[:, 4:], dets[:, 2:4] + 1 / 512)        # jitter never collapses a side
        dets[rng.random(nd) < 0.1, 0] = -1
        dets[:, 1] = rng.integers(0, 17, nd) / 16
        images.append((dets.astype(np.float32), gts.astype(np.float32)))
    return images


@functools.lru_cache(maxsize=None)
def area_set_reference(seed, n_images, C, min_box_diag=0.0, min_box_side=0.0):
    """``(images, summary, records)`` of one generated set: computed once, shared by the tests, never modified."""
    images = area_set(seed, n_images, C)
    return (images,) + evaluate_areas(images, C, (240, 304), min_box_diag=min_box_diag, min_box_side=min_box_side)


def test_all_equals_the_restatement_without_areas():
    """The "all" output of the restatement with areas is tests/coco_map_ref.evaluate: records bit for bit, summaries
    equal (the same arithmetic on the same records), on a generated set and on that restatement's own hand cases."""
    images, got, rec = area_set_reference(1, 6, 2)
    want, wrec = evaluate(images, 2)
    for k in want:
        assert got[k] == want[k], k
    assert np.array_equal(rec["score"], wrec["score"]) and np.array_equal(rec["mask"], wrec["mask"])
    assert np.array_equal(rec["npig"], wrec["npig"])
    for name, case in CASES.items():
        if "kw" in case:
            continue
        got, rec = evaluate_areas(case["images"], case["C"], SIZE)
        want, wrec = evaluate(case["images"], case["C"])
        assert all(got[k] == want[k] for k in want), name
        assert np.array_equal(rec["mask"], wrec["mask"]), name


def test_generated_set_exercises_every_rule():
    """What tests/test_gpu_map_areas.py relies on, asserted on the restatement alone: every range is valid for some
    class, detections are ignored both ways, and somewhere a non-ignored row beat a better-overlapping ignored one."""
    _, _, rec = area_set_reference(1, 6, 2)
    assert (rec["npig_area"] > 0).any(axis=1).all(), rec["npig_area"]
    assert rec["ignored_by_gt"] > 0 and rec["ignored_unmatched"] > 0 and rec["preferred"] > 0
