"""fp64 NumPy restatement of COCO bounding-box mAP with the area ranges small / medium / large, per-class AP / AR and the
box-size filter, as metrics.py states them (rules 1-6, options A-C): COCOeval.evaluateImg / accumulate / summarize for
bbox, no crowd boxes, on pixel areas.

Written loop by loop after COCOeval - the stable sort of the ground truth by its ignore flag, the ``break`` on reaching
ignored rows once a non-ignored row is matched - and independently of the kernels in csrc/metrics.hip; a helper of the
tests, not collected.  Neither torchmetrics nor pycocotools is installed, so it is pinned by the hand-derived cases of
tests/test_map_area_semantics.py and by its "all" output, which must equal tests/coco_map_ref.evaluate, not by a run of
either.  "all" has no area test (real COCOeval applies [0, 1e10] to it, which matters only for boxes with a negative
side).

An image is ``(dets, labels)`` as in tests/coco_map_ref.py; ``image_size = (H, W)`` in pixels.
"""
import numpy as np

from tests.coco_map_ref import IOU_THRESHOLDS, MAX_DETS, REC_THRESHOLDS, iou_matrix

RANGES = (("small", 0.0, 32.0 ** 2), ("medium", 32.0 ** 2, 96.0 ** 2), ("large", 96.0 ** 2, 1e10))


def pixel_sides(boxes, image_size):
    """(wp, hp) of xyxy rows: the fp32 side times the image size, in fp64."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    H, W = float(image_size[0]), float(image_size[1])
    return (b[:, 2] - b[:, 0]).astype(np.float64) * W, (b[:, 3] - b[:, 1]).astype(np.float64) * H


def size_filter(rows, first, image_size, min_box_diag, min_box_side):
    """The rows that the size filter keeps; ``first`` is the column of x1.  A limit is active only when > 0."""
    wp, hp = pixel_sides(rows[:, first:first + 4], image_size)
    drop = np.zeros(len(rows), dtype=bool)
    if min_box_diag > 0:
        drop |= wp * wp + hp * hp < float(min_box_diag) * float(min_box_diag)
    if min_box_side > 0:
        drop |= (wp < float(min_box_side)) | (hp < float(min_box_side))
    return rows[~drop]


def evaluate(images, num_classes, image_size, iou_thresholds=None, rec_thresholds=None, max_dets=None, min_box_diag=0.0,
             min_box_side=0.0):
    """Returns ``(summary, records)``.  summary: map, map_50, map_75, mar_<m>, map_<range>, mar_<range> as Python floats
    and ``map_per_class`` / ``mar_per_class`` as lists (largest maxDet, "all", -1 without ground truth).  records:
    score [I, C, S] float32, mask [I, C, S] uint32 (bit 31 used, bit t matched: "all"), matched / ignored [I, C, 3, S]
    uint32 (bit t), npig [C], npig_area [3, C], and three counts of what the set exercises: ``ignored_by_gt`` (detection,
    threshold, range) matched to an ignored row, ``ignored_unmatched`` unmatched and out of range, ``preferred`` images
    in which a non-ignored row was taken although a free ignored row overlapped better."""
    iou_thrs = list(iou_thresholds or IOU_THRESHOLDS)
    rec_thrs = np.array(rec_thresholds or REC_THRESHOLDS, dtype=np.float64)
    max_dets = sorted(max_dets or MAX_DETS)
    S, T, R, M, C, I = max_dets[-1], len(iou_thrs), len(rec_thrs), len(max_dets), num_classes, len(images)
    NA = 1 + len(RANGES)                                     # area index 0 is "all"
    score = np.full((I, C, S), -np.inf, dtype=np.float32)
    used = np.zeros((I, C, S), dtype=bool)
    dtm = np.zeros((NA, I, C, S, T), dtype=bool)
    dtig = np.zeros((NA, I, C, S, T), dtype=bool)
    npig = np.zeros((NA, C), dtype=np.int64)
    stats = {"ignored_by_gt": 0, "ignored_unmatched": 0, "preferred": 0}
    for i, (dets, labels) in enumerate(images):
        dets = np.asarray(dets, dtype=np.float32).reshape(-1, 6)
        labels = np.asarray(labels, dtype=np.float32).reshape(-1, 5)
        dets = size_filter(dets[dets[:, 0] >= 0], 2, image_size, min_box_diag, min_box_side)
        labels = size_filter(labels[labels[:, 0] >= 0], 1, image_size, min_box_diag, min_box_side)
        preferred = False
        for c in range(C):
            dt = dets[dets[:, 0].astype(np.int64) == c]
            gt = labels[labels[:, 0].astype(np.int64) == c]
            dt = dt[np.argsort(-dt[:, 1], kind="mergesort")][:S]      # stable sort, truncation before matching
            score[i, c, :len(dt)] = dt[:, 1]
            used[i, c, :len(dt)] = True
            ious = iou_matrix(dt[:, 2:], gt[:, 1:]).tolist()
            wd, hd = pixel_sides(dt[:, 2:], image_size)
            wg, hg = pixel_sides(gt[:, 1:], image_size)
            d_area, g_area = wd * hd, wg * hg
            for a in range(NA):
                if a == 0:
                    g_ig, d_out = [0] * len(gt), [False] * len(dt)
                else:
                    _, lo, hi = RANGES[a - 1]
                    g_ig = [int(v < lo or v > hi) for v in g_area]
                    d_out = [bool(v < lo or v > hi) for v in d_area]
                npig[a, c] += len(gt) - sum(g_ig)
                gtind = np.argsort(g_ig, kind="mergesort").tolist()   # non-ignored rows first, row order kept
                for t, thr in enumerate(iou_thrs):
                    gtm = [False] * len(gt)
                    for d in range(len(dt)):
                        iou, m = min(thr, 1 - 1e-10), -1
                        for g in gtind:
                            if gtm[g]:
                                continue
                            if m > -1 and g_ig[m] == 0 and g_ig[g] == 1:
                                break                                   # a non-ignored match: stop at the ignored rows
                            if ious[d][g] < iou:
                                continue
                            iou, m = ious[d][g], g
                        if m == -1:
                            if d_out[d]:
                                dtig[a, i, c, d, t] = True
                                stats["ignored_unmatched"] += 1
                            continue
                        if g_ig[m]:
                            stats["ignored_by_gt"] += 1
                        elif any(g_ig[g] and not gtm[g] and ious[d][g] > iou for g in range(len(gt))):
                            preferred = True
                        gtm[m] = True
                        dtm[a, i, c, d, t] = True
                        dtig[a, i, c, d, t] = bool(g_ig[m])
        stats["preferred"] += int(preferred)
    precision = -np.ones((T, R, C, NA, M))
    recall = -np.ones((T, C, NA, M))
    for a in range(NA):
        for c in range(C):
            if npig[a, c] == 0:
                continue
            for mi, md in enumerate(max_dets):
                keep = np.concatenate([used[i, c, :md] for i in range(I)])
                sc = np.concatenate([score[i, c, :md] for i in range(I)])[keep]
                inds = np.argsort(-sc, kind="mergesort")
                m_ = np.concatenate([dtm[a, i, c, :md] for i in range(I)])[keep][inds]      # [records, T]
                ig = np.concatenate([dtig[a, i, c, :md] for i in range(I)])[keep][inds]
                for t in range(T):
                    tp = np.cumsum(m_[:, t] & ~ig[:, t]).astype(dtype=float)
                    fp = np.cumsum(~m_[:, t] & ~ig[:, t]).astype(dtype=float)
                    nd = len(tp)
                    rc = tp / npig[a, c]
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, c, a, mi] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for k in range(nd - 1, 0, -1):
                        if pr[k] > pr[k - 1]:
                            pr[k - 1] = pr[k]
                    ids = np.searchsorted(rc, rec_thrs, side="left")
                    q = np.zeros(R)
                    for r, k in enumerate(ids):
                        if k < nd:
                            q[r] = pr[k]
                    precision[t, :, c, a, mi] = q

    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    out = {"map": mean(precision[:, :, :, 0, M - 1])}
    for key, thr in (("map_50", 0.5), ("map_75", 0.75)):
        t = [k for k, v in enumerate(iou_thrs) if v == thr]
        out[key] = mean(precision[t, :, :, 0, M - 1]) if t else -1.0
    for mi, md in enumerate(max_dets):
        out[f"mar_{md}"] = mean(recall[:, :, 0, mi])
    for a, (name, _, _) in enumerate(RANGES, start=1):
        out[f"map_{name}"] = mean(precision[:, :, :, a, M - 1])
        out[f"mar_{name}"] = mean(recall[:, :, a, M - 1])
    out["map_per_class"] = [mean(precision[:, :, c, 0, M - 1]) for c in range(C)]
    out["mar_per_class"] = [mean(recall[:, c, 0, M - 1]) for c in range(C)]

    def bits(x):                                             # [..., S, T] bool -> [..., S] uint32, bit t
        return (x.astype(np.uint32) << np.arange(T, dtype=np.uint32)).sum(axis=-1, dtype=np.uint32)

    records = {"score": score, "mask": bits(dtm[0]) | (used.astype(np.uint32) << np.uint32(31)),
               "matched": np.moveaxis(bits(dtm[1:]), 0, 2), "ignored": np.moveaxis(bits(dtig[1:]), 0, 2),
               "npig": npig[0], "npig_area": npig[1:], **stats}
    return out, records
