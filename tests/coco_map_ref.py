"""fp64 NumPy restatement of COCO bounding-box mAP as the reference computes it (torchmetrics MeanAveragePrecision,
iou_type "bbox", area range "all", no crowd boxes: COCOeval.evaluateImg / accumulate / summarize, pycocotools bbIou).

Written loop by loop after COCOeval, independently of the kernels in csrc/metrics.hip; a helper of the tests, not
collected.  Neither torchmetrics nor pycocotools is installed, so it is pinned by the hand-derived cases of
tests/test_map_semantics.py, not by a run of either.

An image is ``(dets, labels)``: ``dets[n, 6]`` rows (class, score, x1, y1, x2, y2), ``labels[g, 5]`` rows
(class, x1, y1, x2, y2); class < 0 is padding.  Images are given in evaluation order.
"""
import numpy as np
import torch

IOU_THRESHOLDS = torch.linspace(0.5, 0.95, 10).tolist()     # torchmetrics' defaults: fp32 linspace values
REC_THRESHOLDS = torch.linspace(0.0, 1.0, 101).tolist()
MAX_DETS = [1, 10, 100]


def bb_iou(d, g):
    """pycocotools bbIou of xyxy rows d, g whose xywh form is taken in fp32 (torchmetrics' box_convert)."""
    d = np.asarray(d, dtype=np.float32)
    g = np.asarray(g, dtype=np.float32)
    xd, yd, wd, hd = float(d[0]), float(d[1]), float(d[2] - d[0]), float(d[3] - d[1])
    xg, yg, wg, hg = float(g[0]), float(g[1]), float(g[2] - g[0]), float(g[3] - g[1])
    w = min(wd + xd, wg + xg) - max(xd, xg)
    if w <= 0:
        return 0.0
    h = min(hd + yd, hg + yg) - max(yd, yg)
    if h <= 0:
        return 0.0
    i = w * h
    return i / (wd * hd + wg * hg - i)


def iou_matrix(dt, gt):
    """``bb_iou`` for every (detection, ground truth) pair of xyxy arrays, elementwise fp64 (the same operations in the
    same order, so the same bits as the scalar form)."""
    d = np.asarray(dt, dtype=np.float32).reshape(-1, 4)
    g = np.asarray(gt, dtype=np.float32).reshape(-1, 4)
    xd, yd = d[:, 0].astype(np.float64)[:, None], d[:, 1].astype(np.float64)[:, None]
    wd, hd = (d[:, 2] - d[:, 0]).astype(np.float64)[:, None], (d[:, 3] - d[:, 1]).astype(np.float64)[:, None]
    xg, yg = g[:, 0].astype(np.float64)[None, :], g[:, 1].astype(np.float64)[None, :]
    wg, hg = (g[:, 2] - g[:, 0]).astype(np.float64)[None, :], (g[:, 3] - g[:, 1]).astype(np.float64)[None, :]
    w = np.minimum(wd + xd, wg + xg) - np.maximum(xd, xg)
    h = np.minimum(hd + yd, hg + yg) - np.maximum(yd, yg)
    i = w * h
    with np.errstate(divide="ignore", invalid="ignore"):
        o = i / (wd * hd + wg * hg - i)
    return np.where((w <= 0) | (h <= 0), 0.0, o)


def evaluate(images, num_classes, iou_thresholds=None, rec_thresholds=None, max_dets=None):
    """Returns ``(summary, records)``: summary = {map, map_50, map_75, mar_<m>} as Python floats (fp64), records =
    {"score": [I, C, S] float32 (-inf empty), "mask": [I, C, S] uint32 (bit 31 used, bit t matched at threshold t),
    "npig": [C] int64}."""
    iou_thrs = list(iou_thresholds or IOU_THRESHOLDS)
    rec_thrs = np.array(rec_thresholds or REC_THRESHOLDS, dtype=np.float64)
    max_dets = sorted(max_dets or MAX_DETS)
    S, T, R, M, C, I = max_dets[-1], len(iou_thrs), len(rec_thrs), len(max_dets), num_classes, len(images)
    score = np.full((I, C, S), -np.inf, dtype=np.float32)
    mask = np.zeros((I, C, S), dtype=np.uint32)
    npig = np.zeros(C, dtype=np.int64)
    for i, (dets, labels) in enumerate(images):
        dets = np.asarray(dets, dtype=np.float32).reshape(-1, 6)
        labels = np.asarray(labels, dtype=np.float32).reshape(-1, 5)
        for c in range(C):
            dt = dets[(dets[:, 0] >= 0) & (dets[:, 0].astype(np.int64) == c)]
            gt = labels[(labels[:, 0] >= 0) & (labels[:, 0].astype(np.int64) == c)]
            npig[c] += len(gt)
            dt = dt[np.argsort(-dt[:, 1], kind="mergesort")][:S]      # stable sort, truncation before matching
            for k in range(len(dt)):
                score[i, c, k] = dt[k, 1]
                mask[i, c, k] = np.uint32(1 << 31)
            ious = iou_matrix(dt[:, 2:], gt[:, 1:]).tolist()
            for t, thr in enumerate(iou_thrs):
                gtm = [False] * len(gt)
                for d in range(len(dt)):
                    iou, m = min(thr, 1 - 1e-10), -1
                    for g in range(len(gt)):
                        if gtm[g]:
                            continue
                        o = ious[d][g]
                        if o < iou:
                            continue
                        iou, m = o, g
                    if m >= 0:
                        gtm[m] = True
                        mask[i, c, d] |= np.uint32(1 << t)
    precision = -np.ones((T, R, C, M))
    recall = -np.ones((T, C, M))
    for c in range(C):
        if npig[c] == 0:
            continue
        for mi, md in enumerate(max_dets):
            sc = np.concatenate([score[i, c, :md] for i in range(I)])
            mk = np.concatenate([mask[i, c, :md] for i in range(I)])
            used = ((mk >> 31) & 1) == 1
            sc, mk = sc[used], mk[used]
            inds = np.argsort(-sc, kind="mergesort")
            mk = mk[inds]
            for t in range(T):
                hit = ((mk >> t) & 1) == 1
                tp = np.cumsum(hit).astype(dtype=float)
                fp = np.cumsum(~hit).astype(dtype=float)
                nd = len(tp)
                rc = tp / npig[c]
                pr = tp / (fp + tp + np.spacing(1))
                recall[t, c, mi] = rc[-1] if nd else 0
                pr = pr.tolist()
                for k in range(nd - 1, 0, -1):
                    if pr[k] > pr[k - 1]:
                        pr[k - 1] = pr[k]
                ids = np.searchsorted(rc, rec_thrs, side="left")
                q = np.zeros(R)
                for r, k in enumerate(ids):
                    if k < nd:
                        q[r] = pr[k]
                precision[t, :, c, mi] = q

    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    out = {"map": mean(precision[:, :, :, M - 1])}
    for key, thr in (("map_50", 0.5), ("map_75", 0.75)):
        t = [k for k, v in enumerate(iou_thrs) if v == thr]
        out[key] = mean(precision[t, :, :, M - 1]) if t else -1.0
    for mi, md in enumerate(max_dets):
        out[f"mar_{md}"] = mean(recall[:, :, mi])
    return out, {"score": score, "mask": mask, "npig": npig}
