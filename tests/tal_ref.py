"""Reference of the task-aligned anchor assignment (DESIGN "Anchor assignment"; TEST INFRASTRUCTURE ONLY, nothing here
imports the package) and the table of cases ``tests/test_tal_host.py`` and ``tests/test_gpu_tal.py`` run.

``tal_ref``  restates the definition in float64: the per-pair quantities (decoded box, probability, overlap, metric,
anchor IoU) as numpy expressions over the anchors of one label row, every DECISION - the top-k of a row, the owner of an
anchor several rows selected, the anchor a fall-back claims - in a plain loop.  Next to the integer assignment it
records the margin of every decision:

  ``topk``      (row, relative gap between the k-th and the (k+1)-th metric of the row), rows with more candidates than k;
  ``conflict``  (anchor, relative gap between the two largest overlaps among the rows that selected it);
  ``fallback``  (row, relative gap between the two largest anchor IoUs among the anchors still unassigned).

A gap of exactly 0 is a tie, decided by the index.  The fp32 paths reproduce the integer assignment exactly when every
margin is far above fp32 rounding; ``MARGIN`` = 1e-4 is what the committed cases keep outside the duplication cases
(asserted by ``test_tal_host.py``), and a metric that takes part in a top-k decision also stays above ``TINY``, far from
the fp32 underflow of ``u^beta``.

All coordinates lie on a binary grid (1/64, the large case 1/256): centres, sizes and the candidate test are exact in
fp32, and the offsets 10 * dxy / wh round once - the bounds of ``check_offsets`` are those of
``tests/test_gpu_targets_fp64.py`` for ``snn_roi_assign``.
"""
import math
from typing import Callable, List, NamedTuple, Optional

import numpy as np
import torch

from tests import targets_ref as TR

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
EXP_CLAMP = math.log(1000.0 / 16.0)
IOU_EPS = 1e-7
MARGIN = 1e-4
TINY = 1e-30
GRID = 64


class TalRecord(NamedTuple):
    amap: List[int]                  # [A] label row or -1
    part: List[bool]                 # [N] the row takes part
    n_cand: List[int]                # [N] candidates of the row (0 for rows that take no part)
    selected: List[List[int]]        # [N] the anchors the row selected, in selection order
    topk: list                       # (row, margin, k-th metric, (k+1)-th metric)
    conflict: list                   # (anchor, margin, rows that selected it in row order)
    fallback: list                   # (row, margin, claimed anchor or -1)
    zero_fill: int                   # selected candidates with metric 0
    u: np.ndarray                    # [A, N] overlaps (0 for rows that take no part)
    s: np.ndarray                    # [A, N] probabilities


def _rel_gap(a, b):
    return 0.0 if a == b else (a - b) / abs(a)


def decode64(anchors, bb):
    """offset_inverse with the exponent argument replaced by the clamp where it is not <= it (NaN included) -> corners"""
    with np.errstate(all="ignore"):
        cxa, cya = (anchors[:, 0] + anchors[:, 2]) / 2, (anchors[:, 1] + anchors[:, 3]) / 2
        wa, ha = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
        ew, eh = bb[:, 2] / 5, bb[:, 3] / 5
        w = np.exp(np.where(ew <= EXP_CLAMP, ew, EXP_CLAMP)) * wa
        h = np.exp(np.where(eh <= EXP_CLAMP, eh, EXP_CLAMP)) * ha
        cx, cy = bb[:, 0] * wa / 10 + cxa, bb[:, 1] * ha / 10 + cya
        return np.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], axis=1)


def _positive(v):
    return np.where(v > 0, v, 0.0)           # NaN > 0 is False


def tal_ref(anchors, label, cls, bb, topk, alpha, beta) -> TalRecord:
    """One sample: ``anchors[A,4]``, ``label[N,5]``, ``cls[A,C]``, ``bb[A,4]`` (their fp32 values, taken exactly)."""
    anchors, label, cls, bb = (np.asarray(t.detach().to("cpu", F64).numpy()) for t in (anchors, label, cls, bb))
    A, N, C = anchors.shape[0], label.shape[0], cls.shape[1]
    p = decode64(anchors, bb)
    acx, acy = (anchors[:, 0] + anchors[:, 2]) / 2, (anchors[:, 1] + anchors[:, 3]) / 2
    with np.errstate(all="ignore"):
        e = np.exp(cls - np.max(cls, axis=1, keepdims=True))      # a NaN or +inf logit makes the whole row NaN
        prob = e / e.sum(axis=1, keepdims=True)
    part, n_cand = [], []
    u, s, t = np.zeros((A, N)), np.zeros((A, N)), np.zeros((A, N))
    cand, iou = np.zeros((A, N), dtype=bool), np.zeros((A, N))
    for j in range(N):
        c, x1, y1, x2, y2 = (float(v) for v in label[j])
        ok = c >= 0 and c + 1 < C and x2 > x1 and y2 > y1
        part.append(bool(ok))
        if not ok:
            n_cand.append(0)
            continue
        with np.errstate(all="ignore"):
            s[:, j] = _positive(prob[:, int(c) + 1])
            ap, ag = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]), (x2 - x1) * (y2 - y1)
            iw = np.maximum(np.minimum(p[:, 2], x2) - np.maximum(p[:, 0], x1), 0)
            ih = np.maximum(np.minimum(p[:, 3], y2) - np.maximum(p[:, 1], y1), 0)
            inter = iw * ih
            u[:, j] = _positive(inter / ((ap + ag - inter) + IOU_EPS))
            t[:, j] = _positive(s[:, j] ** alpha * u[:, j] ** beta)
            # box_iou of the anchor itself, for the fall-back
            a1 = (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
            ow = np.maximum(np.minimum(anchors[:, 2], x2) - np.maximum(anchors[:, 0], x1), 0)
            oh = np.maximum(np.minimum(anchors[:, 3], y2) - np.maximum(anchors[:, 1], y1), 0)
            iou[:, j] = (ow * oh) / (a1 + ag - ow * oh)
        cand[:, j] = (acx > x1) & (acx < x2) & (acy > y1) & (acy < y2)
        n_cand.append(int(cand[:, j].sum()))
    # ---- every row selects up to topk of its candidates: descending metric, the lower anchor on ties
    selected, topk_rec, zero_fill = [[] for _ in range(N)], [], 0
    for j in range(N):
        if not part[j]:
            continue
        order = []
        for a in range(A):
            if cand[a, j]:
                order.append((-t[a, j], a))
        order.sort()
        selected[j] = [a for _, a in order[:topk]]
        zero_fill += sum(1 for v, _ in order[:topk] if v == 0)
        if len(order) > topk:
            tk, tk1 = -order[topk - 1][0], -order[topk][0]
            topk_rec.append((j, _rel_gap(tk, tk1), tk, tk1))
    # ---- an anchor selected by several rows goes to the row of largest overlap, the lower row on ties
    amap, conflict_rec = [-1] * A, []
    for a in range(A):
        rows = [j for j in range(N) if a in selected[j]]
        if not rows:
            continue
        best = rows[0]
        for j in rows[1:]:
            if u[a, j] > u[a, best]:
                best = j
        amap[a] = best
        if len(rows) > 1:
            us = sorted((u[a, j] for j in rows), reverse=True)
            conflict_rec.append((a, _rel_gap(us[0], us[1]), rows))
    # ---- in row order, a row left without an anchor claims the unassigned anchor of highest IoU (first maximum)
    fallback_rec = []
    for j in range(N):
        if not part[j] or j in amap:
            continue
        best, best_v, second_v = -1, -math.inf, -math.inf
        for a in range(A):
            if amap[a] >= 0:
                continue
            v = iou[a, j]
            if v > best_v:
                best, best_v, second_v = a, v, best_v
            elif v > second_v:
                second_v = v
        if best >= 0:
            amap[best] = j
        fallback_rec.append((j, _rel_gap(best_v, second_v) if second_v > -math.inf else 1.0, best))
    return TalRecord(amap, part, n_cand, selected, topk_rec, conflict_rec, fallback_rec, zero_fill, u, s)


class TalTargets(NamedTuple):
    rows: torch.Tensor            # [B, A] int64, -1 = background
    classes: torch.Tensor         # [B, A] int64
    masks: torch.Tensor           # [B, A, 4] fp32
    offsets64: torch.Tensor       # [B, A, 4] fp64, from the integer assignment
    records: List[TalRecord]


def tal_targets_ref(anchors, labels, cls, bb, topk, alpha, beta) -> TalTargets:
    """A batch: ``labels[B,N,5]``, ``cls[B,A,C]``, ``bb[B,A,4]`` -> the targets formed from the integer assignment."""
    anchors = anchors.detach().to("cpu", F32)
    A = anchors.shape[0]
    rows_l, cls_l, mask_l, off_l, recs = [], [], [], [], []
    for b in range(labels.shape[0]):
        label = labels[b].detach().to("cpu", F32)
        rec = tal_ref(anchors, label, cls[b], bb[b], topk, alpha, beta)
        amap = torch.tensor(rec.amap, dtype=torch.long)
        assigned = amap >= 0
        mask = assigned.float().unsqueeze(-1).repeat(1, 4)
        classes = torch.zeros(A, dtype=torch.long)
        boxes = torch.zeros((A, 4), dtype=F32)
        classes[assigned] = label[amap[assigned], 0].long() + 1
        boxes[assigned] = label[amap[assigned], 1:]
        off_l.append(TR._offset_boxes(anchors.to(F64), boxes.to(F64), TR.EPS32) * mask.to(F64))
        rows_l.append(amap)
        cls_l.append(classes)
        mask_l.append(mask)
        recs.append(rec)
    return TalTargets(torch.stack(rows_l), torch.stack(cls_l), torch.stack(mask_l), torch.stack(off_l), recs)


def check_offsets(off, ref: TalTargets):
    """The bounds of tests/test_gpu_targets_fp64.py::check_roi against the fp64 offsets: columns 0 / 1 round once, in
    the division (u |r|); columns 2 / 3, 5 * logf(eps + tw / aw), within u (10 + 3 |r|).  -> the two ratios"""
    err = (off.double() - ref.offsets64).abs()
    r64 = ref.offsets64.abs()
    xy = float((err[..., :2] / (U * r64[..., :2] + 1e-300)).max())
    wh = float((err[..., 2:] / (U * (10.0 + 3.0 * r64[..., 2:]))).max())
    assert xy <= 1.0, f"offsets 0 / 1: max |d - r64| / (u |r64|) = {xy:.3g}"
    assert wh <= 1.0, f"offsets 2 / 3: max |d - r64| / (u (10 + 3 |r64|)) = {wh:.3g}"
    return xy, wh


def margins(rec: TalRecord):
    """Every decision margin of one sample and the number of top-k decisions taken on a metric inside (0, TINY)."""
    ms = [m for _, m, _, _ in rec.topk] + [m for _, m, _ in rec.conflict] + [m for _, m, _ in rec.fallback]
    tiny = sum(1 for _, _, tk, tk1 in rec.topk if 0 < tk < TINY or 0 < tk1 < TINY)
    return ms, tiny


# ------------------------------------------------------------------------------------------------------ cases
class TalCase(NamedTuple):
    id: str
    anchors: torch.Tensor                 # [A, 4] fp32
    labels: torch.Tensor                  # [B, N, 5] fp32
    cls: torch.Tensor                     # [B, A, C] fp32
    bb: torch.Tensor                      # [B, A, 4] fp32
    topk: int = 10
    alpha: float = 1.0
    beta: float = 6.0
    check: Optional[Callable] = None      # check(records): asserts on the reference's record that the edge is reached
    duplication: bool = False             # holds exact ties on purpose


PADDING_ROW = [-1.0] * 5


def _b(*xs):
    return [x / GRID for x in xs]


def make_anchors():
    """Two maps, 6 x 8 pixels with three and 3 x 4 pixels with two anchors per pixel: A = 168, centres and half sides on
    the 1/64 grid.  Map 0 has its centres at x = 4, 12, .. 60 and y = 5, 15, .. 55, map 1 at x = 8, 24, 40, 56 and
    y = 10, 30, 50 (grid steps)."""
    out = []
    for r in range(6):
        for c in range(8):
            for hw, hh in ((5, 5), (7, 4), (4, 7)):
                cx, cy = 8 * c + 4, 10 * r + 5
                out.append(_b(cx - hw, cy - hh, cx + hw, cy + hh))
    for r in range(3):
        for c in range(4):
            for hw, hh in ((10, 10), (14, 7)):
                cx, cy = 16 * c + 8, 20 * r + 10
                out.append(_b(cx - hw, cy - hh, cx + hw, cy + hh))
    return torch.tensor(out, dtype=F32)


def random_labels(N, C, g, min_side=14, max_side=40):
    boxes = TR.grid_boxes(N, g, max_side=max_side)
    wh = boxes[:, 2:] - boxes[:, :2]
    grow = torch.clamp(min_side / GRID - wh, min=0)
    boxes[:, 2:] = boxes[:, 2:] + grow                       # may leave [0, 1]: nothing depends on that
    cls = torch.randint(0, C - 1, (N, 1), generator=g).float()
    return torch.cat([cls, boxes], dim=1)


def predictions(B, A, C, g, logit_scale=2.0, offset_scale=1.0):
    return torch.randn(B, A, C, generator=g) * logit_scale, torch.randn(B, A, 4, generator=g) * offset_scale


def _random_case(N, C, B, topk, seed, pad=0):
    g = torch.Generator().manual_seed(seed)
    anchors = make_anchors()
    labels = torch.stack([random_labels(N, C, g) for _ in range(B)])
    for b in range(1, B):
        if pad:
            labels[b, N - min(pad, N - 1):] = torch.tensor(PADDING_ROW)
    cls, bb = predictions(B, anchors.shape[0], C, g)
    return TalCase(f"rand_N{N}_C{C}_B{B}_k{topk}", anchors, labels, cls, bb, topk)


def _anchor_at(anchors, cx, cy):
    """the anchors of map 0 centred on grid point (cx, cy)"""
    c = torch.tensor(_b(cx, cy))
    ctr = (anchors[:, :2] + anchors[:, 2:]) / 2
    return [int(i) for i in torch.arange(anchors.shape[0])[(ctr == c).all(dim=1)]]


def tal_cases() -> List[TalCase]:
    cases = [
        _random_case(1, 2, 1, 1, 11),
        _random_case(2, 3, 1, 3, 12),
        _random_case(3, 5, 2, 10, 213, pad=1),
        _random_case(5, 3, 3, 3, 14, pad=2),
        _random_case(8, 4, 2, 10, 15, pad=3),
        _random_case(8, 2, 1, 1, 16),
        _random_case(4, 5, 3, 1, 17),
    ]
    anchors = make_anchors()
    A = anchors.shape[0]

    # ---- a row with fewer candidates than topk: the box holds the one centre (20, 25) - three anchors of map 0
    g = torch.Generator().manual_seed(21)
    cls, bb = predictions(1, A, 3, g)
    lab = torch.tensor([[[1.0] + _b(17, 21, 23, 29), [0.0] + _b(30, 8, 62, 52)]])

    def check_few(recs):
        assert recs[0].n_cand[0] == 3 and len(recs[0].selected[0]) == 3 and recs[0].n_cand[1] > 10
    cases.append(TalCase("fewer_candidates_than_topk", anchors, lab, cls, bb, 10, check=check_few))

    # ---- a row containing no anchor centre (x in 13 .. 18 lies between the centres 12 and 20 of map 0, 8 and 24 of
    # map 1): nothing is selected, the fall-back claims the anchor of highest IoU
    g = torch.Generator().manual_seed(22)
    cls, bb = predictions(1, A, 3, g)
    lab = torch.tensor([[[0.0] + _b(4, 6, 40, 44), [1.0] + _b(13, 7, 18, 24)]])

    def check_no_centre(recs):
        r = recs[0]
        assert r.n_cand[1] == 0 and r.selected[1] == [] and [f[0] for f in r.fallback] == [1] and r.amap.count(1) == 1
    cases.append(TalCase("no_centre_fallback", anchors, lab, cls, bb, 3, check=check_no_centre))

    # ---- two overlapping objects that share selected anchors
    g = torch.Generator().manual_seed(23)
    cls, bb = predictions(1, A, 3, g)
    lab = torch.tensor([[[0.0] + _b(6, 6, 44, 42), [1.0] + _b(14, 12, 52, 50)]])

    def check_conflict(recs):
        assert len(recs[0].conflict) >= 2
    cases.append(TalCase("conflict", anchors, lab, cls, bb, 10, check=check_conflict))

    # ---- an all-padding sample, a zero-area row and a row of a class the logits have no column for, in one batch
    g = torch.Generator().manual_seed(24)
    C = 3
    cls, bb = predictions(3, A, C, g)
    s0 = random_labels(4, C, g)
    s1 = torch.tensor([PADDING_ROW] * 4)
    s2 = random_labels(4, C, g)
    s2[1, 1:] = torch.tensor(_b(10, 12, 10, 30))          # zero area
    s2[2, 0] = float(C - 1)                               # class + 1 == C
    s2[3, 0] = 7.0                                        # far outside

    def check_excluded(recs):
        assert recs[1].part == [False] * 4 and recs[1].amap == [-1] * A
        assert recs[2].part == [True, False, False, False] and set(recs[2].amap) == {-1, 0}
    cases.append(TalCase("padding_zero_area_bad_class", anchors, torch.stack([s0, s1, s2]), cls, bb, 3,
                         check=check_excluded))

    # ---- NaN / inf logits and offsets on anchors inside the boxes, and an offset past the exponent clamp.  Row 1 holds
    # the three anchors at (20, 25) only: its list is filled with metric-0 candidates.
    g = torch.Generator().manual_seed(25)
    cls, bb = predictions(1, A, 3, g)
    lab = torch.tensor([[[0.0] + _b(30, 8, 62, 52), [1.0] + _b(17, 21, 23, 29)]])
    inside0 = _anchor_at(anchors, 44, 25) + _anchor_at(anchors, 52, 35)
    a20 = _anchor_at(anchors, 20, 25)
    cls[0, inside0[0], 1] = float("nan")
    cls[0, inside0[1], 2] = float("inf")
    cls[0, inside0[2], 0] = float("-inf")
    bb[0, inside0[3], 0] = float("nan")
    bb[0, inside0[4], 2] = float("inf")
    bb[0, inside0[5], 3] = float("-inf")
    bb[0, a20[0], 1] = float("nan")
    cls[0, a20[1], :] = float("nan")
    past = _anchor_at(anchors, 36, 25)[0]
    bb[0, past, 2] = 40.0                                  # 40 / 5 = 8 > log(62.5)

    def check_nonfinite(recs, bb=bb):
        r = recs[0]
        assert r.zero_fill >= 2 and a20[0] in r.selected[1] and a20[1] in r.selected[1]
        assert all(r.u[a, 0] == 0 or r.s[a, 0] == 0 for a in (inside0[0], inside0[1], inside0[3]))
        w = float(anchors[past, 2] - anchors[past, 0])
        p = decode64(anchors.double().numpy(), bb[0].double().numpy())[past]
        assert abs((p[2] - p[0]) - 62.5 * w) < 1e-9
    cases.append(TalCase("nonfinite_and_clamp", anchors, lab, cls, bb, 10, check=check_nonfinite))

    # ---- real ties, by exact duplication.  Two identical anchor rows with identical predictions and the largest metric
    # of the row: with topk = 1 the lower anchor wins.
    g = torch.Generator().manual_seed(26)
    dup = anchors.clone()
    lo, hi = _anchor_at(dup, 28, 25)[0], _anchor_at(dup, 36, 35)[1]
    dup[hi] = dup[lo]
    cls, bb = predictions(1, A, 3, g)
    cls[0, lo] = torch.tensor([-4.0, 6.0, -4.0])
    bb[0, lo] = 0.0
    cls[0, hi], bb[0, hi] = cls[0, lo], bb[0, lo]
    lab = torch.cat([torch.tensor([0.0]), dup[lo]]).reshape(1, 1, 5)

    def check_dup_anchor(recs):
        r = recs[0]
        assert lo < hi and r.selected[0] == [lo] and r.amap[lo] == 0 and r.amap[hi] == -1
        assert r.topk[0][1] == 0.0 and r.topk[0][2] > 0.9
    cases.append(TalCase("dup_anchors", dup, lab, cls, bb, 1, check=check_dup_anchor, duplication=True))

    # ---- two identical label rows: every conflict ties and goes to row 0; row 1 is left to the fall-back
    g = torch.Generator().manual_seed(27)
    cls, bb = predictions(1, A, 3, g)
    row = [1.0] + _b(9, 7, 41, 39)
    lab = torch.tensor([[row, row]])

    def check_dup_rows(recs):
        r = recs[0]
        assert r.selected[0] == r.selected[1] and len(r.conflict) == 3 and all(m == 0.0 for _, m, _ in r.conflict)
        assert all(r.amap[a] == 0 for a in r.selected[0]) and [f[0] for f in r.fallback] == [1]
        assert r.amap.count(1) == 1
    cases.append(TalCase("dup_rows", anchors, lab, cls, bb, 3, check=check_dup_rows, duplication=True))
    return cases


def gen1_case() -> TalCase:
    """The GEN1 anchor count (A = 13 545 = 4515 centres x 3 shapes, on a 1/256 grid) with N = 16 and B = 2: the
    grid-stride loops of all three kernels run several times."""
    A, N, C = 13_545, 16, 3
    g = torch.Generator().manual_seed(31)
    ctr = torch.randint(8, 249, (A // 3, 2), generator=g)
    half = torch.tensor([[6, 6], [9, 4], [4, 9]])
    lo = (ctr[:, None, :] - half[None]).reshape(A, 2)
    hi = (ctr[:, None, :] + half[None]).reshape(A, 2)
    anchors = torch.cat([lo, hi], dim=1).float() / 256
    labels = []
    for _ in range(2):
        w = torch.randint(10, 90, (N, 2), generator=g)
        p = torch.randint(0, 256 - 90, (N, 2), generator=g)
        cls = torch.randint(0, C - 1, (N, 1), generator=g).float()
        labels.append(torch.cat([cls, p.float() / 256, (p + w).float() / 256], dim=1))
    labels = torch.stack(labels)
    labels[1, 12:] = torch.tensor(PADDING_ROW)
    cls, bb = predictions(2, A, C, g)
    return TalCase("gen1_A13545_N16", anchors, labels, cls, bb, 10)


CACHE = 14_336     # anchors whose metrics k_tal_select keeps in LDS between its rounds (kTalCache, csrc/targets.hip)


def beyond_cache_case() -> TalCase:
    """A = 15 000, a little above the 14 336 metrics the select kernel keeps in LDS: anchors behind the cache are
    recomputed in every round.  topk = 3, N = 4, one sample; ``check`` asserts that anchors on both sides of the cache
    boundary are selected, and that a row's list mixes them."""
    A, N, C = 15_000, 4, 3
    g = torch.Generator().manual_seed(41)
    ctr = torch.randint(8, 249, (A // 3, 2), generator=g)
    half = torch.tensor([[6, 6], [9, 4], [4, 9]])
    lo = (ctr[:, None, :] - half[None]).reshape(A, 2)
    hi = (ctr[:, None, :] + half[None]).reshape(A, 2)
    anchors = torch.cat([lo, hi], dim=1).float() / 256
    w = torch.randint(30, 90, (N, 2), generator=g)
    p = torch.randint(0, 256 - 90, (N, 2), generator=g)
    cls = torch.randint(0, C - 1, (N, 1), generator=g).float()
    labels = torch.cat([cls, p.float() / 256, (p + w).float() / 256], dim=1).unsqueeze(0)
    logits, bb = predictions(1, A, C, g)
    # the best candidates would mostly lie in front of the cache boundary (14 336 of 15 000 anchors): raise the class
    # logit of the anchors behind it, so that every row's list holds some of them
    logits[0, CACHE:, 1:] += 3.0

    def check(recs):
        sel = [a for row in recs[0].selected for a in row]
        assert any(a >= CACHE for a in sel) and any(a < CACHE for a in sel), sorted(sel)
        assert any(min(row) < CACHE <= max(row) for row in recs[0].selected if row), recs[0].selected
        assert all(len(row) == 3 for row in recs[0].selected)
    return TalCase("beyond_cache_A15000", anchors, labels, logits, bb, 3, check=check)


def steps_labels(cs: TalCase, K: int, t0: int, seed: int):
    """Six-column labels and ``steps[K,B]`` built from a five-column case: every real row gets a timestep out of K + 1
    distinct ones - the last of them is in no slot ("rows of other timesteps") - and the last slot of sample 0 is left
    empty.  -> (labels6[B,N,6], steps[K,B] int32, per slot the five-column rows of that slot with every other row
    replaced by padding, so that row indices stay those of the sample)"""
    g = torch.Generator().manual_seed(seed)
    B, N, _ = cs.labels.shape
    times = torch.tensor([3, 5, 8, 9][:K + 1]) + t0
    pick = torch.randint(0, K + 1, (B, N), generator=g)
    ts = times[pick].float()
    real = cs.labels[:, :, 0] >= 0
    ts = torch.where(real, ts, torch.full_like(ts, -1.0))
    labels6 = torch.cat([ts.unsqueeze(-1), cs.labels], dim=2)
    steps = (times[:K] - t0).to(torch.int32).unsqueeze(1).repeat(1, B)
    steps[K - 1, 0] = -1
    slots = []
    for k in range(K):
        for b in range(B):
            own = real[b] & (pick[b] == k) & (steps[k, b] >= 0)
            slots.append(torch.where(own.unsqueeze(-1), cs.labels[b], torch.tensor(PADDING_ROW)))
    return labels6, steps, torch.stack(slots).reshape(K, B, N, 5)
