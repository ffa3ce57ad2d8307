"""References for the training-target kernels of csrc/targets.hip and csrc/det_loss.hip (TEST INFRASTRUCTURE ONLY;
nothing here imports the package).

``roi_assign_ref``  restates the anchor <-> ground-truth assignment of the reference (utils/roi.py:18-109 with
utils/box.py:31-69) statement by statement in torch float32 on the host.  float32 and not float64 on purpose: the result
is an integer decision taken on fp32 IoUs (the kernel is compiled with contraction off to reproduce exactly those), and an
fp64 IoU would decide ties differently from the operation under test.  Next to the fp32 offsets it returns fp64 offsets
formed from the integer assignment - the high-precision reference of the offset VALUES - and, per greedy round, the flat
argmax index with the (box_idx, anc_idx) derived from it, so that a test can assert that an edge was reached.

``det_loss_ref``  is the loss of models/soda.py:259-281 and its gradient in float64, closed form, no autograd.

``roi_cases``  builds the table of assignment cases both test files run (coordinates on a grid of 1/64 inside [0, 1]:
equal geometry gives bit-equal IoUs, so ties are real ties).
"""
from typing import Callable, List, NamedTuple, Optional, Tuple

import torch

F32, F64 = torch.float32, torch.float64
EPS32 = float(torch.tensor(1e-6, dtype=F32))      # offset_boxes' eps as the fp32 tensor arithmetic sees it


# ------------------------------------------------------------------------------------------------------ RoI
class RoiRef(NamedTuple):
    classes: torch.Tensor        # [B, A] int64
    masks: torch.Tensor          # [B, A, 4] fp32
    offsets: torch.Tensor        # [B, A, 4] fp32, the reference's own arithmetic
    offsets64: torch.Tensor      # [B, A, 4] fp64, from the integer assignment
    amap: torch.Tensor           # [B, A] int64, -1 = unassigned
    rounds: List[List[Tuple[int, int, int]]]   # per sample, per greedy round: (flat index, box_idx, anc_idx)


def _corner_to_center(b):
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), dim=-1)


def box_iou_ref(boxes1, boxes2):
    """utils/box.py:49-59, same operations in the same order."""
    areas1 = torch.prod(boxes1[:, 2:] - boxes1[:, :2], dim=1)
    areas2 = torch.prod(boxes2[:, 2:] - boxes2[:, :2], dim=1)
    up_left = torch.max(boxes1[:, None, :2], boxes2[:, :2])
    low_right = torch.min(boxes1[:, None, 2:], boxes2[:, 2:])
    inters = torch.clamp(low_right - up_left, min=0)
    inter_areas = torch.prod(inters, dim=2)
    union_areas = areas1[:, None] + areas2 - inter_areas
    return inter_areas / union_areas


def _offset_boxes(anchors, assigned_bb, eps):
    """utils/box.py:62-69 in the dtype of its operands."""
    c_anc, c_bb = _corner_to_center(anchors), _corner_to_center(assigned_bb)
    xy = 10 * (c_bb[:, :2] - c_anc[:, :2]) / c_anc[:, 2:]
    wh = 5 * torch.log(eps + c_bb[:, 2:] / c_anc[:, 2:])
    return torch.cat([xy, wh], dim=1)


def _assign(ground_truth, anchors, thr):
    """utils/roi.py:79-109; also returns the record of the greedy rounds."""
    num_anchors, num_gt = anchors.shape[0], ground_truth.shape[0]
    jaccard = box_iou_ref(anchors, ground_truth)
    amap = torch.full((num_anchors,), -1, dtype=torch.long)
    max_ious, indices = torch.max(jaccard, dim=1)
    keep = max_ious >= thr
    amap[keep] = indices[keep]
    rounds = []
    for _ in range(num_gt):
        max_idx = torch.argmax(jaccard)
        box_idx = (max_idx % num_gt).long()
        anc_idx = (max_idx / num_gt).long()          # int64 / int: torch's true division in float32, then truncation
        amap[anc_idx] = box_idx                      # IndexError when the quotient rounds up to num_anchors
        jaccard[:, box_idx] = -1.0
        jaccard[anc_idx, :] = -1.0
        rounds.append((int(max_idx), int(box_idx), int(anc_idx)))
    return amap, rounds


def roi_assign_ref(anchors: torch.Tensor, labels: torch.Tensor, thr: float) -> RoiRef:
    anchors = anchors.detach().to("cpu", F32).contiguous()
    labels = labels.detach().to("cpu", F32).contiguous()
    A = anchors.shape[0]
    cls_l, mask_l, off_l, off64_l, amap_l, rounds_l = [], [], [], [], [], []
    for label in labels:
        amap, rounds = _assign(label[:, 1:], anchors, thr)
        assigned = amap >= 0
        mask = assigned.float().unsqueeze(-1).repeat(1, 4)
        classes = torch.zeros(A, dtype=torch.long)
        bb = torch.zeros((A, 4), dtype=F32)
        rows = amap[assigned]
        classes[assigned] = label[rows, 0].long() + 1
        bb[assigned] = label[rows, 1:]
        off_l.append(_offset_boxes(anchors, bb, 1e-6) * mask)
        off64_l.append(_offset_boxes(anchors.to(F64), bb.to(F64), EPS32) * mask.to(F64))
        cls_l.append(classes)
        mask_l.append(mask)
        amap_l.append(amap)
        rounds_l.append(rounds)
    return RoiRef(torch.stack(cls_l), torch.stack(mask_l), torch.stack(off_l), torch.stack(off64_l),
                  torch.stack(amap_l), rounds_l)


# ------------------------------------------------------------------------------------------------------ RoI cases
GRID = 64


class RoiCase(NamedTuple):
    id: str
    anchors: torch.Tensor                 # [A, 4] fp32
    labels: torch.Tensor                  # [B, N, 5] fp32
    thr: float = 0.5
    check: Optional[Callable] = None      # check(ref: RoiRef): asserts on the reference that the edge is reached


def grid_boxes(n, g, lo=0, hi=GRID, max_side=GRID):
    """n corner boxes with corners on the 1/64 grid inside [lo, hi] / 64, every side at least one grid step."""
    span = hi - lo
    w = torch.randint(1, min(max_side, span) + 1, (n, 2), generator=g)
    p = (torch.rand(n, 2, generator=g) * (span - w + 1).float()).floor().long().clamp(max=span) + lo
    p = torch.minimum(p, hi - w)
    return torch.cat([p, p + w], dim=1).float() / GRID


def populated_labels(anchors, N, g, classes=3):
    """Half of the rows repeat an anchor (IoU exactly 1, ties where the anchor set has copies), the others are boxes of
    their own."""
    A = anchors.shape[0]
    boxes = grid_boxes(N, g, max_side=24)
    take = torch.randint(0, A, (N,), generator=g)
    use = torch.arange(N) % 2 == 0
    boxes[use] = anchors[take[use]]
    cls = torch.randint(0, classes, (N, 1), generator=g).float()
    return torch.cat([cls, boxes], dim=1)


PADDING_ROW = [-1.0] * 5


def _anchor_set(A, seed):
    g = torch.Generator().manual_seed(seed)
    return grid_boxes(A, g, max_side=24)


def _claimed(ref, b=0):
    return [r[2] for r in ref.rounds[b]]


def _b(*xs):
    return [x / GRID for x in xs]


def batch_case():
    """B = 4 over one anchor set (A = 1025: two 1024-strides, one anchor in the second): a populated sample, one that is
    all padding, one with a duplicated row, a zero-area box and a box that overlaps nothing, and one partly padded."""
    A, N = 1025, 7
    g = torch.Generator().manual_seed(404)
    anchors = grid_boxes(A, g, hi=GRID // 2, max_side=20)
    s0 = populated_labels(anchors, N, g)
    s1 = torch.tensor([PADDING_ROW] * N)
    s2 = populated_labels(anchors, N, g)
    s2[1] = s2[0]
    s2[1, 0] = (s2[0, 0] + 1) % 3
    s2[3, 1:] = torch.tensor(_b(10, 12, 10, 30))          # zero area
    s2[5, 1:] = torch.tensor(_b(40, 40, 60, 64))          # right half: no anchor reaches it
    s3 = populated_labels(anchors, N, g)
    s3[3:] = torch.tensor(PADDING_ROW)
    return RoiCase("batch4", anchors, torch.stack([s0, s1, s2, s3]))


def large_case():
    """A * N > 2^24 (a 72 MB IoU workspace).  With N = 32 a flat index a * 32 + 31 above 2^24 is odd, (float)idx rounds
    to the neighbour with the even significand, (a + 1) * 32, and the fp32 quotient is a + 1: label row 31 repeats an
    anchor a >= 2^19 whose geometry no other anchor has, so one round's argmax is exactly that index.  a + 1 < A: the
    reference never forms anc_idx >= A.  (N = 128 at A = 140 000 reaches the same edge but costs the host reference 128
    argmax passes over 18 M IoUs, ~5 s; 32 passes take ~1 s.)"""
    A, N = 560_000, 32
    g = torch.Generator().manual_seed(2024)
    anchors = grid_boxes(A, g, max_side=20)
    labels = populated_labels(anchors, N, g)
    a_star = 540_000
    big = torch.tensor(_b(1, 2, 62, 63))                   # larger than any other anchor: unique geometry
    anchors[a_star] = big
    labels[N - 1, 1:] = big

    def check(ref):
        assert all(r[2] < A for r in ref.rounds[0])
        odd = [(f, bx, an) for f, bx, an in ref.rounds[0] if an != f // N]
        assert odd and (a_star * N + N - 1, N - 1, a_star + 1) in odd, odd
    return RoiCase("large_AN_gt_2p24", anchors, labels.unsqueeze(0), 0.5, check)


def roi_cases(large=True) -> List[RoiCase]:
    cases = []
    # ---- A below / at / above the wave (64) and the block (1024), a partly filled last wave; N = 1 ... 33
    for A in (1, 3, 63, 64, 65, 1000, 1023, 1024, 1025, 2500):
        anchors = _anchor_set(A, 1000 + A)
        for N in (1, 2, 7, 33):
            g = torch.Generator().manual_seed(A * 100 + N)
            cases.append(RoiCase(f"A{A}_N{N}", anchors, populated_labels(anchors, N, g).unsqueeze(0)))
    # ---- more rows than anchors: once every row and column is discarded argmax of a constant is flat index 0
    anchors = _anchor_set(3, 7)
    g = torch.Generator().manual_seed(35)

    def check_n_gt_a(ref):
        assert [r[0] for r in ref.rounds[0][3:]] == [0, 0], ref.rounds
    cases.append(RoiCase("A3_N5", anchors, populated_labels(anchors, 5, g).unsqueeze(0), 0.5, check_n_gt_a))
    # ---- all padding: every round ties at IoU 0, anchors 0, 1, 2, ... are claimed with mask 1 and class 0
    anchors = _anchor_set(1500, 8)

    def check_padding(ref):
        assert _claimed(ref) == list(range(5))
        assert bool((ref.classes == 0).all()) and int(ref.masks[0, :, 0].sum()) == 5
        assert bool((ref.masks[0, :5] == 1).all())
    cases.append(RoiCase("all_padding", anchors, torch.tensor([[PADDING_ROW] * 5]), 0.5, check_padding))
    # ---- IoU exactly on the threshold: anchors 0 and 1 are (0,0,1,1), the box (0,0,1,1/2) has IoU 0.5 with both.  The
    # greedy phase claims anchor 0; anchor 1 is a positive only through best >= thr.  One grid step smaller: IoU 31/64.
    anchors = torch.cat([torch.tensor([_b(0, 0, 64, 64)] * 2), _anchor_set(70, 9) * 0.25 + 0.75])

    def check_on_thr(ref):
        assert ref.amap[0, :3].tolist() == [0, 0, -1] and _claimed(ref) == [0]
    cases.append(RoiCase("iou_on_threshold", anchors, torch.tensor([[[1.0] + _b(0, 0, 64, 32)]]), 0.5, check_on_thr))

    def check_below_thr(ref):
        assert ref.amap[0, :3].tolist() == [0, -1, -1] and _claimed(ref) == [0]
    cases.append(RoiCase("iou_below_threshold", anchors, torch.tensor([[[1.0] + _b(0, 0, 64, 31)]]), 0.5, check_below_thr))
    # ---- a duplicated ground-truth row: the per-anchor maximum takes the first row, the second row the next-best anchor
    anchors = _anchor_set(300, 10) * 0.5 + 0.5                      # all inside [1/2, 1]
    anchors[10] = torch.tensor(_b(0, 0, 20, 20))
    anchors[20] = torch.tensor(_b(0, 0, 20, 16))                    # IoU 0.8 with the box
    anchors[30] = torch.tensor(_b(0, 0, 20, 15))                    # IoU 0.75: positive through the threshold, row 0
    for tag, c1 in (("same_class", 2.0), ("other_class", 0.0)):
        lab = torch.tensor([[[2.0] + _b(0, 0, 20, 20), [c1] + _b(0, 0, 20, 20)]])

        def check_dup(ref, c1=c1):
            assert _claimed(ref) == [10, 20]
            assert ref.amap[0, [10, 20, 30]].tolist() == [0, 1, 0]
            assert ref.classes[0, [10, 20, 30]].tolist() == [3, int(c1) + 1, 3]
        cases.append(RoiCase(f"dup_gt_{tag}", anchors, lab, 0.5, check_dup))
    # ---- duplicated anchors in different threads (a, a + 1), waves (a + 64) and 1024-strides (a + 1024): the lowest
    # flat index wins each round.  Box G sits at 70, 71, 134, 1094 (the lowest in wave 1), H at 1030 and 7.
    anchors = _anchor_set(2500, 11) * 0.5 + 0.5
    G, H = torch.tensor(_b(2, 2, 22, 30)), torch.tensor(_b(1, 3, 9, 31))
    anchors[[70, 71, 134, 1094]] = G
    anchors[[1030, 7]] = H
    lab = torch.stack([torch.cat([torch.tensor([0.0]), G]), torch.cat([torch.tensor([1.0]), H]),
                       torch.cat([torch.tensor([2.0]), G])]).unsqueeze(0)

    def check_dup_anchors(ref):
        assert _claimed(ref) == [7, 70, 71]      # all IoU 1: flat indices 7 N + 1 < 70 N + 0 < 71 N + 2
        assert ref.amap[0, [70, 71, 134, 1094, 7, 1030]].tolist() == [0, 2, 0, 0, 1, 1]
    cases.append(RoiCase("dup_anchors", anchors, lab, 0.5, check_dup_anchors))
    # ---- a zero-area box and a box that overlaps no anchor (anchors in the left half)
    anchors = grid_boxes(130, torch.Generator().manual_seed(12), hi=GRID // 2, max_side=16)
    lab = torch.tensor([[[0.0] + _b(10, 12, 10, 30), [1.0] + _b(40, 40, 60, 64), [2.0] + _b(4, 4, 12, 12)]])

    def check_degenerate(ref):
        iou = box_iou_ref(anchors, lab[0, :, 1:])
        assert bool((iou[:, :2] == 0).all()) and bool(torch.isfinite(iou).all()) and float(iou[:, 2].max()) > 0
    cases.append(RoiCase("zero_area_and_no_overlap", anchors, lab, 0.5, check_degenerate))
    cases.append(batch_case())
    if large:
        cases.append(large_case())
    return cases


# ------------------------------------------------------------------------------------------------------ loss
class LossRef(NamedTuple):
    stats: torch.Tensor       # [5] fp64: sum CE over positives, positives, sum CE over negatives, negatives, sum L1
    loss: float               # NaN without positives or without negatives, as the reference expression
    g_logits: torch.Tensor    # [R, K] fp64
    g_bbox: torch.Tensor      # [R, 4] fp64
    w: torch.Tensor           # [R] fp64: the weight of each row's softmax - onehot
    w_l1: float
    ce: torch.Tensor          # [R] fp64


def det_loss_ref(logits, bbox, offset, mask, labels, ratio, g_loss=1.0) -> LossRef:
    """``ratio`` is taken as the fp32 number the operation receives (torch multiplies an fp32 scalar tensor by it; the
    kernel's argument is a float)."""
    K = logits.shape[-1]
    x = logits.detach().to("cpu", F64).reshape(-1, K)
    bb, off, m = (t.detach().to("cpu", F64).reshape(-1, 4) for t in (bbox, offset, mask))
    y = labels.detach().to("cpu").reshape(-1).long()
    R = y.numel()
    ratio = float(torch.tensor(ratio, dtype=F32))
    g = float(torch.tensor(g_loss, dtype=F32))
    mx = x.max(dim=1, keepdim=True).values              # logsumexp - x[y], both taken relative to the row maximum:
    xs = x - mx                                          # exact for fp32 logits, so nothing cancels at the size of mx
    first_max = torch.zeros_like(xs).scatter_(1, xs.argmax(dim=1, keepdim=True), 1.0)
    rest = (torch.exp(xs) * (1.0 - first_max)).sum(dim=1)            # the maximum's own term is exp(0) = 1: log1p of the rest
    ce = torch.log1p(rest) - xs.gather(1, y[:, None])[:, 0]
    pos = y > 0
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    diff = bb * m - off * m
    stats = torch.stack([ce[pos].sum(), torch.tensor(float(n_pos), dtype=F64), ce[~pos].sum(),
                         torch.tensor(float(n_neg), dtype=F64), diff.abs().sum()])
    nan = float("nan")
    gt = float(stats[0]) / n_pos if n_pos else nan
    bg = float(stats[2]) / n_neg if n_neg else nan
    loss = (gt * ratio + bg * (1.0 - ratio)) + float(stats[4]) / (4.0 * R)      # soda.py:277-281, the three terms in order
    w_pos = g * ratio / n_pos if n_pos else nan                                 # no row carries a NaN weight
    w_neg = g * (1.0 - ratio) / n_neg if n_neg else nan
    w = torch.where(pos, torch.tensor(w_pos, dtype=F64), torch.tensor(w_neg, dtype=F64))
    onehot = torch.zeros_like(x)
    onehot.scatter_(1, y[:, None], 1.0)
    g_logits = w[:, None] * (torch.softmax(x, dim=1) - onehot)
    w_l1 = g / (4.0 * R)
    g_bbox = w_l1 * torch.sign(diff) * m
    return LossRef(stats, loss, g_logits, g_bbox, w, w_l1, ce)


def loss_inputs(rows, K, cond, seed):
    """Inputs of one loss case (fp32 host tensors).  Every case carries rows with bbox * mask == offset * mask exactly
    and the padded-label quirk (class 0 with mask 1); ``cond`` is one of base, g_ratio, no_pos, no_neg, big_logits."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(rows, K, generator=g)
    labels = (torch.rand(rows, generator=g) < 0.25).long() * torch.randint(1, K, (rows,), generator=g)
    if cond == "no_pos":
        labels.zero_()
    elif cond == "no_neg":
        labels = torch.randint(1, K, (rows,), generator=g)
    mask = (labels > 0).float().unsqueeze(-1).repeat(1, 4)
    quirk = torch.arange(rows) % 5 == 0
    mask[quirk & (labels == 0)] = 1.0                        # padded label rows: class 0 with a box mask
    bbox = torch.randn(rows, 4, generator=g)
    offset = torch.randn(rows, 4, generator=g) * mask
    same = torch.arange(rows) % 3 == 0
    bbox[same, 1] = offset[same, 1]                          # equal operands: sign 0 where the mask is 1 ...
    bbox[same, 2] = -offset[same, 2]
    offset[same & (mask[:, 0] == 0), 3] = 1.5                # ... and where both products are 0 * something
    if cond == "big_logits":
        # even rows: shifted so that the row maximum is +80 / -80 alternately (differences stay O(1): an unshifted
        # softmax overflows / underflows to 0, and mx + log(se) - x[y] cancels); odd rows: scaled by 80 / |row maximum|
        mx = logits.max(dim=1, keepdim=True).values
        r = torch.arange(rows)[:, None]
        shifted = (logits - mx) + torch.where(r % 4 == 0, 80.0, -80.0)
        scaled = logits * (80.0 / mx.abs())
        logits = torch.where(r % 2 == 0, shifted, scaled)
    g_loss, ratio = (-2.5, 0.5) if cond == "g_ratio" else (1.0, 0.04)
    return logits, bbox, offset, mask, labels, ratio, g_loss
