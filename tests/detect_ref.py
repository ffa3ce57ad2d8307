"""Restatement of the detection tail of ``csrc/detect.hip`` (TEST INFRASTRUCTURE ONLY; no device, no ``box.py``).

``decode`` / ``nms_sorted`` / ``nms_sorted_batched`` / ``assemble`` / ``detect`` state what ``snn_detect_decode[_batched]``,
``snn_nms_sorted[_batched]`` and ``snn_detect_assemble`` compute as ``include/snn_hip.h`` documents it, in the plainest
form: one float32 operation per arithmetic step (torch / numpy elementwise operations round once each), loops where the
kernels have tiles, chunks, masks and scans.  tests/test_detect_ref_host.py holds it against the reference goldens, the
host path and the oracle; tests/test_gpu_detect_kernels.py holds the kernels against it.

The second half builds the crafted inputs of those tests: boxes on the dyadic grid (coordinates k * 2^-6 in [0, 8)), where
every subtraction, product and sum of the IoU is exact in float32 and only its one division rounds.
"""
import functools

import numpy as np
import torch

FILL = -7                      # what `kept` holds where nothing is written (the tests compare written entries only)


# ============================================================================================================ decode
def argmax_first(prob):
    """conf, cls of ``prob[..., K]``: start from column 0, move on ``p[k] > best`` only - the first maximum wins, a NaN
    never replaces a finite best, a NaN in column 0 stays (then class -1, confidence NaN).  conf is the chosen ENTRY
    (its bits: -0 stays -0)."""
    prob = torch.as_tensor(prob, dtype=torch.float32)
    best = prob[..., 0].clone()
    arg = torch.zeros(prob.shape[:-1], dtype=torch.int32)
    for k in range(1, prob.shape[-1]):
        move = prob[..., k] > best
        best = torch.where(move, prob[..., k], best)
        arg = torch.where(move, torch.full_like(arg, k), arg)
    return best, arg - 1


def decode_boxes(offsets, anchors, dtype=torch.float32, ten=10.0, shift=0):
    """offset_inverse of ``offsets[A, 4]`` on ``anchors[A, 4]`` in ``dtype``, every operation on its own and in the
    order of decode_box: centre and size of the anchor, ``(off * size / 10) + centre``, ``exp(off / 5) * size``, corners.
    ``ten`` / ``shift`` exist for the teeth checks only (a wrong divisor, the anchor of the next row)."""
    off = torch.as_tensor(offsets).to(dtype)
    anc = torch.roll(torch.as_tensor(anchors).to(dtype), -shift, 0)
    x1, y1, x2, y2 = anc[:, 0], anc[:, 1], anc[:, 2], anc[:, 3]
    centre = torch.stack(((x1 + x2) / 2, (y1 + y2) / 2), dim=-1)
    size = torch.stack((x2 - x1, y2 - y1), dim=-1)
    xy = (off[:, :2] * size / ten) + centre
    wh = torch.exp(off[:, 2:] / 5) * size
    cx, cy, w, h = xy[:, 0], xy[:, 1], wh[:, 0], wh[:, 1]
    return torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)


def decode(prob, offsets, anchors, dtype=torch.float32):
    """``prob[N, A, K]``, ``offsets[N, A, 4]``, ``anchors[A, 4]`` (or one frame without N) -> conf (float32), cls
    (int32), boxes (``dtype``: float32 = op by op as the kernel, float64 = the yardstick of the general inputs)."""
    prob, offsets = torch.as_tensor(prob), torch.as_tensor(offsets)
    conf, cls = argmax_first(prob)
    if prob.dim() == 2:
        return conf, cls, decode_boxes(offsets, anchors, dtype)
    return conf, cls, torch.stack([decode_boxes(o, anchors, dtype) for o in offsets])


# =============================================================================================================== NMS
def iou_f32(p, q):
    """iou_of(p, q) of detect.hip in float32, one operation at a time; ``p[4]`` against ``q[M, 4]`` (or ``[4]``).
    fmaxf / fminf return the operand that is not NaN (np.fmax / np.fmin)."""
    p, q = np.asarray(p, np.float32), np.asarray(q, np.float32)
    with np.errstate(all="ignore"):
        area1 = (p[..., 2] - p[..., 0]) * (p[..., 3] - p[..., 1])
        area2 = (q[..., 2] - q[..., 0]) * (q[..., 3] - q[..., 1])
        lx, ly = np.fmax(p[..., 0], q[..., 0]), np.fmax(p[..., 1], q[..., 1])
        rx, ry = np.fmin(p[..., 2], q[..., 2]), np.fmin(p[..., 3], q[..., 3])
        ow, oh = np.fmax(rx - lx, np.float32(0)), np.fmax(ry - ly, np.float32(0))
        overlap = ow * oh
        return overlap / (area1 + area2 - overlap)


def greedy(boxes, ids, thr):
    """Kept ids of one class: walk ``ids`` in the given order; a candidate survives only while ``iou <= thr`` against
    every box kept before it (so a NaN IoU, or a NaN threshold, suppresses)."""
    thr = np.float32(thr)
    kept = []
    for i in ids:
        if not kept or bool(np.all(iou_f32(boxes[kept], boxes[i]) <= thr)):
            kept.append(int(i))
    return kept


def _nms_ranges(boxes, order, ranges, thr, num_rows):
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    order = np.asarray(order, np.int64).reshape(-1)
    kept = np.full(order.shape[0], FILL, np.int64)
    nkept = np.zeros(len(ranges), np.int64)
    flag = np.zeros(num_rows, bool)
    rank = np.full(num_rows, FILL, np.int64)
    for c, (lo, hi) in enumerate(ranges):
        got = greedy(boxes, order[lo:hi], thr)
        kept[lo:lo + len(got)] = got
        nkept[c] = len(got)
        flag[got] = True
        rank[got] = np.arange(len(got))
    return kept, nkept, flag, rank


def nms_sorted(boxes, order, seg, thr):
    """snn_nms_sorted: the members of class c are ``order[seg[c] .. seg[c + 1])``.  -> kept (FILL where nothing is
    written), nkept[C], kept_flag[A] (bool), kept_rank[A] (FILL where not kept)."""
    seg = [int(s) for s in np.asarray(seg).reshape(-1)]
    return _nms_ranges(boxes, order, list(zip(seg[:-1], seg[1:])), thr, np.asarray(boxes).reshape(-1, 4).shape[0])


def nms_sorted_batched(boxes, order, seg, N, A, thr):
    """snn_nms_sorted_batched: rows ``n * A + anchor``, ``seg[N][C + 1]`` counting inside the frame; a class whose
    segment is not a non-decreasing pair inside [0, A] is empty.  nkept comes back ``[N, C]``, the others flat."""
    seg = np.asarray(seg, np.int64).reshape(N, -1)
    ranges = []
    for n in range(N):
        for lo, hi in zip(seg[n, :-1], seg[n, 1:]):
            if lo < 0 or hi > A or lo > hi:
                lo = hi = 0
            ranges.append((n * A + int(lo), n * A + int(hi)))
    kept, nkept, flag, rank = _nms_ranges(boxes, order, ranges, thr, N * A)
    return kept, nkept.reshape(N, -1), flag, rank


# ========================================================================================================== assemble
def assemble_positions(cls, nkept, kept_flag, kept_rank):
    """Output position of every row of one frame: kept rows at class_off[class] + rank (class_off = exclusive sum of
    nkept), the others behind all kept rows in anchor order."""
    class_off = np.concatenate(([0], np.cumsum(nkept)))
    pos, rest = [], int(class_off[-1])
    for a in range(len(cls)):
        if kept_flag[a]:
            pos.append(int(class_off[int(cls[a])] + kept_rank[a]))
        else:
            pos.append(rest)
            rest += 1
    return pos


def assemble(conf, cls, boxes, nkept, kept_flag, kept_rank, pos_threshold):
    """snn_detect_assemble for ``[N, A]`` inputs -> ``out[N, A, 6]`` (float32; NaN where no row lands): class (-1 for a
    row not kept or weak), confidence (1 - conf for a weak row, in float32), box.  weak is ``conf < pos_threshold`` in
    float32, so equality and NaN are not weak."""
    conf = np.asarray(conf, np.float32)
    N, A = conf.shape
    cls = np.asarray(cls).reshape(N, A)
    boxes = np.asarray(boxes, np.float32).reshape(N, A, 4)
    nkept = np.asarray(nkept).reshape(N, -1)
    flag, rank = np.asarray(kept_flag).reshape(N, A), np.asarray(kept_rank).reshape(N, A)
    out = np.full((N, A, 6), np.nan, np.float32)
    pt = np.float32(pos_threshold)
    for n in range(N):
        for a, pos in enumerate(assemble_positions(cls[n], nkept[n], flag[n], rank[n])):
            p = conf[n, a]
            weak = bool(p < pt)
            out[n, pos, 0] = np.float32(cls[n, a]) if (flag[n, a] and not weak) else np.float32(-1)
            out[n, pos, 1] = np.float32(1) - p if weak else p
            out[n, pos, 2:] = boxes[n, a]
    return torch.from_numpy(out)


# ============================================================================================================ the tail
def order_and_seg(conf, cls, K):
    """Candidate order of one frame, by sorting tuples: (class ascending, confidence descending, anchor ascending),
    background (and with it every NaN confidence: only column 0 can leave one) in front.  seg[K] = inclusive counts."""
    conf, cls = np.asarray(conf, np.float32), np.asarray(cls)
    assert not np.any(np.isnan(conf[cls >= 0]))
    ids = sorted(range(len(cls)), key=lambda a: (int(cls[a]), -float(conf[a]) if cls[a] >= 0 else 0.0, a))
    seg = np.cumsum([int(np.sum(cls == k - 1)) for k in range(K)])
    return np.asarray(ids, np.int64), seg


def detect(prob, offsets, anchors, thr, pos, boxes=None):
    """The whole tail for ``prob[N, A, K]``: decode (float32; or the given ``boxes[N, A, 4]``, to judge NMS and assembly
    on another decode's boxes), order, per-class greedy NMS, output rows.  Equal confidences of a class are candidates
    in anchor order - the documented order of snn_nms_sorted_batched."""
    prob = torch.as_tensor(prob, dtype=torch.float32)
    N, A, K = prob.shape
    conf, cls, dec = decode(prob, offsets, anchors)
    boxes = dec if boxes is None else torch.as_tensor(boxes, dtype=torch.float32).reshape(N, A, 4)
    conf, cls, boxes = conf.numpy(), cls.numpy(), boxes.numpy()
    nk, fl, rk = [], [], []
    for n in range(N):
        order, seg = order_and_seg(conf[n], cls[n], K)
        _, nkept, flag, rank = nms_sorted(boxes[n], order, seg, thr)
        nk.append(nkept), fl.append(flag), rk.append(rank)
    return assemble(conf, cls, boxes, np.stack(nk), np.stack(fl), np.stack(rk), pos)


# ==================================================================================================== crafted inputs
G = 2.0 ** -6                  # the grid; a cell is 16 x 16 grid steps, 32 x 32 cells tile [0, 8)^2
CELLS = 1024


def cell(k, dx=0, dy=0, shrink=0):
    """Cell k of the 32 x 32 tiling (side 1/4), moved by dx / dy grid steps, its top edge lowered by ``shrink`` steps.
    Cells are disjoint (neighbours touch: IoU exactly 0); cell(k, dx=1) against cell(k) has IoU 15/17, a cell with
    shrink=1 lies inside its cell with IoU 15/16."""
    x = (k % 32) * 16 + (dx if k % 32 < 31 else -dx)       # (the last column / row moves the other way: all in [0, 8))
    y = (k // 32) * 16 + (dy if k // 32 < 31 else -dy)
    return [x * G, y * G, (x + 16) * G, (y + 16 - shrink) * G]


class NmsCase:
    """One input of snn_nms_sorted: ``boxes[A, 4]``, ``order[A]``, ``seg[C + 1]``.  ``classes`` lists, per class, the boxes
    in candidate order; they are scattered over the anchors by a seeded permutation (ids differ from positions) unless
    the class is named in ``ascending``, whose ids then rise along the candidate order (the order of equal
    confidences).  ``background`` rows stand in front of seg[0]."""

    def __init__(self, name, classes, thr=0.5, background=(), ascending=(), seed=0, note=None):
        self.name, self.thr, self.note = name, thr, note or {}
        rows = [list(b) for b in background] + [list(b) for cl in classes for b in cl]
        A = len(rows)
        perm = torch.randperm(A, generator=torch.Generator().manual_seed(1000 + seed)).numpy() if A else np.zeros(0, np.int64)
        seg, at = [len(background)], len(background)
        for c, cl in enumerate(classes):
            if c in ascending:
                perm[at:at + len(cl)] = np.sort(perm[at:at + len(cl)])
            at += len(cl)
            seg.append(at)
        self.A, self.C = A, len(classes)
        self.order = perm.astype(np.int64)
        self.seg = np.asarray(seg, np.int64)
        self.boxes = np.zeros((A, 4), np.float32)
        if A:
            self.boxes[perm] = np.asarray(rows, np.float32).reshape(A, 4)

    def position_of_class(self, c, i):
        """Position in ``order`` of candidate i of class c."""
        return int(self.seg[c]) + i

    def expected(self):
        if not hasattr(self, "_exp"):
            self._exp = nms_sorted(self.boxes, self.order, self.seg, self.thr)
        return self._exp


def count_case(n):
    """n candidates in class 1 (class 0 has two, class 2 one or none): candidate 2i is cell i, candidate 2i + 1 the same
    cell moved by one grid step (IoU 15/17: suppressed), so ceil(n / 2) are kept and kept / suppressed alternate through
    every chunk boundary."""
    mid = [cell(i // 2, dx=i % 2) for i in range(n)]
    last = [cell(900)] if n % 2 else []
    return NmsCase(f"count-{n}", [[cell(800), cell(801)], mid, last], background=[cell(1000), cell(1001)], seed=n,
                   note=dict(nkept=[2, (n + 1) // 2, len(last)]))


TILE_PROBES = (0, 255, 256, 257, 511, 512)


def tile_case(m):
    """m disjoint kept boxes (cells 0 .. m-1), copies of cell 0 (suppressed) up to the next chunk boundary, then the
    probes: for t in TILE_PROBES below m a box inside cell t (IoU 15/16 with kept box t, 0 with every other), and one cell
    that overlaps nothing.  The probes start a chunk, so they meet the kept boxes only through the kept tiles."""
    start = -(-m // 256) * 256
    probes = [t for t in TILE_PROBES if t < m]
    cands = [cell(k) for k in range(m)] + [cell(0)] * (start - m) + [cell(t, shrink=1) for t in probes] + [cell(1023)]
    return NmsCase(f"tiles-{m}", [cands], background=[cell(1000)], seed=m,
                   note=dict(m=m, start=start, probes=probes, nkept=[m + 1]))


TRIPLE_AT = (64, 128, 192, 255)       # C of each triple sits here, B one before, A two before


def _triple(x, y):
    """A, B, C: unit squares 1/4 apart.  IoU(A, B) = IoU(B, C) = 3/5, IoU(A, C) = 1/3."""
    return [[x, y, x + 1, y + 1], [x + 0.25, y, x + 1.25, y + 1], [x + 0.5, y, x + 1.5, y + 1]]


def greedy_case():
    """One class of 264 candidates, disjoint cells (rows y >= 2) except five A/B/C triples: A suppresses B, B alone
    would suppress C, so C is kept.  Four triples straddle the 64-bit mask words of chunk 0 (B / C at 63 / 64, 127 / 128,
    191 / 192, 254 / 255); the fifth has A at position 10 and B, C at 261, 262 in chunk 1 (B falls to the kept tile)."""
    cands = [cell(256 + i) for i in range(264)]
    where = {}
    for t, at in enumerate(TRIPLE_AT):
        a, b, c = _triple(2.0 * t, 0.0)
        cands[at - 2], cands[at - 1], cands[at] = a, b, c
        where[t] = (at - 2, at - 1, at)
    a, b, c = _triple(0.0, 1.0)
    cands[10], cands[261], cands[262] = a, b, c
    where[4] = (10, 261, 262)
    return NmsCase("greedy", [cands], seed=5, note=dict(triples=where, nkept=[264 - 5]))


P_BOX, Q_BOX = [0, 0, 2, 1], [0, 0, 1, 1]                          # IoU exactly 1/2
HALF_BELOW = float(np.nextafter(np.float32(0.5), np.float32(0)))
# name -> (threshold, kept per class of edge_case)
EDGE_ROWS = {"half": (0.5, [2, 2, 1, 3, 1]), "below-half": (HALF_BELOW, [1, 2, 1, 3, 1]), "zero": (0.0, [1, 2, 1, 3, 1]),
             "one": (1.0, [2, 2, 2, 3, 5]), "negative": (-0.25, [1, 1, 1, 1, 1]), "nan": (float("nan"), [1, 1, 1, 1, 1])}


def edge_case(name):
    """One row of EDGE_ROWS.  class 0: P, Q (IoU 1/2); class 1: two touching squares (IoU 0); class 2: two identical squares (IoU 1); class 3:
    three disjoint cells; class 4: five identical boxes of equal confidence, ids ascending - the first is the lowest."""
    classes = [[P_BOX, Q_BOX], [[2, 2, 3, 3], [3, 2, 4, 3]], [[4, 4, 5, 5]] * 2, [cell(600), cell(601), cell(602)],
               [[6, 6, 7, 7]] * 5]
    thr, nkept = EDGE_ROWS[name]
    return NmsCase(f"edge-{name}", classes, thr=thr, background=[cell(1000)], ascending=(4,), seed=9,
                   note=dict(nkept=nkept))


INF, NAN = float("inf"), float("nan")


def degenerate_case():
    """What the float32 arithmetic of iou_of makes of boxes that are no boxes (threshold 1/2), class by class:
    0: two identical zero-area boxes - 0 / 0 = NaN, the second is suppressed;
    1: a zero-area box, then a proper one around it - IoU 0, both kept;
    2: a proper box, an inverted one (x2 < x1) inside it and the inverted one again - the overlap clamps to 0, the
       quotients are 0 / 1 and 0 / -2 = -0: all kept;
    3: [0, 0, inf, 1], a finite box inside it (1 / inf = 0: kept), the inf box again (inf / (inf + inf - inf) = NaN:
       suppressed);
    4: a proper box, a box with a NaN coordinate over it (NaN area: suppressed), a disjoint proper box (kept);
    5: the NaN box first (kept), then a proper box over it (NaN: suppressed)."""
    nan_box = [NAN, 0, 1, 1]
    classes = [[[1, 1, 1, 1]] * 2, [[1, 1, 1, 2], [0, 0, 2, 2]], [[0, 0, 2, 1], [2, 0, 1, 1], [2, 0, 1, 1]],
               [[0, 0, INF, 1], [0, 0, 1, 1], [0, 0, INF, 1]], [[0, 0, 1, 1], nan_box, [4, 4, 5, 5]],
               [nan_box, [0, 0, 1, 1]]]
    return NmsCase("degenerate", classes, background=[cell(1000)], seed=11, note=dict(nkept=[1, 2, 3, 2, 2, 1]))


def many_classes_case():
    """C = 1024: class c has cell c; every third class has a second candidate - a moved copy of the cell (suppressed)
    or, in every sixth class, a far cell (kept)."""
    classes = []
    for c in range(1024):
        cl = [cell(c)]
        if c % 6 == 0:
            cl.append(cell((c + 512) % 1024))
        elif c % 3 == 0:
            cl.append(cell(c, dx=1))
        classes.append(cl)
    return NmsCase("classes-1024", classes, background=[cell(5), cell(6), cell(7)], seed=13,
                   note=dict(nkept=[2 if c % 6 == 0 else 1 for c in range(1024)]))


COUNTS = (0, 1, 2, 255, 256, 257, 511, 512, 513)
NMS_CASE_NAMES = tuple([f"count-{n}" for n in COUNTS] + ["tiles-257", "tiles-513", "greedy"]
                       + [f"edge-{name}" for name in EDGE_ROWS] + ["degenerate", "classes-1024"])


@functools.lru_cache(maxsize=None)
def nms_case(name):
    """The case of that name, built when it is first asked for (the tests parametrise over NMS_CASE_NAMES)."""
    kind, _, arg = name.partition("-")
    case = {"count": lambda: count_case(int(arg)), "tiles": lambda: tile_case(int(arg)), "greedy": greedy_case,
            "edge": lambda: edge_case(arg), "degenerate": degenerate_case, "classes": many_classes_case}[kind]()
    assert case.name == name
    return case


def nms_cases():
    return [nms_case(name) for name in NMS_CASE_NAMES]


# seg entries of frame `pos` that batched_frames makes malformed for C = 1024: (index, value) with A for the frame size.
# 301 falls below its predecessor and 302 lies above A (classes 300, 301, 302 lose a bound), 701 is negative (700, 701).
def malformed(seg, A):
    seg = seg.copy()
    seg[301], seg[302], seg[701] = seg[300] - 1, A + 3, -5
    return seg, (300, 301, 302, 700, 701)


def batched_frames(case, pos):
    """The case as frame ``pos`` of N = 3, between two neighbours made from it: one with every class's candidates in
    reverse order, one with the boxes rolled by one row under the same order (other boxes per id).  With C = 1024 the
    case's own frame gets the malformed seg rows.  -> boxes[3 * A, 4], order[3 * A] (row ids), seg[3, C + 1], bad classes."""
    A = case.A
    rev = case.order.copy()
    for lo, hi in zip(case.seg[:-1], case.seg[1:]):
        rev[lo:hi] = rev[lo:hi][::-1].copy()
    others = [(case.boxes, rev, case.seg), (np.roll(case.boxes, 1, 0), case.order, case.seg)]
    seg, bad = (malformed(case.seg, A) if case.C == 1024 else (case.seg, ()))
    frames = others[:pos] + [(case.boxes, case.order, seg)] + others[pos:]
    boxes = np.concatenate([f[0] for f in frames]).reshape(3 * A, 4)
    order = np.concatenate([f[1] + n * A for n, f in enumerate(frames)])
    return boxes, order, np.stack([f[2] for f in frames]), bad


# --------------------------------------------------------------------------------------------------- assemble inputs
ASSEMBLE_SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
PATTERNS = ("none", "all", "alternating", "lane63", "lane0", "last")
POS_THRESHOLD = 0.25


def pattern(name, A):
    a = np.arange(A)
    return {"none": a < 0, "all": a >= 0, "alternating": a % 2 == 0, "lane63": a % 64 == 63, "lane0": a % 64 == 0,
            "last": a == A - 1}[name]


def assemble_frame(A, C, name, seed):
    """One frame whose kept rows are exactly ``pattern(name, A)``, by construction and then through the restatement's
    own NMS: a row of the pattern is a cell of its own with class a % C; another row is a background row or - every
    second one, when the pattern has a row - a copy of a kept row's box in that row's class with a lower confidence.
    Confidences of kept rows cycle through 1/8 (weak at POS_THRESHOLD = 1/4: slot kept, class -1, 7/8), 1/4 (equal: not
    weak), 1/2, 3/4; background rows cycle through 15/16, 1/8 (weak), NaN.  After the NMS step the middle one of the kept
    rows gets a NaN confidence (no decode gives a kept row one, but the kernel takes what it is handed): NaN is not weak,
    so that row keeps its class - the one place where weak and not weak differ for a NaN.
    -> conf, cls, boxes, nkept, flag, rank."""
    want = pattern(name, A)
    kept_rows = np.flatnonzero(want)
    conf, cls, boxes = np.zeros(A, np.float32), np.zeros(A, np.int64), np.zeros((A, 4), np.float32)
    j = 0
    for a in range(A):
        if want[a]:                                     # (a -> (7 a + seed) mod 1024 is one to one: disjoint cells)
            cls[a], conf[a] = a % C, (0.125, 0.25, 0.5, 0.75)[(a // 3 + seed) % 4]
            boxes[a] = cell((a * 7 + seed) % CELLS)
        elif len(kept_rows) and j % 2 == 0:
            src = int(kept_rows[(j // 2) % len(kept_rows)])
            cls[a], conf[a] = src % C, (0.0625, 0.03125)[(j // 2) % 2]
            boxes[a] = cell((src * 7 + seed) % CELLS)
            j += 1
        else:
            cls[a], conf[a] = -1, (0.9375, 0.125, NAN)[(a + seed) % 3]
            boxes[a] = cell((a * 7 + seed) % CELLS, dx=3)
            j += 1
    order, seg = order_and_seg(conf, cls, C + 1)
    _, nkept, flag, rank = nms_sorted(boxes, order, seg, 0.5)
    if len(kept_rows):
        conf[kept_rows[len(kept_rows) // 2]] = NAN
    return conf, cls, boxes, nkept, flag, rank


def assemble_input(A, C, names, seed=0):
    """N = len(names) frames -> conf[N, A], cls[N, A], boxes[N, A, 4], nkept[N, C], flag[N, A], rank[N, A] (rank 0
    where not kept, as the zeroed array of the caller holds it)."""
    parts = [assemble_frame(A, C, name, seed + 17 * n) for n, name in enumerate(names)]
    conf, cls, boxes, nkept, flag, rank = (np.stack([p[i] for p in parts]) for i in range(6))
    return conf, cls, boxes, nkept, flag, np.where(flag, rank, 0)


# ----------------------------------------------------------------------------------------------------- decode inputs
def dyadic_anchors(A, seed=0):
    """Anchors on the grid: corners k * 2^-6 in [0, 8), sides of at least one step."""
    g = torch.Generator().manual_seed(300 + seed)
    lo = torch.randint(0, 384, (A, 2), generator=g)
    side = torch.randint(1, 128, (A, 2), generator=g)
    return torch.cat((lo, lo + side), dim=1).float() * G


def random_anchors(A, seed=0):
    g = torch.Generator().manual_seed(400 + seed)
    centre, wh = torch.rand(A, 2, generator=g), 0.02 + 0.3 * torch.rand(A, 2, generator=g)
    return torch.cat((centre - wh / 2, centre + wh / 2), dim=1)


# rows of the argmax table (K = 3 columns; wider inputs repeat the last column, narrower ones cut): name, row, class, conf
_Z = -0.0
ARGMAX_ROWS = [
    ("tie-first-wins", [0.25, 0.375, 0.375], 0, 0.375),
    ("tie-with-background", [0.5, 0.5, 0.0], -1, 0.5),
    ("all-equal", [0.25, 0.25, 0.25], -1, 0.25),
    ("all-nan", [NAN, NAN, NAN], -1, NAN),
    ("nan-in-column-0", [NAN, 0.75, 0.25], -1, NAN),
    ("nan-in-later-column", [0.125, NAN, NAN], -1, 0.125),
    ("plus-then-minus-zero", [0.0, _Z, _Z], -1, 0.0),
    ("minus-then-plus-zero", [_Z, 0.0, 0.0], -1, _Z),
]


def argmax_table(K):
    """The rows of ARGMAX_ROWS at K columns (K = 2 keeps columns 0 and 1) plus, for K >= 3, a NaN in the middle of a row
    whose maximum stands behind it."""
    rows = [(r[:2] if K == 2 else r + [r[2]] * (K - 3)) for _, r, _, _ in ARGMAX_ROWS]
    if K >= 3:
        rows.append([0.125, NAN] + [0.5] * (K - 2))
    return torch.tensor(rows, dtype=torch.float32)


def decode_probs(shape, K, seed=0):
    """Random probabilities on the 1/64 grid (many ties) with the argmax table written over the first rows of the last
    frame (as far as there is room)."""
    g = torch.Generator().manual_seed(500 + seed)
    prob = torch.randint(0, 65, (*shape, K), generator=g).float() * G
    table = argmax_table(K)
    n = min(len(table), shape[-1])
    prob.reshape(-1, shape[-1], K)[-1, :n] = table[:n]
    return prob


def exact_offsets(shape, seed=0):
    """Centre offsets on a 1/8 grid in [-8, 8], size offsets 0 (expf(0) = 1 on every implementation)."""
    g = torch.Generator().manual_seed(600 + seed)
    off = torch.zeros(*shape, 4)
    off[..., :2] = torch.randint(-64, 65, (*shape, 2), generator=g).float() / 8
    return off


def general_offsets(shape, seed=0):
    """|offset| <= 8, and in the first rows size offsets at which exp(off / 5) leaves float32 AND float64 at both ends
    (+-4000: inf and 0 on both sides, so the yardstick says the same)."""
    g = torch.Generator().manual_seed(700 + seed)
    off = (torch.rand(*shape, 4, generator=g) * 16 - 8)
    flat = off.reshape(-1, 4)
    if flat.shape[0] >= 8:
        flat[1, 2], flat[2, 3], flat[3, 2], flat[4, 3] = 4000.0, 4000.0, -4000.0, -4000.0
        flat[5, 2:] = torch.tensor([4000.0, -4000.0])
    return off


def pipeline_exact(N, A, K, seed=0):
    """Exact pipeline input: anchors = cells and moved copies of them (IoUs 0, 15/17, 1 ...), centre offsets 0, size
    offsets 0, probabilities on a 1/8 grid - groups of equal confidence inside every class."""
    g = torch.Generator().manual_seed(800 + seed)
    which = torch.randint(0, max(A // 4, 1), (A,), generator=g)
    dx = torch.randint(0, 3, (A,), generator=g)
    anchors = torch.tensor([cell(int(k), dx=int(d)) for k, d in zip(which, dx)], dtype=torch.float32)
    prob = torch.randint(0, 9, (N, A, K), generator=g).float() / 8
    return prob, torch.zeros(N, A, 4), anchors


def pipeline_random(N, A, K, seed=0):
    g = torch.Generator().manual_seed(900 + seed)
    centre, wh = torch.rand(A, 2, generator=g), 0.05 + 0.2 * torch.rand(A, 2, generator=g)
    anchors = torch.cat((centre - wh / 2, centre + wh / 2), dim=1)
    prob = torch.softmax(3 * torch.randn(N, A, K, generator=g), dim=2)
    return prob, 0.5 * torch.randn(N, A, 4, generator=g), anchors
