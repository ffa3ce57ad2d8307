"""Reference of the selectable detection loss (TEST INFRASTRUCTURE ONLY; nothing here imports the package).

A torch restatement of the formulas of include/snn_hip.h ("Selectable detection loss"), written from the focal-loss
(Lin et al. 2017), GIoU (Rezatofighi et al. 2019) and DIoU / CIoU (Zheng et al. 2020) papers, with the gradients taken by
torch autograd.  ``ext_loss_ref(..., dtype=torch.float64)`` is the reference; the same function at ``torch.float32`` is
the yardstick the tests measure the kernels against (fp32 CPU arithmetic of the same expressions, independent of the
code under test).

    cls  = ratio * sum_pos f / max(n_pos, 1) + (1 - ratio) * sum_neg f / max(n_neg, 1)
           f = ce or (1 - p_y)^gamma ce,  ce = -log softmax(x)[y],  pos: class > 0
    box  = weight * sum |bbox m - off m| / (4 A V)                                 (l1)
         = weight * sum over box rows (1 - IoU + penalty) / max(n_pos, 1)          (giou, diou, ciou)
           box rows: class > 0 and mask row == 1; boxes decoded from the anchor (row % A) with the exponent argument
           clamped above at log(1000 / 16)

Frames (``A`` rows each) whose entry of ``steps`` is negative are empty slots: dropped from every sum, zero gradients, as
in tests/seq_targets_ref.py; ``V`` counts the others, ``V = 0`` gives loss 0.
"""
import math
from typing import NamedTuple, Optional

import torch

F32, F64 = torch.float32, torch.float64
EXP_CLAMP = math.log(1000.0 / 16.0)
EPS = 1e-7
CLS_MODES = ("ce", "focal")
BOX_MODES = ("l1", "giou", "diou", "ciou")
MODES = [(c, b) for c in CLS_MODES for b in BOX_MODES]
TIE_MARGIN = 1e-4      # in units of the anchor's side: corners / clamp arguments closer than this count as tied


def decode(anchors, offsets):
    """offset_inverse (utils/box.py:72-79) with the clamp -> corner boxes."""
    cxa, cya = (anchors[:, 0] + anchors[:, 2]) / 2, (anchors[:, 1] + anchors[:, 3]) / 2
    wa, ha = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    cx, cy = offsets[:, 0] * wa / 10 + cxa, offsets[:, 1] * ha / 10 + cya
    w = torch.exp(torch.clamp(offsets[:, 2] / 5, max=EXP_CLAMP)) * wa
    h = torch.exp(torch.clamp(offsets[:, 3] / 5, max=EXP_CLAMP)) * ha
    return torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=1)


def iou_terms(p, g):
    px1, py1, px2, py2 = p.unbind(1)
    gx1, gy1, gx2, gy2 = g.unbind(1)
    iw = torch.clamp(torch.minimum(px2, gx2) - torch.maximum(px1, gx1), min=0)
    ih = torch.clamp(torch.minimum(py2, gy2) - torch.maximum(py1, gy1), min=0)
    inter = iw * ih
    union = (px2 - px1) * (py2 - py1) + (gx2 - gx1) * (gy2 - gy1) - inter
    cw = torch.maximum(px2, gx2) - torch.minimum(px1, gx1)
    ch = torch.maximum(py2, gy2) - torch.minimum(py1, gy1)
    return inter, union, cw, ch


def box_loss_rows(p, g, mode):
    """1 - IoU + penalty per row of corner boxes."""
    inter, union, cw, ch = iou_terms(p, g)
    iou = inter / (union + EPS)
    if mode == "giou":
        c = cw * ch
        return 1 - iou + (c - union) / (c + EPS)
    rho2 = ((p[:, 0] + p[:, 2]) / 2 - (g[:, 0] + g[:, 2]) / 2) ** 2 + ((p[:, 1] + p[:, 3]) / 2 - (g[:, 1] + g[:, 3]) / 2) ** 2
    out = 1 - iou + rho2 / (cw ** 2 + ch ** 2 + EPS)
    if mode == "ciou":
        v = 4 / math.pi ** 2 * (torch.atan((g[:, 2] - g[:, 0]) / (g[:, 3] - g[:, 1] + EPS))
                                - torch.atan((p[:, 2] - p[:, 0]) / (p[:, 3] - p[:, 1] + EPS))) ** 2
        alpha = (v / (1 - iou + v + EPS)).detach()
        out = out + alpha * v
    return out


class ExtRef(NamedTuple):
    V: int
    loss: float
    cls: float
    box: float
    g_logits: torch.Tensor       # [F, A, K], zeros in the empty slots
    g_bbox: torch.Tensor         # [F, A, 4]
    box_rows: torch.Tensor       # [F, A] bool: the rows of the IoU box term (valid slots only)
    n_pos: int


def ext_loss_ref(logits, bbox, offset, mask, labels, anchors, ratio, cls_mode, gamma, box_mode, box_weight, steps=None,
                 g_loss=1.0, dtype=F64) -> ExtRef:
    """``logits[F, A, K]``, ``bbox / offset / mask [F, A, 4]``, ``labels[F, A]``, ``anchors[A, 4]``, ``steps`` None or F
    entries (any shape).  ``ratio``, ``gamma``, ``box_weight`` and ``g_loss`` are taken as the fp32 numbers the operation
    receives."""
    Fr, A, K = logits.shape
    f32 = lambda v: float(torch.tensor(v, dtype=F32))
    ratio, gamma, box_weight, g_loss = f32(ratio), f32(gamma), f32(box_weight), f32(g_loss)
    valid = torch.ones(Fr, dtype=torch.bool) if steps is None else steps.detach().cpu().reshape(-1) >= 0
    V = int(valid.sum())
    g_logits, g_bbox = torch.zeros(Fr, A, K, dtype=dtype), torch.zeros(Fr, A, 4, dtype=dtype)
    box_rows = torch.zeros(Fr, A, dtype=torch.bool)
    if V == 0:
        return ExtRef(0, 0.0, 0.0, 0.0, g_logits, g_bbox, box_rows, 0)
    x = logits.detach().cpu()[valid].to(dtype).reshape(-1, K).requires_grad_()
    bb = bbox.detach().cpu()[valid].to(dtype).reshape(-1, 4).requires_grad_()
    off, m = (t.detach().cpu()[valid].to(dtype).reshape(-1, 4) for t in (offset, mask))
    y = labels.detach().cpu()[valid].reshape(-1).long()
    anc = anchors.detach().cpu().to(dtype).repeat(V, 1)
    logp = torch.log_softmax(x, dim=1)
    ce = -logp.gather(1, y[:, None])[:, 0]
    if cls_mode == "focal":
        p_y = torch.softmax(x, dim=1).gather(1, y[:, None])[:, 0]
        ce = (1 - p_y) ** gamma * ce
    pos = y > 0
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    cls = ratio * ce[pos].sum() / max(n_pos, 1) + (1 - ratio) * ce[~pos].sum() / max(n_neg, 1)
    rows = pos & (m == 1).all(dim=1)
    if box_mode == "l1":
        box = box_weight * (bb * m - off * m).abs().sum() / (4.0 * A * V)
    else:
        per_row = box_loss_rows(decode(anc[rows], bb[rows]), decode(anc[rows], off[rows]), box_mode)
        box = box_weight * per_row.sum() / max(n_pos, 1)
        box_rows[valid] = rows.reshape(V, A)
    loss = cls + box
    (loss * g_loss).backward()
    g_logits[valid] = x.grad.reshape(V, A, K)
    g_bbox[valid] = bb.grad.reshape(V, A, 4) if bb.grad is not None else 0
    return ExtRef(V, float(loss.detach()), float(cls.detach()), float(box.detach()), g_logits, g_bbox, box_rows, n_pos)


def tied_rows(bbox, offset, mask, labels, anchors) -> torch.Tensor:
    """``[F, A]`` bool: box rows (class > 0, mask row 1) on which a minimum / maximum / clamp of the box term is decided by
    less than ``TIE_MARGIN`` anchor sides (fp64): the subgradient there is ambiguous, and an fp32 evaluation may take the
    other branch."""
    Fr, A, _ = bbox.shape
    bb, off, m = (t.detach().cpu().to(F64).reshape(-1, 4) for t in (bbox, offset, mask))
    anc = anchors.detach().cpu().to(F64).repeat(Fr, 1)
    rows = (labels.detach().cpu().reshape(-1) > 0) & (m == 1).all(dim=1)
    p, g = decode(anc, bb), decode(anc, off)
    side = torch.stack((anc[:, 2] - anc[:, 0], anc[:, 3] - anc[:, 1], anc[:, 2] - anc[:, 0], anc[:, 3] - anc[:, 1]), dim=1)
    near = ((p - g).abs() < TIE_MARGIN * side).any(dim=1)                            # corner against corner
    dw = torch.minimum(p[:, 2], g[:, 2]) - torch.maximum(p[:, 0], g[:, 0])
    dh = torch.minimum(p[:, 3], g[:, 3]) - torch.maximum(p[:, 1], g[:, 1])
    near |= (dw.abs() < TIE_MARGIN * side[:, 0]) | (dh.abs() < TIE_MARGIN * side[:, 1])   # the intersection's clamp at 0
    near |= ((bb[:, 2:] / 5 - EXP_CLAMP).abs() < TIE_MARGIN).any(dim=1)              # the exponent's clamp
    return (rows & near).reshape(Fr, A)


# ------------------------------------------------------------------------------------------------------ inputs
CASES = ("random", "disjoint", "pred_contains", "target_contains", "clamped", "equal", "no_pos")


class ExtInputs(NamedTuple):
    logits: torch.Tensor     # [F, A, K] fp32
    bbox: torch.Tensor       # [F, A, 4]
    offset: torch.Tensor
    mask: torch.Tensor
    labels: torch.Tensor     # [F, A] int64
    anchors: torch.Tensor    # [A, 4]


def ext_inputs(Fr, A, K, case, seed) -> ExtInputs:
    """Continuous draws with a fixed seed.  A quarter of the rows are positive (mask row 1); every fifth background row
    carries the padded-label quirk (class 0 with mask 1) and every seventh positive row a zero mask: neither is a box row.
    ``case`` shapes the predicted offsets of the positive rows; outside ``equal`` the box rows are redrawn until none is
    tied (``tied_rows``)."""
    g = torch.Generator().manual_seed(seed)
    c = 0.2 + 0.6 * torch.rand(A, 2, generator=g)
    s = 0.05 + 0.35 * torch.rand(A, 2, generator=g)
    anchors = torch.cat((c - s / 2, c + s / 2), dim=1)
    logits = torch.randn(Fr, A, K, generator=g) * 2
    labels = (torch.rand(Fr, A, generator=g) < 0.25).long() * torch.randint(1, K, (Fr, A), generator=g)
    if case == "no_pos":
        labels.zero_()
    idx = torch.arange(Fr * A).reshape(Fr, A)
    mask = (labels > 0).float()
    mask[(labels == 0) & (idx % 5 == 0)] = 1.0
    mask[(labels > 0) & (idx % 7 == 0)] = 0.0
    mask = mask.unsqueeze(-1).repeat(1, 1, 4)
    offset = torch.randn(Fr, A, 4, generator=g) * torch.tensor([1.0, 1.0, 0.5, 0.5]) * mask

    def draw():
        r = torch.rand(Fr, A, 4, generator=g)
        n = torch.randn(Fr, A, 4, generator=g)
        sign = torch.where(r[..., :2] < 0.5, -1.0, 1.0)
        if case == "disjoint":         # the centre moves by 3 .. 5 anchor sides; no side exceeds e^0.45 of the anchor's
            shift = torch.cat((sign * (30.0 + 20.0 * r[..., 2:]), 0.5 * n[..., 2:].clamp(-1, 1)), dim=-1)
        elif case == "pred_contains":  # the centre moves by <= 0.02 sides, the sides grow by 1.5 .. 2
            shift = torch.cat((0.2 * (2 * r[..., :2] - 1), 5 * torch.log(1.5 + 0.5 * r[..., 2:])), dim=-1)
        elif case == "target_contains":
            shift = torch.cat((0.2 * (2 * r[..., :2] - 1), -5 * torch.log(1.5 + 0.5 * r[..., 2:])), dim=-1)
        elif case == "clamped":        # both size offsets 0.5 .. 1.5 beyond the clamp
            shift = torch.cat((n[..., :2], 5 * (EXP_CLAMP + 0.5 + r[..., 2:]) - offset[..., 2:]), dim=-1)
        elif case == "equal":
            shift = torch.zeros(Fr, A, 4)
        else:
            shift = 0.5 * n
        return offset + shift

    bbox = draw()
    if case != "equal":
        for _ in range(20):
            tied = tied_rows(bbox, offset, mask, labels, anchors)
            if not bool(tied.any()):
                break
            bbox = torch.where(tied.unsqueeze(-1), draw(), bbox)
    bbox = torch.where(mask > 0, bbox, torch.randn(Fr, A, 4, generator=g))    # rows without a target: free predictions
    return ExtInputs(logits, bbox, offset, mask, labels, anchors)


def deviation(got_loss, got_g_logits, got_g_bbox, ref: ExtRef, skip_box_rows=False):
    """-> ``(loss, g_logits, g_bbox)`` deviations from the fp64 reference: the loss relative to the reference loss, each
    gradient as the largest elementwise error over the largest reference magnitude of the tensor (0 / 0 = 0: an all-zero
    reference gradient must be met exactly).  ``skip_box_rows``: the box rows of g_bbox are left out (``equal``)."""
    def rel(err, scale):
        return 0.0 if err == 0.0 else (err / scale if scale > 0 else float("inf"))
    d_loss = rel(abs(float(got_loss) - ref.loss), abs(ref.loss))
    e = (got_g_logits.to(F64) - ref.g_logits.to(F64)).abs()
    d_gl = rel(float(e.max()), float(ref.g_logits.abs().max()))
    e = (got_g_bbox.to(F64) - ref.g_bbox.to(F64)).abs()
    r = ref.g_bbox.to(F64).abs()
    if skip_box_rows:
        keep = ~ref.box_rows.unsqueeze(-1).expand_as(e)
        e, r = e[keep], r[keep]
    d_gb = rel(float(e.max()) if e.numel() else 0.0, float(r.max()) if r.numel() else 0.0)
    return d_loss, d_gl, d_gb
