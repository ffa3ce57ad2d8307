"""The detection losses (``csrc/det_loss.hip``) and the labelled-timestep selection / gather that feed them."""

from typing import Optional, Tuple

import torch
from torch.autograd import Function

from . import _hip
from ._layout import _F32, _new_cl, _ptr, _raw_to_cl, _require_device, _stream, cl_stride


def _loss_entry(ptrs, anc, steps, dims, ratio, modes):
    """The C entry family of ``csrc/det_loss.hip`` a call goes through, by its shape ->
    ``(symbol stem, doubles of stats, workspace-size arguments, leading call arguments)``."""
    rows, A, C = dims
    if modes is not None:      # selectable objective: means over max(n, 1) rows; stats = totals, V, the three terms
        return "snn_det_loss_ext", 9, (rows,), ptrs + [_ptr(anc), _ptr(steps), rows, A, C, ratio, *modes]
    if steps is not None:      # the reference's objective over K x B slots: means as they are (NaN); stats = totals, V
        K, B = steps.shape
        return "snn_det_loss_steps", 6, (K, B, A), ptrs + [steps.data_ptr(), K, B, A, C, ratio]
    return "snn_det_loss", 5, (rows,), ptrs + [rows, C, ratio]   # ... over all rows; stats = totals


class _DetectionLoss(Function):
    """The detection loss and its gradient (``csrc/det_loss.hip``): two kernel launches forward, one backward, no host
    round trip.  ``modes`` None: ``loss_ratio * mean(CE[pos]) + (1 - loss_ratio) * mean(CE[neg]) + mean(L1(bbox*mask,
    offset*mask))`` (models/soda.py:259-281), NaN for an empty class; ``modes`` from ``check_loss_options`` (``anchors``
    required): a selectable classification term (cross entropy | focal) and box term (L1 | GIoU | DIoU | CIoU), 0 for an
    empty class.  ``steps`` None or ``[K,B]``: over the anchors of the valid slots only (``steps[k][b] >= 0``); their
    number ``V`` is counted on the device, ``V = 0`` gives loss 0 and the gradients of empty slots are exact zeros.
    Returns the loss and ``stats``; with ``modes`` its last three entries are the terms of the loss."""

    @staticmethod
    def forward(ctx, cls_preds, bbox_preds, bbox_offset, bbox_mask, class_labels, anchors, steps, loss_ratio: float,
                modes: Optional[Tuple[int, float, int, float]]):
        who = "detection_loss_steps" if modes is None else "detection_loss_steps_ext"
        _require_device(cls_preds, "loss: class predictions")
        _require_device(bbox_preds, "loss: box predictions")
        # the targets and anchors go to the kernel as raw pointers: a host or float64 tensor would be a wild address
        _require_device(bbox_offset, "loss: box offsets")
        _require_device(bbox_mask, "loss: box mask")
        others = [(bbox_preds, "box predictions"), (bbox_offset, "box offsets"), (bbox_mask, "box mask"),
                  (class_labels, "class labels")]
        if modes is not None:
            _require_device(anchors, "loss: anchors")
            others.append((anchors, "anchors"))
        for t, what in others:
            if t.device != cls_preds.device:
                raise RuntimeError(f"loss: {what} are on {t.device}, the class predictions on {cls_preds.device}")
        A, anc = 1, None   # (without anchors and steps every row is a frame of its own)
        if modes is not None:
            if anchors.dim() != 2 or anchors.shape[1] != 4 or cls_preds.dim() < 2 or cls_preds.shape[-2] != anchors.shape[0]:
                raise RuntimeError(f"detection loss: anchors [A,4] and class predictions [..., A, C+1] required, got "
                                   f"{tuple(anchors.shape)} and {tuple(cls_preds.shape)}")
            A, anc = int(anchors.shape[0]), anchors.detach().contiguous()
        Ks = None
        if steps is not None:
            if cls_preds.dim() != 4:
                raise RuntimeError(f"{who}: class predictions [K,B,A,C+1] required")
            A = int(cls_preds.shape[2])
            Ks, steps = _require_steps(steps, int(cls_preds.shape[1]), cls_preds, who)
        C = int(cls_preds.shape[-1])
        logits, boxes = cls_preds.detach().contiguous(), bbox_preds.detach().contiguous()
        off, msk = bbox_offset.contiguous(), bbox_mask.contiguous()
        lab = class_labels.contiguous()
        rows = lab.numel()
        with_steps = "detection loss: predictions, targets and steps differ in shape"
        if (modes is not None and rows == 0) or logits.numel() != rows * C or boxes.numel() != rows * 4 or \
                off.numel() != rows * 4 or msk.numel() != rows * 4 or lab.dtype != torch.int64:
            raise RuntimeError(with_steps if Ks is not None and modes is None else
                               "detection loss: predictions and targets differ in shape")
        if Ks is not None and Ks != cls_preds.shape[0]:
            raise RuntimeError(with_steps)
        dev = logits.device
        ctx.args = ((rows, A, C), float(loss_ratio), modes)
        entry, n_stats, size_args, head = _loss_entry([t.data_ptr() for t in (logits, boxes, off, msk, lab)], anc, steps,
                                                      *ctx.args)
        ws = torch.empty(_hip.query(entry + "_workspace_size", *size_args), device=dev, dtype=torch.uint8)
        stats = torch.empty(n_stats, device=dev, dtype=torch.float64)
        loss = torch.empty((), device=dev, dtype=_F32)
        _hip.call(entry + "_fwd", *head, ws.data_ptr(), stats.data_ptr(), loss.data_ptr(), _stream())
        ctx.optional = (anc is not None, steps is not None)
        ctx.save_for_backward(logits, boxes, off, msk, lab, stats, *(t for t in (anc, steps) if t is not None))
        ctx.shapes = (cls_preds.shape, bbox_preds.shape)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, g, _g_stats):
        logits, boxes, off, msk, lab, stats, *rest = ctx.saved_tensors
        anc = rest.pop(0) if ctx.optional[0] else None
        steps = rest.pop(0) if ctx.optional[1] else None
        g = g.detach().to(_F32).contiguous()
        g_logits, g_boxes = torch.empty_like(logits), torch.empty_like(boxes)
        entry, _, _, head = _loss_entry([t.data_ptr() for t in (logits, boxes, off, msk, lab)], anc, steps, *ctx.args)
        _hip.call(entry + "_bwd", *head, stats.data_ptr(), g.data_ptr(), g_logits.data_ptr(), g_boxes.data_ptr(), _stream())
        return (g_logits.view(ctx.shapes[0]), g_boxes.view(ctx.shapes[1])) + (None,) * 7


def detection_loss(cls_preds: torch.Tensor, bbox_preds: torch.Tensor, bbox_offset: torch.Tensor,
                   bbox_mask: torch.Tensor, class_labels: torch.Tensor, loss_ratio: float) -> torch.Tensor:
    """``loss_ratio * mean(CE[pos]) + (1 - loss_ratio) * mean(CE[neg]) + mean(L1(bbox*mask, offset*mask))``
    (models/soda.py:259-281); a sample set without positives (or negatives) gives NaN, as the reference."""
    return _DetectionLoss.apply(cls_preds, bbox_preds, bbox_offset, bbox_mask, class_labels, None, None, loss_ratio, None)[0]


# ------------------------------------------------------------------------------------------- every labelled timestep
MAX_LABEL_STEPS = 32   # frame slots per sample the *_steps kernels take (kMaxLabelSteps of csrc/snn_common.h)


def _require_steps(steps: torch.Tensor, B: int, like: torch.Tensor, what: str) -> Tuple[int, torch.Tensor]:
    """``steps[K,B]`` as the kernels read it: int32, on ``like``'s device, contiguous.  Returns ``(K, steps)``."""
    if steps.dim() != 2 or steps.shape[1] != B or steps.dtype != torch.int32 or steps.device != like.device:
        raise RuntimeError(f"{what}: steps must be an int32 [K, {B}] tensor on {like.device}, got {steps.dtype} "
                           f"{tuple(steps.shape)} on {steps.device}")
    return int(steps.shape[0]), steps.contiguous()


def select_label_steps(labels: torch.Tensor, T: int, K: int, t0: int = 0) -> torch.Tensor:
    """The labelled frames of a batch, chosen on the device: ``labels[B,N,6]`` rows ``(ts, class, x1, y1, x2, y2)`` (``ts``
    counts the steps of the uncut sequence, padding rows are -1) -> ``steps[K,B]`` int32.  For every sample the latest
    ``K`` distinct steps ``ts - t0`` of its real rows that lie inside the cut sequence ``[0, T)``, in ascending order from
    slot 0; unused slots hold -1.  One launch, no host synchronisation."""
    if not labels.is_cuda or labels.dim() != 3 or labels.shape[2] != 6:
        raise RuntimeError(f"select_label_steps: labels[B,N,6] on a HIP device required, got {tuple(labels.shape)} on "
                           f"{labels.device}")
    lab = labels.detach().float().contiguous()
    B, N, _ = lab.shape
    if N == 0:
        return torch.full((int(K), B), -1, device=lab.device, dtype=torch.int32)
    steps = torch.empty((int(K), B), device=lab.device, dtype=torch.int32)
    _hip.call("snn_label_steps", lab.data_ptr(), B, N, int(T), int(K), int(t0), steps.data_ptr(), _stream())
    return steps


class _GatherSteps(Function):
    """``Y[T,B,C,H,W] -> out[K,B,C,H,W]`` with ``out[k][b] = Y[steps[k][b]][b]`` (zeros for an empty slot); the backward
    writes every frame of the gradient in one pass (zeros where no slot selected the frame)."""

    @staticmethod
    def forward(ctx, Y, steps):
        _require_device(Y, "gather_steps")
        Y = _raw_to_cl(Y)
        T, B, C, H, W = Y.shape
        K, steps = _require_steps(steps, B, Y, "gather_steps")
        out = _new_cl((K, B), C, H, W, Y)
        _hip.call("snn_gather_steps_fwd", Y.data_ptr(), cl_stride(Y), steps.data_ptr(), out.data_ptr(), C, T, B, K, H * W,
                  C, _stream())
        ctx.save_for_backward(steps)
        ctx.dims = (T, B, C, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        (steps,) = ctx.saved_tensors
        T, B, C, H, W = ctx.dims
        g = _raw_to_cl(g)
        gY = _new_cl((T, B), C, H, W, g)
        _hip.call("snn_gather_steps_bwd", g.data_ptr(), cl_stride(g), steps.data_ptr(), gY.data_ptr(), C, T, B,
                  int(steps.shape[0]), H * W, C, _stream())
        return gY, None


def gather_steps(Y: torch.Tensor, steps: torch.Tensor) -> torch.Tensor:
    """The frames ``steps[K,B]`` names (``select_label_steps``) out of a sequence ``Y[T,B,C,H,W]`` - dense or an aliased
    channel slice of a wider channels-last buffer - as a dense channels-last ``[K,B,C,H,W]``."""
    if Y.dim() != 5:
        raise RuntimeError(f"gather_steps takes a sequence Y[T,B,C,H,W], got a tensor of rank {Y.dim()}")
    return _GatherSteps.apply(Y, steps)


def detection_loss_steps(cls_preds: torch.Tensor, bbox_preds: torch.Tensor, bbox_offset: torch.Tensor,
                         bbox_mask: torch.Tensor, class_labels: torch.Tensor, steps: torch.Tensor,
                         loss_ratio: float) -> torch.Tensor:
    """``detection_loss`` of ``cls_preds[K,B,A,C+1]`` / ``bbox_preds[K,B,A,4]`` over the valid slots of ``steps[K,B]``:
    ``r mean(CE[pos]) + (1 - r) mean(CE[neg]) + sum |bbox m - off m| / (4 A V)``."""
    if steps is None:
        raise RuntimeError("detection_loss_steps: steps[K,B] required")
    return _DetectionLoss.apply(cls_preds, bbox_preds, bbox_offset, bbox_mask, class_labels, None, steps, loss_ratio, None)[0]


# ------------------------------------------------------------------------------------------- selectable detection loss
def check_loss_options(cls_loss: str, focal_gamma: float, box_loss: str, box_loss_weight: float) -> Tuple[int, float, int, float]:
    """The loss options by name -> ``(cls_mode, gamma, box_mode, box_weight)`` as the kernels take them, or ``ValueError``."""
    if cls_loss not in _hip.LOSS_CLS_MODES:
        raise ValueError(f"cls_loss must be one of {sorted(_hip.LOSS_CLS_MODES)}, got {cls_loss!r}")
    if box_loss not in _hip.LOSS_BOX_MODES:
        raise ValueError(f"box_loss must be one of {sorted(_hip.LOSS_BOX_MODES)}, got {box_loss!r}")
    if not float(focal_gamma) >= 0.0:
        raise ValueError(f"focal_gamma must be >= 0, got {focal_gamma}")
    if not float(box_loss_weight) >= 0.0:
        raise ValueError(f"box_loss_weight must be >= 0, got {box_loss_weight}")
    return _hip.LOSS_CLS_MODES[cls_loss], float(focal_gamma), _hip.LOSS_BOX_MODES[box_loss], float(box_loss_weight)


def _loss_ext(cls_preds, bbox_preds, bbox_offset, bbox_mask, class_labels, anchors, steps, loss_ratio, cls_loss,
              focal_gamma, box_loss, box_loss_weight, return_terms):
    modes = check_loss_options(cls_loss, focal_gamma, box_loss, box_loss_weight)
    loss, stats = _DetectionLoss.apply(cls_preds, bbox_preds, bbox_offset, bbox_mask, class_labels, anchors, steps,
                                       loss_ratio, modes)
    if not return_terms:
        return loss
    terms = stats[6:9].to(_F32)       # the kernel's own fp32 terms: (terms[0] + terms[1]) + terms[2] is the loss, bit for bit
    return loss, terms[0] + terms[1], terms[2]


def detection_loss_ext(cls_preds: torch.Tensor, bbox_preds: torch.Tensor, bbox_offset: torch.Tensor,
                       bbox_mask: torch.Tensor, class_labels: torch.Tensor, anchors: torch.Tensor, loss_ratio: float,
                       cls_loss: str = "ce", focal_gamma: float = 2.0, box_loss: str = "l1",
                       box_loss_weight: float = 1.0, return_terms: bool = False):
    """``detection_loss`` with a selectable objective: ``cls_loss`` ``"ce"`` or ``"focal"`` (``(1 - p_y)^gamma ce``, same
    ``loss_ratio`` weighting, means over ``max(n, 1)`` rows), ``box_loss`` ``"l1"`` (the term of ``detection_loss``) or
    ``"giou" | "diou" | "ciou"`` of the boxes decoded from ``anchors[A,4]`` with the predicted and the target offsets,
    summed over the positive rows and divided by ``max(n_pos, 1)``; the box term is scaled by ``box_loss_weight``.
    ``return_terms``: ``(loss, classification term, box term)`` - device scalars, ``loss`` is their fp32 sum."""
    return _loss_ext(cls_preds, bbox_preds, bbox_offset, bbox_mask, class_labels, anchors, None, loss_ratio, cls_loss,
                     focal_gamma, box_loss, box_loss_weight, return_terms)


def detection_loss_steps_ext(cls_preds: torch.Tensor, bbox_preds: torch.Tensor, bbox_offset: torch.Tensor,
                             bbox_mask: torch.Tensor, class_labels: torch.Tensor, anchors: torch.Tensor,
                             steps: torch.Tensor, loss_ratio: float, cls_loss: str = "ce", focal_gamma: float = 2.0,
                             box_loss: str = "l1", box_loss_weight: float = 1.0, return_terms: bool = False):
    """``detection_loss_ext`` of ``cls_preds[K,B,A,C+1]`` / ``bbox_preds[K,B,A,4]`` over the valid slots of ``steps[K,B]``
    (their number ``V`` is counted on the device; the L1 term divides by ``4 A V``); no valid slot: loss 0, zero gradients."""
    if steps is None:
        raise RuntimeError("detection_loss_steps_ext: steps[K,B] required")
    return _loss_ext(cls_preds, bbox_preds, bbox_offset, bbox_mask, class_labels, anchors, steps, loss_ratio, cls_loss,
                     focal_gamma, box_loss, box_loss_weight, return_terms)
