"""Basic object detector class (mirror of the reference's ``models/soda.py``).

Same constructor, hooks and step logic; what differs:

* ``forward`` hands the WHOLE event sequence ``X[T,B,2,H,W]`` to the generated networks, which run
  layer-major on the gfx950 kernels (``generator.py`` here).  ``forward(X, time_outer=True)`` runs the
  reference's literal loop ``for ts in X`` (``soda.py:141-144``) on the same kernels with ``T = 1``;
  both give the same result and the second exists for parity tests and streaming use.
* Lightning / torchmetrics are not dependencies: the class is a plain ``nn.Module`` exposing the
  Lightning hook names (``training_step``, ``configure_optimizers`` ...) so a trainer loop or a
  LightningModule shim can drive it.
* mAP evaluation (``soda.py:160-182, 283-321``) keeps the reference's hooks and keys but runs on the device:
  ``validation_step`` / ``test_step`` hand ``multibox_detection`` of the step's predictions to
  ``metrics.MeanAveragePrecision.update_padded`` (no host synchronisation), ``on_validation_epoch_end`` /
  ``on_test_epoch_end`` log ``map, map_50, mar_1, mar_10, mar_100`` through ``log_dict``.  As in the reference
  (``sync_on_compute=False``) each rank's mAP covers the images that rank saw.
* ``label_steps=K`` trains on every labelled timestep: six-column labels ``(ts, class, x1, y1, x2, y2)`` (the
  reference's ``one_label: false`` sample format, which nothing there consumes) supervise up to ``K`` labelled frames
  per sample instead of the last frame only (DESIGN "Every labelled timestep").
* ``cls_loss`` / ``focal_gamma`` / ``box_loss`` / ``box_loss_weight`` select the objective: focal classification and a
  GIoU / DIoU / CIoU term on the decoded boxes next to the reference's cross entropy + L1, which stays the default and
  runs exactly as before (DESIGN "Detection loss").
* ``assigner`` / ``tal_topk`` / ``tal_alpha`` / ``tal_beta`` select which anchors are positives: ``"iou"`` is the
  reference's static rule (``roi.RoI``), the default, with the same calls and launches as before; ``"tal"`` is the
  task-aligned assigner (``roi.TaskAlignedAssigner``), which reads the detached predictions of the step (DESIGN "Anchor
  assignment").
* ``carry_state=True`` trains on consecutive windows of a recording: the detached detector state of a step is kept (one
  per stage) and handed to the next one, batches may carry ``first[B]`` - the samples that start a new recording, whose
  state ``functional.reset_state_`` puts back to rest on the device (DESIGN "Carried state").
"""

import math
from types import SimpleNamespace
from typing import Optional, Tuple

import torch
from torch import nn
from torch.nn import functional as F

from . import box
from .metrics import AREA_RANGES, MeanAveragePrecision
from .generator import BackboneGen, Head, ListGen, ListState, NeckGen
from .roi import RoI, TaskAlignedAssigner

LOSS_CLS_NAMES = ("ce", "focal")
LOSS_BOX_NAMES = ("l1", "giou", "diou", "ciou")
ASSIGNER_NAMES = ("iou", "tal")
_EXP_CLAMP = math.log(1000.0 / 16.0)   # upper clamp of the exponent argument of a decoded box side
_IOU_EPS = 1e-7


def _decode_corners(anchors: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """``box.offset_inverse`` with the exponent argument clamped above (zero gradient past the clamp)."""
    anc = box.box_corner_to_center(anchors)
    xy = (offsets[:, :2] * anc[:, 2:] / 10) + anc[:, :2]
    wh = torch.exp(torch.clamp(offsets[:, 2:] / 5, max=_EXP_CLAMP)) * anc[:, 2:]
    return box.box_center_to_corner(torch.cat((xy, wh), dim=1))


def iou_box_loss(pred: torch.Tensor, target: torch.Tensor, mode: str) -> torch.Tensor:
    """``1 - IoU + penalty`` per row of corner boxes ``pred[n,4]`` / ``target[n,4]``: GIoU ``(C - U) / C`` of the enclosing
    box, DIoU ``rho^2 / c^2``, CIoU DIoU ``+ alpha v`` (``alpha`` detached); ``eps = 1e-7`` in every denominator."""
    eps = _IOU_EPS
    px1, py1, px2, py2 = pred.unbind(-1)
    gx1, gy1, gx2, gy2 = target.unbind(-1)
    inter = torch.clamp(torch.minimum(px2, gx2) - torch.maximum(px1, gx1), min=0) * \
        torch.clamp(torch.minimum(py2, gy2) - torch.maximum(py1, gy1), min=0)
    union = (px2 - px1) * (py2 - py1) + (gx2 - gx1) * (gy2 - gy1) - inter
    iou = inter / (union + eps)
    cw = torch.maximum(px2, gx2) - torch.minimum(px1, gx1)
    ch = torch.maximum(py2, gy2) - torch.minimum(py1, gy1)
    if mode == "giou":
        area = cw * ch
        return (1 - iou) + (area - union) / (area + eps)
    rho2 = ((px1 + px2) / 2 - (gx1 + gx2) / 2) ** 2 + ((py1 + py2) / 2 - (gy1 + gy2) / 2) ** 2
    pen = rho2 / ((cw * cw + ch * ch) + eps)
    if mode == "ciou":
        v = (4 / math.pi ** 2) * (torch.atan((gx2 - gx1) / ((gy2 - gy1) + eps))
                                  - torch.atan((px2 - px1) / ((py2 - py1) + eps))) ** 2
        alpha = (v / (((1 - iou) + v) + eps)).detach()
        pen = pen + alpha * v
    return (1 - iou) + pen


def detection_loss_host(cls_preds, bbox_preds, bbox_offset, bbox_mask, class_labels, anchors, loss_ratio: float,
                        cls_loss: str = "ce", focal_gamma: float = 2.0, box_loss: str = "l1",
                        box_loss_weight: float = 1.0, valid: Optional[torch.Tensor] = None):
    """The selectable detection loss (``functional.detection_loss_ext`` / ``detection_loss_steps_ext``) as a plain torch
    expression in the dtype of its operands: predictions ``[..., A, C+1]`` / ``[..., A, 4]``, ``anchors[A,4]``, ``valid``
    a boolean per frame (the valid slots; None: every frame).  -> ``(classification term, box term)``; the loss is their
    sum.  Means run over ``max(n, 1)`` rows; no valid frame gives zeros."""
    A, C = anchors.shape[0], cls_preds.shape[-1]
    x, bb = cls_preds.reshape(-1, A, C), bbox_preds.reshape(-1, A, 4)
    off, msk, y = bbox_offset.reshape(-1, A, 4), bbox_mask.reshape(-1, A, 4), class_labels.reshape(-1, A)
    if valid is not None:
        keep = valid.reshape(-1).bool()
        x, bb, off, msk, y = x[keep], bb[keep], off[keep], msk[keep], y[keep]
    V = x.shape[0]
    if V == 0:
        zero = cls_preds.sum() * 0
        return zero, zero
    x, bb, off, msk, y = x.reshape(-1, C), bb.reshape(-1, 4), off.reshape(-1, 4), msk.reshape(-1, 4), y.reshape(-1)
    ce = F.cross_entropy(x, y, reduction="none")
    if cls_loss == "focal":
        p_y = F.softmax(x, dim=1).gather(1, y[:, None])[:, 0]
        ce = (1 - p_y) ** focal_gamma * ce
    pos = y > 0
    n_pos, n_neg = max(int(pos.sum()), 1), max(int((~pos).sum()), 1)
    cls = (ce[pos].sum() / n_pos) * loss_ratio + (ce[~pos].sum() / n_neg) * (1 - loss_ratio)
    if box_loss == "l1":
        return cls, F.l1_loss(bb * msk, off * msk) * box_loss_weight
    rows = pos & (msk == 1).all(dim=1)
    anc = anchors.repeat(V, 1)[rows]
    per_row = iou_box_loss(_decode_corners(anc, bb[rows]), _decode_corners(anc, off[rows]), box_loss)
    return cls, (per_row.sum() / n_pos) * box_loss_weight


class SODa(nn.Module):
    """Base detector; subclasses supply ``backbone_cfgs / neck_cfgs / head_cfgs`` (soda.py:98-133)."""

    def __init__(
        self,
        num_classes: int,
        loss_ratio: float = 0.04,
        time_window: int = 16,
        iou_threshold: float = 0.4,
        learning_rate: float = 0.001,
        state_storage: bool = False,
        init_weights: bool = True,
        plotter=None,
        label_steps: Optional[int] = None,
        cls_loss: str = "ce",
        focal_gamma: float = 2.0,
        box_loss: str = "l1",
        box_loss_weight: float = 1.0,
        map_options: Optional[dict] = None,
        assigner: str = "iou",
        tal_topk: int = 10,
        tal_alpha: float = 1.0,
        tal_beta: float = 6.0,
        carry_state: bool = False,
    ):
        super().__init__()
        if label_steps is not None and not 1 <= int(label_steps) <= 32:
            raise ValueError(f"label_steps must be None or in 1 .. 32, got {label_steps}")
        if cls_loss not in LOSS_CLS_NAMES:
            raise ValueError(f"cls_loss must be one of {LOSS_CLS_NAMES}, got {cls_loss!r}")
        if box_loss not in LOSS_BOX_NAMES:
            raise ValueError(f"box_loss must be one of {LOSS_BOX_NAMES}, got {box_loss!r}")
        if not float(focal_gamma) >= 0.0:
            raise ValueError(f"focal_gamma must be >= 0, got {focal_gamma}")
        if not float(box_loss_weight) >= 0.0:
            raise ValueError(f"box_loss_weight must be >= 0, got {box_loss_weight}")
        if assigner not in ASSIGNER_NAMES:
            raise ValueError(f"assigner must be one of {ASSIGNER_NAMES}, got {assigner!r}")
        if isinstance(tal_topk, bool) or int(tal_topk) != tal_topk or not 1 <= int(tal_topk) <= 64:
            raise ValueError(f"tal_topk must be an integer in 1 .. 64, got {tal_topk}")
        if not (float(tal_alpha) >= 0.0 and math.isfinite(float(tal_alpha))):
            raise ValueError(f"tal_alpha must be finite and >= 0, got {tal_alpha}")
        if not (float(tal_beta) >= 0.0 and math.isfinite(float(tal_beta))):
            raise ValueError(f"tal_beta must be finite and >= 0, got {tal_beta}")
        if carry_state and time_window:
            raise ValueError(f"carry_state=True needs time_window=0, got time_window={time_window}: cutting a random "
                             "prefix off a window would tear the stream the carried state belongs to")
        self.hparams = SimpleNamespace(
            num_classes=num_classes, loss_ratio=loss_ratio, time_window=time_window,
            iou_threshold=iou_threshold, learning_rate=learning_rate, state_storage=state_storage,
            init_weights=init_weights, label_steps=None if label_steps is None else int(label_steps),
            cls_loss=cls_loss, focal_gamma=float(focal_gamma), box_loss=box_loss,
            box_loss_weight=float(box_loss_weight), assigner=assigner, tal_topk=int(tal_topk),
            tal_alpha=float(tal_alpha), tal_beta=float(tal_beta), carry_state=bool(carry_state),
        )
        self.plotter = plotter
        self.logged = {}
        self._sync_logged = set()
        # set by trainer.FlatTrainer.attach(): called in the backward pass when it crosses the backbone / neck boundary
        # (every neck and head gradient is complete or enqueued there) to start their all-reduce early
        self._snn_neck_grads_ready = None
        self._loss_terms = None   # (classification term, box term) of the last loss under a selected objective
        # carry_state=True: stage ("train" / "val" / "test") -> ((B, H, W), detached state tree after the stage's last step);
        # plain attributes - never in state_dict(), never exchanged between ranks
        self._carried = {}

        self.base_net = BackboneGen(self.backbone_cfgs, in_channels=2, init_weights=self.hparams.init_weights)
        self.neck_net = NeckGen(self.neck_cfgs, self.base_net.out_channels, init_weights=self.hparams.init_weights)
        self.head_net = Head(self.head_cfgs, self.hparams.num_classes, self.neck_net.out_shape,
                             init_weights=self.hparams.init_weights)
        self.roi_blk = RoI(self.hparams.iou_threshold)
        # assigner="tal": the positives follow the detached predictions; None: roi_blk alone decides, as before
        self.tal_blk = (TaskAlignedAssigner(self.hparams.tal_topk, self.hparams.tal_alpha, self.hparams.tal_beta)
                        if assigner == "tal" else None)
        self.cls_loss = nn.CrossEntropyLoss(reduction="none")
        self.box_loss = nn.L1Loss(reduction="none")
        # soda.py:89-96; a plain attribute, not a submodule: state_dict() is unchanged
        # map_options: keyword arguments of metrics.MeanAveragePrecision (area_ranges, class_metrics, min_box_diag, ...)
        self.map_metric = MeanAveragePrecision(self.hparams.num_classes, **(map_options or {}))

    # ------------------------------------------------------------------ description hooks
    def backbone_cfgs(self) -> ListGen:
        raise NotImplementedError

    def neck_cfgs(self) -> ListGen:
        raise NotImplementedError

    def head_cfgs(self, box_out: int, cls_out: int) -> ListGen:
        raise NotImplementedError

    # ------------------------------------------------------------------ optimisation
    def configure_optimizers(self) -> torch.optim.Optimizer:
        return torch.optim.Adamax(self.parameters(), lr=self.hparams.learning_rate)

    def log(self, name, value, sync_dist: bool = False, **kwargs) -> None:
        """Lightning's ``self.log`` reduced to a dict.  ``sync_dist=True`` (every loss the reference logs,
        ``soda.py:151-157``) marks the entry for the cross-rank mean, which ``synced_logs()`` takes with ONE all-reduce
        over all marked entries when the values are actually read - not one collective per logged value per step."""
        self.logged[name] = value.detach() if isinstance(value, torch.Tensor) else value
        if sync_dist:
            self._sync_logged.add(name)

    def log_dict(self, dictionary, sync_dist: bool = False, **kwargs) -> None:
        """Lightning's ``self.log_dict``: ``log`` for every entry."""
        for name, value in dictionary.items():
            self.log(name, value, sync_dist=sync_dist, **kwargs)

    def synced_logs(self, process_group=None) -> dict:
        """The logged values with the ``sync_dist`` entries averaged over the ranks (Lightning's reduction)."""
        import torch.distributed as dist
        out = dict(self.logged)
        names = sorted(n for n in self._sync_logged if isinstance(out.get(n), torch.Tensor))
        if names and dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1:
            flat = torch.stack([out[n].float().reshape(()) for n in names])
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=process_group)
            flat = flat / dist.get_world_size(process_group)
            for k, n in enumerate(names):
                out[n] = flat[k]
        return out

    # ------------------------------------------------------------------ forward
    def forward(self, X: torch.Tensor, time_outer: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``X[T,B,2,H,W]`` -> ``(anchors[A,4], cls_preds[B,A,C+1], bbox_preds[B,A,4])`` of the last step."""
        if time_outer:
            state = None
            for ts in X:
                preds, state = self._forward_impl(ts, state)
            return preds
        preds, _ = self._forward_impl(X, None)
        return preds

    def _forward_impl(self, X: torch.Tensor, state: Optional[ListState], all_steps: bool = False,
                      steps: Optional[torch.Tensor] = None):
        from . import functional as HF
        state = [None] * 3 if state is None else state
        HF.begin_counter_batch()
        try:
            base_out, state[0] = self.base_net.forward(X, state[0])
            if self._snn_neck_grads_ready is not None and base_out.dim() == 5:
                base_out = HF.grad_ready_hook(base_out, self._snn_neck_grads_ready)
            neck_out, state[1] = self.neck_net.forward(base_out, state[1])
            anchors, cls_preds, bbox_preds, state[2] = self.head_net.forward(neck_out, state[2], all_steps=all_steps,
                                                                                 steps=steps)
        finally:
            HF.flush_counter_batch()
        return (anchors, cls_preds, bbox_preds), state

    # ------------------------------------------------------------------ steps
    def _step(self, batch: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        if batch[1].shape[-1] == 6:
            return self._step_labelled_frames(batch)[0]
        X, labels = batch[0][self._rand_start_time():], batch[1]
        preds = self.forward(X)
        return self._loss(preds, labels)

    def _default_loss(self) -> bool:
        """The reference's objective (cross entropy + L1): the steps then call exactly ``detection_loss`` /
        ``detection_loss_steps`` and log the reference's keys."""
        return self.hparams.cls_loss == "ce" and self.hparams.box_loss == "l1" and self.hparams.box_loss_weight == 1.0

    def _loss_options(self) -> dict:
        hp = self.hparams
        return dict(cls_loss=hp.cls_loss, focal_gamma=hp.focal_gamma, box_loss=hp.box_loss,
                    box_loss_weight=hp.box_loss_weight)

    def _log_loss(self, stage: str, loss: torch.Tensor, batch) -> None:
        """``<stage>_loss`` as the reference logs it; with a selected objective also its two terms (device scalars)."""
        kw = {"prog_bar": True} if stage == "train" else {}
        self.log(f"{stage}_loss", loss, batch_size=batch[0].shape[1], sync_dist=True, **kw)
        if self._loss_terms is not None:
            self.log(f"{stage}_loss_cls", self._loss_terms[0], batch_size=batch[0].shape[1], sync_dist=True)
            self.log(f"{stage}_loss_box", self._loss_terms[1], batch_size=batch[0].shape[1], sync_dist=True)

    def _step_labelled_frames(self, batch: Tuple[torch.Tensor, torch.Tensor], carry: Optional[list] = None):
        """Six-column labels ``(ts, class, x1, y1, x2, y2)``: the loss over every labelled frame the ``label_steps`` slots
        hold.  The random prefix ``t0`` is cut from the frames and subtracted from the rows' timesteps alike; the frames
        are chosen on the device (``steps[K,B]``), so the step stays free of host synchronisation.
        ``carry`` (``carry_state=True``): a one-element list holding the state the window starts from; the state after the
        window replaces it.
        -> ``(loss, preds of the K*B frames, steps, t0)``"""
        from . import functional as HF
        K = self.hparams.label_steps
        if K is None:
            raise ValueError("labels with six columns (ts, class, x1, y1, x2, y2) need the constructor keyword "
                             "label_steps (the number of labelled frames kept per sample)")
        t0 = self._rand_start_time()
        X, labels = batch[0][t0:], batch[1]
        if X.dim() != 5:
            raise ValueError(f"six-column labels need a sequence X[T,B,2,H,W], got a tensor of rank {X.dim()}")
        T = X.shape[0]
        if K > T:
            raise ValueError(f"label_steps = {K} exceeds the {T} timesteps left of the sequence")
        labels = labels.to(X.device)
        steps = HF.select_label_steps(labels, T, K, t0)
        preds, state = self._forward_impl(X, None if carry is None else carry[0], steps=steps)
        if carry is not None:
            carry[0] = state
        anchors, cls_preds, bbox_preds = preds
        if self.tal_blk is not None:
            bbox_offset, bbox_mask, class_labels = self.tal_blk.steps(anchors, labels, steps, t0, cls_preds.detach(),
                                                                      bbox_preds.detach())
        else:
            bbox_offset, bbox_mask, class_labels = self.roi_blk.steps(anchors, labels, steps, t0)
        if self._default_loss():
            loss = HF.detection_loss_steps(cls_preds, bbox_preds, bbox_offset, bbox_mask, class_labels, steps,
                                           self.hparams.loss_ratio)
        else:
            loss, *self._loss_terms = HF.detection_loss_steps_ext(
                cls_preds, bbox_preds, bbox_offset, bbox_mask, class_labels, anchors, steps, self.hparams.loss_ratio,
                return_terms=True, **self._loss_options())
        return loss, preds, steps, t0

    def _eval_labelled_frames(self, batch: Tuple[torch.Tensor, torch.Tensor], carry: Optional[list] = None) -> torch.Tensor:
        """``validation_step`` / ``test_step`` on six-column labels: the loss as in training, and mAP over exactly the
        valid slots - every labelled frame is one image, with the label rows of its own timestep.  Device ``where`` only."""
        loss, preds, steps, t0 = self._step_labelled_frames(batch, carry)
        anchors, cls_preds, bbox_preds = (p.detach() for p in preds)
        labels = batch[1].to(cls_preds.device).float()
        K, B, A = cls_preds.shape[:3]
        dets = box.multibox_detection_batched(F.softmax(cls_preds.reshape(K * B, A, -1), dim=2),
                                              bbox_preds.reshape(K * B, A, 4), anchors)
        dets[..., 2:] = torch.clamp(dets[..., 2:], min=0.0, max=1.0)     # the boxes predict_sequence reports
        valid = (steps >= 0).reshape(K * B, 1)
        dets[..., 0] = torch.where(valid, dets[..., 0], torch.full_like(dets[..., 0], -1.0))
        # rows [K*B, N, 5]: the real rows of the slot's own timestep, -1 everywhere else
        own = (labels[None, :, :, 1] >= 0) & (labels[None, :, :, 0] - float(t0) == steps[:, :, None].float()) \
            & (steps[:, :, None] >= 0)
        rows = torch.where(own.unsqueeze(-1), labels[None, :, :, 1:].expand(K, -1, -1, -1),
                           torch.full((), -1.0, device=labels.device))
        self.map_metric.update_padded(dets, rows.reshape(K * B, labels.shape[1], 5), image_size=batch[0].shape[-2:])
        return loss

    def reset_carried_state(self, stage: Optional[str] = None) -> None:
        """Drop the state kept by ``carry_state=True`` for ``stage`` (``"train"``, ``"val"``, ``"test"``; None: all): the
        stage's next step starts every layer from rest."""
        if stage is None:
            self._carried.clear()
        elif stage not in ("train", "val", "test"):
            raise ValueError(f'reset_carried_state: stage must be "train", "val", "test" or None, got {stage!r}')
        else:
            self._carried.pop(stage, None)

    def _carried_step(self, stage: str, batch) -> torch.Tensor:
        """A step of ``carry_state=True`` on ``(X, labels)`` or ``(X, labels, first)``: the window starts from the state the
        stage's last step ended in - with the samples ``first[b] != 0`` (int32 ``[B]``, device) back at rest - and the
        detached state after the window is kept.  No gradient crosses the boundary.  A batch of another ``B`` or frame
        size than the kept one starts from rest."""
        from . import functional as HF
        X, labels = batch[0], batch[1]
        first = batch[2] if len(batch) > 2 else None
        if X.dim() != 5:
            raise ValueError(f"carry_state=True needs a sequence X[T,B,2,H,W], got a tensor of rank {X.dim()}")
        key = (int(X.shape[1]), int(X.shape[-2]), int(X.shape[-1]))
        if first is not None and tuple(first.shape) != (key[0],):
            raise ValueError(f"carry_state=True: first must be int32 [B = {key[0]}], got shape {tuple(first.shape)}")
        kept = self._carried.pop(stage, None)
        state = None
        if kept is not None and kept[0] == key:
            state = kept[1] if first is None else HF.reset_state_(kept[1], first.to(X.device))
        carry, pair = [state], (X, labels)
        if labels.shape[-1] == 6:
            if stage == "train":
                loss = self._step_labelled_frames(pair, carry)[0]
            else:
                loss = self._eval_labelled_frames(pair, carry)
        else:
            preds, carry[0] = self._forward_impl(X, state)
            loss = self._loss(preds, labels)
            if stage != "train":
                self._map_estimate(preds, labels, X.shape[-2:])
        self._carried[stage] = (key, HF.detach_state(carry[0]))
        self._log_loss(stage, loss, pair)
        return loss

    def training_step(self, batch: Tuple[torch.Tensor, torch.Tensor], batch_idx: int = 0) -> torch.Tensor:
        if self.hparams.carry_state:
            return self._carried_step("train", batch)
        loss = self._step(batch)
        self._log_loss("train", loss, batch)
        return loss

    def validation_step(self, batch: Tuple[torch.Tensor, torch.Tensor], batch_idx: int = 0) -> torch.Tensor:
        if self.hparams.carry_state:
            return self._carried_step("val", batch)
        if batch[1].shape[-1] == 6:
            loss = self._eval_labelled_frames(batch)
            self._log_loss("val", loss, batch)
            return loss
        preds = self.forward(batch[0][self._rand_start_time():])
        loss = self._loss(preds, batch[1])
        self._log_loss("val", loss, batch)
        self._map_estimate(preds, batch[1], batch[0].shape[-2:])
        return loss

    def on_validation_epoch_end(self) -> None:
        self._map_compute()

    def test_step(self, batch: Tuple[torch.Tensor, torch.Tensor], batch_idx: int = 0) -> torch.Tensor:
        if self.hparams.carry_state:
            return self._carried_step("test", batch)
        if batch[1].shape[-1] == 6:
            loss = self._eval_labelled_frames(batch)
            self._log_loss("test", loss, batch)
            return loss
        preds = self.forward(batch[0][self._rand_start_time():])
        loss = self._loss(preds, batch[1])
        self._log_loss("test", loss, batch)
        self._map_estimate(preds, batch[1], batch[0].shape[-2:])
        return loss

    def on_test_epoch_end(self) -> None:
        self._map_compute()

    def _map_estimate(self, preds: Tuple[torch.Tensor, torch.Tensor, torch.Tensor], labels: torch.Tensor,
                      image_size=None) -> None:
        # soda.py:294-321 without the per-image boolean masks: padded rows (class -1) are skipped by the kernels
        anchors, cls_preds, bbox_preds = (p.detach() for p in preds)
        dets = box.multibox_detection(F.softmax(cls_preds, dim=2), bbox_preds, anchors)
        self.map_metric.update_padded(dets, labels, image_size=image_size)

    def _map_compute(self) -> None:
        # soda.py:283-292
        result = self.map_metric.compute()
        self.log_dict({k: result[k] for k in ("map", "map_50", "mar_1", "mar_10", "mar_100")})
        # beyond the reference, only what map_options selected (device scalars; no host read)
        self.log_dict({k: v for k, v in result.items() if k.rsplit("_", 1)[-1] in AREA_RANGES})
        if "map_per_class" in result:
            ar = result[f"mar_{self.map_metric.max_detection_thresholds[-1]}_per_class"]
            for c in range(self.hparams.num_classes):
                self.log_dict({f"map_class_{c}": result["map_per_class"][c], f"mar_class_{c}": ar[c]})
        self.map_metric.reset()

    def predict(self, X: torch.Tensor, state: Optional[ListState]) -> Tuple[torch.Tensor, ListState]:
        """Streaming inference for one event frame ``X[2,H,W]`` (soda.py:202-233).

        Returns rows ``(class id, confidence, x1, y1, x2, y2)`` and the new detector state.
        """
        preds, state = self._forward_impl(X.unsqueeze(0), state)
        anchors, cls, bbox = preds
        prep_pred = box.multibox_detection(F.softmax(cls, dim=2), bbox, anchors).squeeze(0)
        prep_pred = prep_pred[prep_pred[:, 0] >= 0]
        prep_pred[:, 2:] = torch.clamp(prep_pred[:, 2:], min=0.0, max=1.0)
        return prep_pred, state

    def predict_sequence(self, X: torch.Tensor, state: Optional[ListState] = None,
                         skip: int = 0) -> Tuple[torch.Tensor, ListState]:
        """Detections of EVERY timestep of a clip (or of a window of a live stream) from one pass.

        ``X`` is ``[T,2,H,W]`` (one stream, the frames ``predict`` takes one by one) or ``[T,B,2,H,W]``.  The network runs
        once, layer-major, over the sequence; softmax, decode and NMS run once over all ``T*B`` frames.  Returns
        ``(dets, state)`` with ``dets[T,A,6]`` / ``dets[T,B,A,6]`` rows ``(class id, confidence, x1, y1, x2, y2)``, boxes
        clamped to ``[0,1]``, and the detector state after the last timestep: ``predict_sequence(X[:k])`` followed by
        ``predict_sequence(X[k:], state)`` continues the stream as ``predict`` does frame by frame.

        The result is padded: the rows ``predict`` drops (suppressed, background, below the confidence threshold) are
        present with class -1, because dropping them needs their number on the host.  ``dets[t][dets[t][:, 0] >= 0]`` are
        the rows ``predict`` returns for timestep ``t``, in the same order; ``metrics.MeanAveragePrecision.update_padded``
        takes the padded form as it is.  The first ``skip`` timesteps get class -1 in every row (the reference's
        ``idx < time_window`` rule of ``predict_step``: the detector is still warming up).
        """
        if X.dim() not in (4, 5):
            raise ValueError(f"predict_sequence takes X[T,2,H,W] or X[T,B,2,H,W], got a tensor of rank {X.dim()}")
        if self.training:
            raise RuntimeError("predict_sequence needs eval mode: a train-mode BatchNorm would normalise every timestep "
                               "with the statistics of the whole clip")
        single = X.dim() == 4
        with torch.no_grad():
            preds, state = self._forward_impl(X.unsqueeze(1) if single else X, state, all_steps=True)
            anchors, cls, bbox = preds
            T, B, A = cls.shape[:3]
            dets = box.multibox_detection_batched(F.softmax(cls.reshape(T * B, A, -1), dim=2),
                                                  bbox.reshape(T * B, A, 4), anchors).reshape(T, B, A, 6)
            dets[..., 2:] = torch.clamp(dets[..., 2:], min=0.0, max=1.0)
            if skip > 0:
                dets[:skip, ..., 0] = -1.0
        return (dets[:, 0] if single else dets), state

    def _rand_start_time(self) -> int:
        # soda.py:246-257: drop a random prefix of the sequence; the SAME draw (``requires_grad=False``,
        # ``dtype=torch.uint32``: a seeded run consumes the generator exactly as the reference does)
        if not self.hparams.time_window:
            return 0
        return int(torch.randint(0, self.hparams.time_window, (1,), requires_grad=False, dtype=torch.uint32).item())

    def _loss(self, preds: Tuple[torch.Tensor, torch.Tensor, torch.Tensor], labels: torch.Tensor) -> torch.Tensor:
        # soda.py:259-281
        anchors, cls_preds, bbox_preds = preds
        if self.tal_blk is not None:
            bbox_offset, bbox_mask, class_labels = self.tal_blk(anchors, labels, cls_preds.detach(), bbox_preds.detach())
        else:
            bbox_offset, bbox_mask, class_labels = self.roi_blk(anchors, labels)
        if not self._default_loss():
            if cls_preds.is_cuda:   # the same launches as below (csrc/det_loss.hip)
                from . import functional as HF
                loss, *self._loss_terms = HF.detection_loss_ext(
                    cls_preds, bbox_preds, bbox_offset, bbox_mask, class_labels, anchors, self.hparams.loss_ratio,
                    return_terms=True, **self._loss_options())
                return loss
            t_cls, t_box = detection_loss_host(cls_preds, bbox_preds, bbox_offset, bbox_mask, class_labels, anchors,
                                               self.hparams.loss_ratio, **self._loss_options())
            self._loss_terms = [t_cls.detach(), t_box.detach()]
            return t_cls + t_box
        if cls_preds.is_cuda:
            # one launch for the anchor targets (RoI above), two for the loss, one for its gradient (csrc/det_loss.hip)
            from . import functional as HF
            return HF.detection_loss(cls_preds, bbox_preds, bbox_offset, bbox_mask, class_labels,
                                     self.hparams.loss_ratio)
        _, _, num_classes = cls_preds.shape
        cls = self.cls_loss.forward(cls_preds.reshape(-1, num_classes), class_labels.reshape(-1))
        bbox = self.box_loss.forward(bbox_preds * bbox_mask, bbox_offset * bbox_mask)
        mask = class_labels.reshape(-1) > 0
        gt_loss = cls[mask].mean()
        background_loss = cls[~mask].mean()
        return (gt_loss * self.hparams.loss_ratio + background_loss * (1 - self.hparams.loss_ratio) + bbox.mean())

    def activity_report(self, X: torch.Tensor, state: Optional[ListState] = None, per_step: bool = False,
                        process_group=None) -> dict:
        """Firing rates of every LIF layer and the synaptic operations of every convolution over the clip ``X[T,B,2,H,W]``
        (``activity.make_report``): one eval-mode, ``no_grad``, layer-major pass under ``activity.record``, continuing from
        ``state`` when given.  ``per_step``: the LIF counts per timestep."""
        from . import activity
        if X.dim() != 5:
            raise ValueError(f"activity_report takes X[T,B,2,H,W], got a tensor of rank {X.dim()}")
        if self.training:
            raise RuntimeError("activity_report needs eval mode (model.eval()); a training step is recorded with "
                               "`with activity.record(model) as rec: model.training_step(batch)`")
        with torch.no_grad(), activity.record(self, per_step=per_step) as rec:
            self._forward_impl(X, state)
        return rec.report(process_group)

    def spike_taps(self):
        """``{module path: spikes[T,B,C,h,w]}`` of every ``StateStorage`` (``state_storage=True``, eval mode)."""
        from .layer_gen import StateStorage
        return {name: m.get_spikes() for name, m in self.named_modules()
                if isinstance(m, StateStorage) and m.spike_list}
