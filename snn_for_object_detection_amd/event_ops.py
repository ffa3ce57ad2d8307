"""Event scatter into frames (plain, augmented, packed DAT words) and the matching label augmentation."""

from typing import Optional

import numpy as np
import torch

from . import _hip
from ._layout import _F32, _stream


def events_to_frames(t_bin: torch.Tensor, x: torch.Tensor, y: torch.Tensor, p: torch.Tensor, T: int, H: int,
                     W: int) -> torch.Tensor:
    """Scatter events into binary frames ``[T, 2, H, W]`` (utils/datasets.py:378-435), on device."""
    for t in (t_bin, x, y, p):
        if not t.is_cuda or t.dtype != torch.int32:
            raise RuntimeError("events_to_frames: int32 HIP tensors required")
    buf = torch.empty((T, H, W, 2), device=t_bin.device, dtype=_F32)
    _hip.call("snn_events_to_frames", t_bin.data_ptr(), x.data_ptr(), y.data_ptr(), p.data_ptr(), t_bin.numel(),
              buf.data_ptr(), T, H, W, _stream())
    return buf.permute(0, 3, 1, 2)


AUG_Q16_ONE, AUG_Q16_MIN, AUG_Q16_MAX = 1 << 16, 1 << 14, 1 << 18   # zoom factors 1, 0.25 and 4 of an augmentation table


def check_aug_table(table: torch.Tensor, B: int) -> torch.Tensor:
    """A host augmentation table for ``B`` samples (``int32[B, 8]`` rows ``flip, a_q16, ox, oy, drop_bits, seed_bits, 0,
    0``, include/snn_hip.h) or ``ValueError``: the kernels take any contents without harm, the zoom range is kept here."""
    if not isinstance(table, torch.Tensor) or table.is_cuda or table.dtype != torch.int32:
        raise ValueError("aug_table: a host int32 tensor is required")
    if tuple(table.shape) != (B, 8):
        raise ValueError(f"aug_table: shape {tuple(table.shape)} is not [{B}, 8]")
    if B and not bool(((table[:, 0] == 0) | (table[:, 0] == 1)).all()):
        raise ValueError("aug_table: flip must be 0 or 1")
    if B and (int(table[:, 1].min()) < AUG_Q16_MIN or int(table[:, 1].max()) > AUG_Q16_MAX):
        raise ValueError(f"aug_table: a_q16 outside [{AUG_Q16_MIN}, {AUG_Q16_MAX}] (zoom 0.25 to 4)")
    return table.contiguous()


def _check_batch_vectors(events, offsets: torch.Tensor, t0: torch.Tensor, aug: Optional[torch.Tensor], B: int,
                         message: str) -> None:
    """The ``(tensor, dtype, numel)`` triples of ``events`` and the batch's ``offsets[B + 1]``, ``t0[B]``, ``aug[B, 8]`` (or
    None): every one a contiguous HIP tensor of its type and size, or ``ValueError(message)``."""
    want = tuple(events) + ((offsets, torch.int64, B + 1), (t0, torch.int64, B))
    if aug is not None:
        want += ((aug, torch.int32, 8 * B),)
    for v, dtype, n in want:
        if not v.is_cuda or v.dtype != dtype or v.numel() != n or not v.is_contiguous():
            raise ValueError(message)


class EventRepresentation:
    """What the scatter writes into a cell of ``X[T, B, 2, H, W]`` (``SNN_EVREP_*``, rules in ``include/snn_hip.h``):

    * ``"binary"``: 1 where any event fell (the reference's frames; the default everywhere);
    * ``"count"``: the number of events, ``min(n, clip) * scale``;
    * ``"time"``: a time surface per bin - the offset of the bin's latest event inside it, ``(r + 1) / step_us * scale``
      in ``(0, 1] * scale`` (no ``clip``);
    * ``"voxel"``: events spread over the two bins whose centres enclose them, bilinear in time with Q16 weights,
      ``min(sum, clip) * scale``.

    ``clip`` None or 0: no clip.  ``scale`` is finite and positive.  The accumulators are integers, so the frames are
    bit-identical from run to run and under any order of a sample's events.  A value object: it validates here, by name,
    and ``check(step_us)`` asks the library (``snn_events_rep_supported``) what the kernels take."""

    KINDS = tuple(_hip.EVENT_REPS)

    def __init__(self, kind: str = "binary", clip: Optional[int] = None, scale: float = 1.0):
        if kind not in _hip.EVENT_REPS:
            raise ValueError(f"EventRepresentation: kind must be one of {', '.join(self.KINDS)}, got {kind!r}")
        if clip is not None and (isinstance(clip, bool) or not isinstance(clip, (int, np.integer))):
            raise ValueError(f"EventRepresentation: clip must be an integer or None, got {clip!r}")
        clip = 0 if clip is None else int(clip)
        if clip < 0:
            raise ValueError(f"EventRepresentation: clip must not be negative, got {clip}")
        if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)):
            raise ValueError(f"EventRepresentation: scale must be a number, got {scale!r}")
        with np.errstate(over="ignore"):
            scale = float(np.float32(scale))   # the value the kernel multiplies by
        if not (np.isfinite(scale) and scale > 0.0):
            raise ValueError(f"EventRepresentation: scale must be finite and positive as fp32, got {scale}")
        if kind == "binary" and (clip != 0 or scale != 1.0):
            raise ValueError("EventRepresentation: binary frames take neither clip nor scale")
        if kind == "time" and clip != 0:
            raise ValueError("EventRepresentation: a time surface takes no clip")
        self.kind, self.rep, self.clip, self.scale = kind, _hip.EVENT_REPS[kind], clip, scale

    @classmethod
    def of(cls, value, who: str = "EventRepresentation") -> "EventRepresentation":
        """``value`` as an ``EventRepresentation``: one, a kind's name, or None (binary)."""
        if isinstance(value, cls):
            return value
        if value is None or isinstance(value, str):
            return cls("binary" if value is None else value)
        raise ValueError(f"{who}: representation must be a name ({', '.join(cls.KINDS)}) or an EventRepresentation, got "
                         f"{type(value).__name__}")

    @property
    def is_binary(self) -> bool:
        return self.rep == 0

    def check(self, step_us: int, who: str = "EventRepresentation") -> "EventRepresentation":
        """``ValueError`` unless the kernels take this representation at ``step_us`` (host-only query of the library)."""
        step_us = int(step_us)
        if step_us <= 0:
            raise ValueError(f"{who}: step_us must be positive, got {step_us}")
        if not -(1 << 63) <= step_us < (1 << 63) or self.clip >= (1 << 31) \
                or not _hip.query("snn_events_rep_supported", self.rep, step_us, self.clip):
            raise ValueError(f"{who}: the {self.kind} representation does not take clip {self.clip} at step_us {step_us} "
                             "(count: clip <= 2^24; time: step_us <= 2^32 - 1; voxel: clip <= 65535, step_us < 2^40)")
        return self

    def __eq__(self, other):
        return isinstance(other, EventRepresentation) and (self.kind, self.clip, self.scale) == (other.kind, other.clip,
                                                                                                 other.scale)

    def __hash__(self):
        return hash((self.kind, self.clip, self.scale))

    def __repr__(self):
        return f"EventRepresentation({self.kind!r}, clip={self.clip or None}, scale={self.scale})"


def _representation(representation, step_us: int, who: str):
    """``representation`` (None, a name or an ``EventRepresentation``) checked for ``step_us`` -> the object, or None for
    the binary frames (the entry points without ``_rep``)."""
    if representation is None:
        return None
    rep = EventRepresentation.of(representation, who).check(step_us, who)
    return None if rep.is_binary else rep


def _binary_rep():
    """The binary representation as an object: the tuple form without a table exists only as the ``_rep`` entry point."""
    return EventRepresentation("binary")


def _launch_batch_scatter(entry: str, events, n: int, offsets: torch.Tensor, t0: torch.Tensor,
                          aug: Optional[torch.Tensor], T: int, B: int, H: int, W: int, step_us: int,
                          rep=None) -> torch.Tensor:
    """Allocate ``[T][B][H][W][2]``, call the batch scatter ``entry`` (its ``_rep`` form for a representation ``rep``) on
    the ``events`` tensors and return the logical ``[T, B, 2, H, W]`` view."""
    buf = torch.empty((T, B, H, W, 2), device=events[0].device, dtype=_F32)
    rep_args = () if rep is None else (rep.rep, rep.clip, rep.scale)
    _hip.call(entry + ("_rep" if rep is not None else ""), *(v.data_ptr() for v in events), offsets.data_ptr(),
              t0.data_ptr(), aug.data_ptr() if aug is not None else None, int(n), buf.data_ptr(), T, B, H, W, int(step_us),
              *rep_args, _stream())
    return buf.permute(0, 1, 4, 2, 3)


def events_to_frames_aug(t_us: torch.Tensor, x: torch.Tensor, y: torch.Tensor, p: torch.Tensor, offsets: torch.Tensor,
                         t0: torch.Tensor, aug: Optional[torch.Tensor], T: int, H: int, W: int, step_us: int,
                         representation=None) -> torch.Tensor:
    """``snn_events_to_frames_aug`` on device tensors: the events of a whole batch (``t_us`` int64, ``x, y, p`` int32,
    sample ``b`` at ``offsets[b]:offsets[b+1]``, window starts ``t0[B]``) binned, transformed by the rows of ``aug``
    (a device copy of a table ``check_aug_table`` passed) and scattered -> ``[T, B, 2, H, W]``, channels-last memory.
    ``representation`` (a name or a ``data.EventRepresentation``; None: binary frames) takes
    ``snn_events_to_frames_aug_rep``; ``aug`` may then be None (the identity, no table is read)."""
    B = int(t0.numel())
    if int(step_us) <= 0:
        raise ValueError(f"events_to_frames_aug: step_us must be positive, got {step_us}")
    rep = _representation(representation, step_us, "events_to_frames_aug")
    if aug is None and representation is None:
        raise ValueError("events_to_frames_aug: aug may be None only when a representation is given")
    if aug is None and rep is None:
        rep = _binary_rep()
    n = t_us.numel()
    _check_batch_vectors(((t_us, torch.int64, n), (x, torch.int32, n), (y, torch.int32, n), (p, torch.int32, n)),
                         offsets, t0, aug, B,
                         "events_to_frames_aug: contiguous HIP tensors t_us int64[n], x / y / p int32[n], offsets "
                         "int64[B + 1], t0 int64[B], aug int32[B, 8] required")
    return _launch_batch_scatter("snn_events_to_frames_aug", (t_us, x, y, p), n, offsets, t0, aug, T, B, H, W, step_us,
                                 rep)


def events_to_frames_packed(words: torch.Tensor, offsets: torch.Tensor, t0: torch.Tensor, aug: Optional[torch.Tensor],
                            T: int, B: int, H: int, W: int, step_us: int, representation=None) -> torch.Tensor:
    """``snn_events_to_frames_packed`` on device tensors: the DAT records of a whole batch (``words`` uint32 or int32
    ``[n, 2]`` rows ``ts_us, data``, any storage offset that is a whole record; sample ``b`` at
    ``offsets[b]:offsets[b+1]``, window starts ``t0[B]``) unpacked, binned, transformed by the rows of ``aug`` (``None``: the
    identity, no table is read) and scattered -> ``[T, B, 2, H, W]``, channels-last memory.  ``representation`` (a name or
    a ``data.EventRepresentation``; None: binary frames) takes ``snn_events_to_frames_packed_rep``."""
    T, B, H, W = int(T), int(B), int(H), int(W)
    if int(step_us) <= 0:
        raise ValueError(f"events_to_frames_packed: step_us must be positive, got {step_us}")
    rep = _representation(representation, step_us, "events_to_frames_packed")
    if min(T, B, H, W) <= 0:
        raise ValueError(f"events_to_frames_packed: T, B, H, W must be positive, got {(T, B, H, W)}")
    word_types = tuple(d for d in (getattr(torch, "uint32", None), torch.int32) if d is not None)
    if (not words.is_cuda or words.dtype not in word_types or words.dim() != 2 or words.shape[1] != 2
            or not words.is_contiguous() or words.data_ptr() % 8):
        raise ValueError("events_to_frames_packed: words must be a contiguous 8-byte aligned HIP tensor uint32[n, 2]")
    _check_batch_vectors((), offsets, t0, aug, B,
                         "events_to_frames_packed: contiguous HIP tensors offsets int64[B + 1], t0 int64[B], aug "
                         "int32[B, 8] or None required")
    return _launch_batch_scatter("snn_events_to_frames_packed", (words,), words.shape[0], offsets, t0, aug, T, B, H, W,
                                 step_us, rep)


def labels_augment(labels: torch.Tensor, aug: torch.Tensor, W: int, H: int, min_visible: float = 0.25,
                   min_size_px: float = 2.0) -> torch.Tensor:
    """``snn_labels_augment``: the boxes of device ``labels[B, N, 5 | 6]`` under the rows of the device table ``aug`` -
    clipped to the frame, dropped (-1 rows) when too little stays visible or the box gets too small, the kept rows of a
    sample in front in their order.  Same shape out."""
    if not labels.is_cuda or labels.dtype != _F32 or labels.dim() != 3 or labels.shape[2] not in (5, 6):
        raise ValueError("labels_augment: fp32 HIP labels [B, N, 5 | 6] required")
    B, N, width = (int(v) for v in labels.shape)
    if not aug.is_cuda or aug.dtype != torch.int32 or aug.numel() != 8 * B or not aug.is_contiguous():
        raise ValueError("labels_augment: aug int32[B, 8] on the device required")
    labels = labels.contiguous()
    out = torch.empty_like(labels)
    if B and N:
        _hip.call("snn_labels_augment", labels.data_ptr(), out.data_ptr(), aug.data_ptr(), B, N, width, int(W), int(H),
                  float(min_visible), float(min_size_px), _stream())
    return out
