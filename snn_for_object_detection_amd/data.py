"""The step FEEDING the path: raw events -> a device batch ``X[T, B, 2, H, W]``.

The reference voxelises on the CPU inside DataLoader workers (``utils/datasets.py:403-435``) and ships dense fp32
frames to the GPU: 93 MB per B=5, T=32 GEN1 batch, 1.9 GB for the 1Mpx batch.  Here the host hands over the raw
events (16 bytes each: 5 % occupancy = 19 MB for the GEN1 batch), the copy runs on a side stream out of pinned
memory, and a HIP scatter kernel (``snn_events_to_frames``) writes the binary frames directly in the channels-last
layout the first convolution reads, so the NCHW -> NHWC pass over the input disappears as well.

``EventBatcher`` mirrors the reference's sample / collate contract:
* per sample: events ``(t_us, x, y, p)`` with ``t >= t0`` are binned ``(t - t0) // time_step_us`` into ``num_steps``
  frames, ``x`` clipped to the frame, value 1 not a count (``datasets.py:415-433``);
* the batch stacks samples on dim 1 and pads label rows with -1 (``_stack_data``, ``datasets.py:127-135``).

``EventAugment`` (not in the reference) adds the usual event-camera augmentations - horizontal flip, zoom with a shift,
random event drop - inside the scatter: a batcher that has one hands the raw int64 timestamps to
``snn_events_to_frames_aug``, which bins and transforms them in one launch, and the boxes to ``snn_labels_augment``.

A sample may also be ``(words, t0_us)`` - the 8-byte records of a Prophesee DAT recording as they lie in the file
(``recordings.DatRecording``): the slices go through one of two persistent pinned staging buffers, one copy carries
8 bytes per event, and ``snn_events_to_frames_packed`` unpacks the words inside the scatter.

``EventRepresentation`` (not in the reference) chooses what a cell holds: the binary flag (the default), an event count,
a per-bin time surface or a temporally interpolated voxel grid - integer atomics inside the same scatter and one
finalize pass (``snn_events_to_frames_aug_rep`` / ``snn_events_to_frames_packed_rep``).
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from .event_ops import EventRepresentation  # noqa: F401  (defined beside the scatters that take it)


def collate_labels(labels: Sequence[torch.Tensor], B: int) -> torch.Tensor:
    """``_stack_data`` for the label lists (``datasets.py:127-135``): per-sample rows ``[n, 5]`` (``class, x1, y1, x2,
    y2``) or ``[n, 6]`` (``ts, class, x1, y1, x2, y2``, the multi-target samples) -> host ``[B, n_max, 5 | 6]`` padded
    with -1.  The width is that of the rows given; a sample without rows (any shape with no row in it) fits either,
    and a batch without any row is five columns wide.  Mixed widths raise."""
    n_max = max((int(l.shape[0]) for l in labels), default=0)
    widths = {int(l.shape[1]) for l in labels if l.dim() == 2 and l.shape[0] > 0}
    if len(widths) > 1 or not widths <= {5, 6}:
        raise ValueError(f"EventBatcher: label rows must all have 5 or all have 6 columns, got {sorted(widths)}")
    lab = torch.full((B, n_max, widths.pop() if widths else 5), -1.0, dtype=torch.float32)
    for b, l in enumerate(labels):
        if l.shape[0] > 0:
            lab[b, : l.shape[0]] = l
    return lab


class EventAugment:
    """Per-sample horizontal flip, zoom with shift and random event drop, applied to the events inside the scatter
    kernel (``snn_events_to_frames_aug``) and to the boxes by ``snn_labels_augment`` - the same map for both.

    * ``hflip``: probability of a flip.
    * ``zoom=(lo, hi)``, ``0.25 <= lo <= hi <= 4``: ``a_q16 = round(u * 65536)`` for ``u`` uniform in ``[lo, hi]``; the
      factor applied is ``s = a_q16 / 65536``.  The shift ``ox`` is a uniform integer between ``min(0, W - ceil(s W))``
      and ``max(0, W - ceil(s W))`` (``oy`` likewise with ``H``): a zoomed-out image lands wholly inside the frame, a
      zoomed-in image is a random crop window.  Events are not interpolated: a factor above 1 leaves the gaps that
      sparse events leave.
    * ``drop``: a probability or a range ``(lo, hi)`` of it, ``0 <= lo <= hi < 1``; each sample draws its own probability
      and its own 32-bit seed, and an event is dropped by a hash of the seed and its index inside the sample.
    * ``min_visible``, ``min_size_px``: a box is kept when at least that share of its area stays inside the frame and
      its clipped extents are at least that many pixels wide and high.

    ``draw(B)`` returns the host table ``int32[B, 8]`` (rows ``flip, a_q16, ox, oy, drop_bits, seed_bits, 0, 0``) from the
    object's own ``torch.Generator``: the sequence of tables is a function of ``seed`` alone and the global RNG is never
    touched.  Under data parallelism give every rank a different ``seed`` (``seed + rank``), or all ranks draw the same
    transforms."""

    def __init__(self, hflip: float = 0.0, zoom: Optional[Tuple[float, float]] = None, drop=0.0,
                 min_visible: float = 0.25, min_size_px: float = 2.0, seed: int = 0):
        if not 0.0 <= float(hflip) <= 1.0:
            raise ValueError(f"EventAugment: hflip must be a probability, got {hflip}")
        if zoom is not None:
            if len(zoom) != 2 or not 0.25 <= float(zoom[0]) <= float(zoom[1]) <= 4.0:
                raise ValueError(f"EventAugment: zoom must be (lo, hi) with 0.25 <= lo <= hi <= 4, got {zoom}")
            zoom = (float(zoom[0]), float(zoom[1]))
        drop = tuple(float(v) for v in drop) if isinstance(drop, (tuple, list)) else (float(drop), float(drop))
        if len(drop) != 2 or not 0.0 <= drop[0] <= drop[1] < 1.0:
            raise ValueError(f"EventAugment: drop must be a probability or (lo, hi) with 0 <= lo <= hi < 1, got {drop}")
        if not 0.0 <= float(min_visible) <= 1.0:
            raise ValueError(f"EventAugment: min_visible must lie in [0, 1], got {min_visible}")
        if not float(min_size_px) >= 0.0:
            raise ValueError(f"EventAugment: min_size_px must not be negative, got {min_size_px}")
        self.hflip, self.zoom, self.drop = float(hflip), zoom, drop
        self.min_visible, self.min_size_px, self.seed = float(min_visible), float(min_size_px), int(seed)
        self.W = self.H = None          # bound by the batcher that adopts the object (or passed to draw)
        self._gen = torch.Generator(device="cpu")
        self._gen.manual_seed(self.seed)

    @staticmethod
    def identity(B: int) -> torch.Tensor:
        """The table that changes nothing (validation batches)."""
        table = torch.zeros((B, 8), dtype=torch.int32)
        table[:, 1] = 1 << 16
        return table

    def draw(self, B: int, W: Optional[int] = None, H: Optional[int] = None) -> torch.Tensor:
        W = self.W if W is None else W
        H = self.H if H is None else H
        if W is None or H is None:
            raise ValueError("EventAugment.draw: W and H are needed (pass them, or hand the object to an EventBatcher)")
        u = torch.rand((B, 5), generator=self._gen, dtype=torch.float64)   # the same draws whatever is switched on
        seeds = torch.randint(0, 1 << 32, (B,), generator=self._gen, dtype=torch.int64)
        table = torch.zeros((B, 8), dtype=torch.int64)
        table[:, 0] = u[:, 0] < self.hflip
        table[:, 1] = 1 << 16
        if self.zoom is not None:
            lo, hi = self.zoom
            a = torch.round((lo + (hi - lo) * u[:, 1]) * 65536.0).to(torch.int64)
            a = a.clamp(int(round(lo * 65536.0)), int(round(hi * 65536.0)))
            table[:, 1] = a
            for col, size, k in ((2, int(W), 2), (3, int(H), 3)):
                room = size - (a * size + 65535) // 65536               # size - ceil(s size)
                first, span = room.clamp(max=0), room.abs() + 1
                table[:, col] = first + torch.minimum((u[:, k] * span).floor().to(torch.int64), span - 1)
        if self.drop[1] > 0.0:
            prob = self.drop[0] + (self.drop[1] - self.drop[0]) * u[:, 4]
            table[:, 4] = (prob * 4294967296.0).floor().to(torch.int64).clamp(0, (1 << 32) - 1)
        table[:, 5] = seeds
        bits = table[:, 4:6]                                             # uint32 values -> the int32 with the same bits
        table[:, 4:6] = torch.where(bits >= (1 << 31), bits - (1 << 32), bits)
        return table.to(torch.int32)


class EventBatcher:
    def __init__(self, num_steps: int, height: int, width: int, time_step_us: int, device="cuda",
                 augment: Optional[EventAugment] = None, representation="binary"):
        self.T, self.H, self.W, self.step = int(num_steps), int(height), int(width), int(time_step_us)
        self.representation = EventRepresentation.of(representation, "EventBatcher")
        if not self.representation.is_binary:
            self.representation.check(self.step, "EventBatcher")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("EventBatcher: a HIP device is required (no CPU fallback)")
        if augment is not None and not isinstance(augment, EventAugment):
            raise ValueError("EventBatcher: augment must be an EventAugment")
        self.augment = augment
        self.last_aug_table = None      # host int32[B, 8]: the table of the last augmented call
        if augment is not None:
            if augment.W is None:
                augment.W, augment.H = self.W, self.H
            elif (augment.W, augment.H) != (self.W, self.H):
                raise ValueError(f"EventBatcher: the EventAugment is bound to frames of {augment.W} x {augment.H}")
        # a stream that really runs beside the main stream (HIP streams share a few hardware queues: functional.concurrent_stream)
        from . import functional as _HF
        dev = self.device if self.device.index is not None else torch.device("cuda", torch.cuda.current_device())
        self._copy_stream = _HF.concurrent_stream(torch.cuda.current_stream(dev), avoid=tuple(_HF._SIDE_STREAMS.values()))
        # packed samples: two pinned staging slots used in turn, each with the HIP event recorded behind its last copies
        self._slots = [{"words": None, "words_np": None, "meta": None, "done": None} for _ in range(2)]
        self._slot = 1

    def __call__(self, samples: Sequence[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, int]],
                 labels: Optional[Sequence[torch.Tensor]] = None, *, augment: bool = True,
                 aug_table: Optional[torch.Tensor] = None):
        """``samples[b] = (t_us, x, y, p, t0_us)`` - 1-D host tensors (int64 / int32; pinned memory makes the copy
        asynchronous) and the time of the first frame.  Returns ``X[T, B, 2, H, W]`` (logical NCHW view of a
        channels-last buffer) and, when ``labels`` is given, ``labels[B, N, 5]`` padded with -1 - ``[B, N, 6]`` when the
        rows given carry a timestep in front (``(ts, class, x1, y1, x2, y2)``, the multi-target sample format).
        Or ``samples[b] = (words, t0_us)`` with ``words`` the DAT records of the sample, host ``uint32[n, 2]`` (``_packed``);
        all samples of a call have the same form.

        A batcher built with an ``EventAugment`` draws one transform per sample and applies it to events and boxes
        (``augment=False``: the identity, for validation batches); ``aug_table`` (host ``int32[B, 8]``) replaces the
        draw, with or without an ``EventAugment`` - for a test, or for the same transform on two modalities.  The table
        used is kept as ``last_aug_table``.  Boxes the transform pushes out of the frame become -1 rows behind the kept
        ones; ``N`` stays that of the collate."""
        forms = {len(s) for s in samples}
        if 2 in forms and forms != {2}:
            raise ValueError("EventBatcher: packed (words, t0_us) samples and (t_us, x, y, p, t0_us) samples mixed in one "
                             "call")
        packed = forms == {2}
        if aug_table is None and self.augment is None:
            if packed or not self.representation.is_binary:   # (no table: the kernel reads none)
                return self._packed(samples, labels, None) if packed else self._augmented(samples, labels, None)
            return self._plain(samples, labels)
        from . import functional as _HF
        B = len(samples)
        if aug_table is not None:
            table = _HF.check_aug_table(aug_table, B)
        else:
            table = self.augment.draw(B) if augment else EventAugment.identity(B)
        return self._packed(samples, labels, table) if packed else self._augmented(samples, labels, table)

    def _staging(self, n: int, meta_len: int) -> dict:
        """The next of the two pinned staging slots, free to be written: its last H2D copies have completed (the HIP event
        recorded behind them is waited on here, on the host), and it holds at least ``n`` records and ``meta_len`` int64."""
        self._slot ^= 1
        slot = self._slots[self._slot]
        if slot["done"] is not None:
            slot["done"].synchronize()
        if slot["words"] is None or slot["words"].shape[0] < n:
            cap = max(n, 2 * (0 if slot["words"] is None else int(slot["words"].shape[0])), 1 << 16)
            slot["words"] = torch.empty((cap, 2), dtype=torch.int32, pin_memory=True)
            slot["words_np"] = slot["words"].numpy().view(np.uint32)
        if slot["meta"] is None or slot["meta"].numel() < meta_len:
            slot["meta"] = torch.empty(meta_len, dtype=torch.int64, pin_memory=True)
        return slot

    def _packed(self, samples, labels, table: Optional[torch.Tensor]):
        """Packed samples ``(words, t0_us)`` - ``words`` the 8-byte records of a DAT recording as host ``uint32[n, 2]``
        (numpy, a memory map included, or torch): the slices are copied into a persistent pinned staging buffer, one H2D
        copy carries the events (8 bytes each) and one ``offsets | t0 | table``, one ``snn_events_to_frames_packed`` launch
        unpacks, bins and transforms.  ``table`` None: the kernel reads no table."""
        B = len(samples)
        if self.step <= 0:
            raise ValueError(f"EventBatcher: time_step_us must be positive, got {self.step}")
        words = []
        for w, _ in samples:
            w = w.numpy() if isinstance(w, torch.Tensor) else np.asarray(w)
            if w.dtype.kind not in "ui" or w.dtype.itemsize != 4 or w.ndim != 2 or w.shape[1] != 2:
                raise ValueError(f"EventBatcher: packed events must be uint32 [n, 2], got {w.dtype} {tuple(w.shape)}")
            words.append(w.view(np.uint32) if w.dtype != np.uint32 else w)
        counts = [int(w.shape[0]) for w in words]
        n = sum(counts)
        meta_len = (2 * B + 1) + (4 * B if table is not None else 0)   # offsets[B + 1] | t0[B] | table[B][8] (int32)
        slot = self._staging(n, meta_len)
        at = 0
        for w, c in zip(words, counts):
            if c:
                slot["words_np"][at:at + c] = w
                at += c
        if slot["done"] is None:
            slot["done"] = torch.cuda.Event()   # recorded behind this call's copies: the slot is rewritten only after it

        def copy_events():
            ev = torch.empty((max(n, 1), 2), device=self.device, dtype=torch.int32)
            if n:
                ev[:n].copy_(slot["words"][:n], non_blocking=True)
            return [ev]

        return self._scatter_batch("snn_events_to_frames_packed", counts, [int(s[1]) for s in samples], table, labels,
                                   slot["meta"][:meta_len], copy_events, done=slot["done"])

    def _augmented(self, samples, labels, table: Optional[torch.Tensor]):
        """Four copies per sample into slices of the batch's event arrays, ``offsets | t0 | table`` in one small pinned
        tensor, one ``snn_events_to_frames_aug`` launch that bins and transforms, one ``snn_labels_augment`` launch.
        ``table`` None (a representation other than binary on un-augmented samples): the kernel reads no table."""
        B = len(samples)
        if self.step <= 0:
            raise ValueError(f"EventBatcher: time_step_us must be positive, got {self.step}")
        counts = [int(s[0].numel()) for s in samples]
        n = sum(counts)
        # offsets[B + 1] | t0[B] | table[B][8] (int32)
        meta = torch.empty((6 if table is not None else 2) * B + 1, dtype=torch.int64, pin_memory=True)

        def copy_events():
            ev = [torch.empty(max(n, 1), device=self.device, dtype=d)
                  for d in (torch.int64, torch.int32, torch.int32, torch.int32)]
            at = 0
            for sample, c in zip(samples, counts):
                if c:
                    for dst, src in zip(ev, sample[:4]):
                        dst[at:at + c].copy_(src, non_blocking=True)
                    at += c
            return ev

        return self._scatter_batch("snn_events_to_frames_aug", counts, [int(s[4]) for s in samples], table, labels, meta,
                                   copy_events)

    def _scatter_batch(self, entry: str, counts, t0s, table: Optional[torch.Tensor], labels, meta: torch.Tensor,
                       copy_events, done=None):
        """What ``_packed`` and ``_augmented`` share behind their staging: ``offsets | t0 | table`` into the pinned int64
        ``meta``; on the copy stream the caller's ``copy_events()`` (its H2D copies -> the device event tensors of
        ``entry``), the copy of ``meta`` (``done``, a HIP event, is recorded behind both) and the launch; the hand-over of
        the streams, ``last_aug_table``, and the labels - augmented by the same table - on the main stream.  A
        representation other than binary takes ``entry``'s ``_rep`` form with its three arguments."""
        from . import functional as _HF
        B, n = len(counts), sum(counts)
        T, H, W = self.T, self.H, self.W
        rep = self.representation
        if not rep.is_binary:
            entry += "_rep"
        rep_args = () if rep.is_binary else (rep.rep, rep.clip, rep.scale)
        meta[0] = 0
        meta[1:B + 1] = torch.tensor(counts, dtype=torch.int64).cumsum(0)
        meta[B + 1:2 * B + 1] = torch.tensor(t0s, dtype=torch.int64)
        if table is not None:
            meta[2 * B + 1:].view(torch.int32).copy_(table.reshape(-1))
        main = torch.cuda.current_stream(self.device)
        buf = torch.empty((T, B, H, W, 2), device=self.device, dtype=torch.float32)   # [T][B][H][W][C]
        meta_dev = torch.empty(meta.numel(), device=self.device, dtype=torch.int64)
        self._copy_stream.wait_stream(main)
        with torch.cuda.stream(self._copy_stream):
            ev = copy_events()
            meta_dev.copy_(meta, non_blocking=True)
            if done is not None:
                done.record(self._copy_stream)
            aug_dev = meta_dev[2 * B + 1:].view(torch.int32) if table is not None else None
            _hip.call(entry, *(v.data_ptr() for v in ev), meta_dev.data_ptr(), meta_dev[B + 1:].data_ptr(),
                      aug_dev.data_ptr() if aug_dev is not None else None, n, buf.data_ptr(), T, B, H, W, self.step,
                      *rep_args, self._copy_stream.cuda_stream)
            buf.record_stream(self._copy_stream)
            meta_dev.record_stream(self._copy_stream)
        main.wait_stream(self._copy_stream)
        if table is not None:
            self.last_aug_table = table.clone()
        X = buf.permute(0, 1, 4, 2, 3)
        if labels is None:
            return X
        with torch.cuda.stream(main):
            lab = collate_labels(labels, B).to(self.device, non_blocking=True)
            if table is not None:
                a = self.augment
                lab = _HF.labels_augment(lab, aug_dev, W, H, *((a.min_visible, a.min_size_px) if a is not None else ()))
        return X, lab

    def _plain(self, samples, labels=None):
        B = len(samples)
        T, H, W = self.T, self.H, self.W
        main = torch.cuda.current_stream(self.device)
        buf = torch.empty((T, B, H, W, 2), device=self.device, dtype=torch.float32)   # [T][B][H][W][C]
        self._copy_stream.wait_stream(main)  # the allocation (and earlier users of its memory) precede the scatter
        with torch.cuda.stream(self._copy_stream):
            slots, xs, ys, ps = [], [], [], []
            for b, (t_us, x, y, p, t0) in enumerate(samples):
                if int(t_us.numel()) == 0:
                    continue
                dev = [v.to(self.device, non_blocking=True) for v in (t_us, x, y, p)]
                t_bin = (dev[0].to(torch.int64) - int(t0)).div(self.step, rounding_mode="floor")
                # frame index inside the batch buffer = t * B + b; events before t0 or past the window are dropped
                ok = (t_bin >= 0) & (t_bin < T)
                slots.append(torch.where(ok, t_bin * B + b, torch.full_like(t_bin, -1)).to(torch.int32))
                xs.append(dev[1].to(torch.int32))
                ys.append(dev[2].to(torch.int32))
                ps.append(dev[3].to(torch.int32))
            if slots:
                ev = [torch.cat(v) for v in (slots, xs, ys, ps)]
                n = int(ev[0].numel())
            else:
                ev, n = [torch.zeros(1, device=self.device, dtype=torch.int32)] * 4, 0
            # one launch for the whole batch: zero-fills the buffer, then scatters every sample's events
            _hip.call("snn_events_to_frames", ev[0].data_ptr(), ev[1].data_ptr(), ev[2].data_ptr(), ev[3].data_ptr(), n,
                      buf.data_ptr(), T * B, H, W, self._copy_stream.cuda_stream)
            buf.record_stream(self._copy_stream)
        main.wait_stream(self._copy_stream)
        X = buf.permute(0, 1, 4, 2, 3)  # [T, B, 2, H, W], channels-last memory
        if labels is None:
            return X
        return X, collate_labels(labels, B).to(self.device, non_blocking=True)
