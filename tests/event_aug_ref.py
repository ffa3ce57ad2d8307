"""TEST INFRASTRUCTURE ONLY - numpy restatement of the augmented event feed (``snn_events_to_frames_aug`` and
``snn_labels_augment``, rules in ``include/snn_hip.h``): integer arithmetic for the events, float64 for the boxes.
Nothing here is product code and the product imports nothing from here."""
import numpy as np

M32 = 0xFFFFFFFF


def fmix32(u):
    """murmur3's 32-bit finaliser on uint64 arrays holding 32-bit values."""
    u = np.asarray(u, dtype=np.uint64) & np.uint64(M32)
    u ^= u >> np.uint64(16)
    u = (u * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    u ^= u >> np.uint64(13)
    u = (u * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    u ^= u >> np.uint64(16)
    return u


def drop_hash(j, seed):
    """The 32-bit value compared with the drop threshold, for index ``j`` (any int64 >= 0) inside a sample."""
    j = np.asarray(j, dtype=np.uint64)
    k = fmix32((np.uint64(int(seed) & M32) + np.uint64(0x9E3779B9) * (j >> np.uint64(32))) & np.uint64(M32))
    return fmix32((j & np.uint64(M32)) ^ k)


def identity_table(B):
    table = np.zeros((B, 8), dtype=np.int32)
    table[:, 1] = 65536
    return table


def frames_ref(samples, table, T, B, H, W, step_us):
    """``samples[b] = (t_us, x, y, p, t0)`` (integer arrays), ``table`` int32 ``[B, 8]`` -> uint8 ``[T, B, 2, H, W]`` with
    a 1 in every cell the kernel must set."""
    out = np.zeros((T, B, 2, H, W), dtype=np.uint8)
    assert len(samples) == B
    for b, (t, x, y, p, t0) in enumerate(samples):
        t, x, y, p = (np.asarray(v).astype(np.int64) for v in (t, x, y, p))
        j = np.arange(t.size, dtype=np.int64)
        flip, a, ox, oy = (int(v) for v in table[b, :4])
        drop, seed = int(table[b, 4]) & M32, int(table[b, 5]) & M32
        t_bin = np.floor_divide(t - int(t0), int(step_us))            # numpy floors towards minus infinity
        ok = (t_bin >= 0) & (t_bin < T) & (y >= 0) & (y < H) & ((p == 0) | (p == 1))
        x = np.clip(x, 0, W - 1)
        ok &= ~(drop_hash(j, seed) < np.uint64(drop))
        if flip:
            x = W - 1 - x
        xo = (((2 * x + 1) * a) >> 17) + ox
        yo = (((2 * y + 1) * a) >> 17) + oy
        ok &= (xo >= 0) & (xo < W) & (yo >= 0) & (yo < H)
        out[t_bin[ok], b, p[ok], yo[ok], xo[ok]] = 1
    return out


def label_decisions(labels, table, W, H, min_visible, min_size_px):
    """float64 working of ``labels_ref`` per row: ``(valid, keep, new_boxes[B, N, 4], margins[B, N, 3])`` - the margins
    are the three compared quantities ``A1 - min_visible A0``, ``w W - min_size_px``, ``h H - min_size_px``."""
    lab = np.asarray(labels, dtype=np.float64)
    B, N, width = lab.shape
    c0 = width - 5
    valid = lab[:, :, c0] >= 0
    flip = table[:, 0].astype(bool)[:, None]
    s = (table[:, 1].astype(np.float64) / 65536.0)[:, None]
    dx = (table[:, 2].astype(np.float64) / W)[:, None]
    dy = (table[:, 3].astype(np.float64) / H)[:, None]
    x1, y1, x2, y2 = (lab[:, :, c0 + k] for k in (1, 2, 3, 4))
    x1, x2 = np.where(flip, 1.0 - x2, x1), np.where(flip, 1.0 - x1, x2)
    x1, x2, y1, y2 = x1 * s + dx, x2 * s + dx, y1 * s + dy, y2 * s + dy
    a0 = (x2 - x1) * (y2 - y1)
    x1, x2, y1, y2 = (np.clip(v, 0.0, 1.0) for v in (x1, x2, y1, y2))
    w, h = x2 - x1, y2 - y1
    margins = np.stack([w * h - min_visible * a0, w * W - min_size_px, h * H - min_size_px], axis=-1)
    keep = valid & (margins >= 0).all(axis=-1)
    return valid, keep, np.stack([x1, y1, x2, y2], axis=-1), margins


def labels_ref(labels, table, W, H, min_visible, min_size_px):
    """float64 ``[B, N, width]``: transformed, clipped, filtered and compacted rows, -1 rows behind."""
    lab = np.asarray(labels, dtype=np.float64)
    B, N, width = lab.shape
    _, keep, boxes, _ = label_decisions(labels, table, W, H, min_visible, min_size_px)
    out = np.full((B, N, width), -1.0)
    for b in range(B):
        rows = np.flatnonzero(keep[b])
        out[b, :rows.size, :width - 4] = lab[b, rows, :width - 4]
        out[b, :rows.size, width - 4:] = boxes[b, rows]
    return out
