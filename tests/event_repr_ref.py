"""TEST INFRASTRUCTURE ONLY - numpy integer restatement of the event representations (``snn_events_to_frames_aug_rep`` /
``snn_events_to_frames_packed_rep``, rules in ``include/snn_hip.h``) on the event selection of ``tests/event_aug_ref.py``:
uint64 accumulators reduced mod 2^32, then ``np.float32`` operations in the stated order.  Nothing here is product code
and the product imports nothing from here."""
import numpy as np

from tests.event_aug_ref import M32, drop_hash

BINARY, COUNT, TIME, VOXEL = 0, 1, 2, 3
NAMES = {"binary": BINARY, "count": COUNT, "time": TIME, "voxel": VOXEL}


def select_events(sample, row, T, H, W, step_us):
    """Rules 1-6 of ``snn_events_to_frames_aug`` on one sample ``(t_us, x, y, p, t0)`` under the table row ``row``
    (int32[8]) -> ``(d, p, yo, xo)`` of the events that are written, ``d = t_us - t0`` in ``[0, T step_us)``, in the
    sample's order."""
    t, x, y, p = (np.asarray(v).astype(np.int64) for v in sample[:4])
    j = np.arange(t.size, dtype=np.int64)
    flip, a, ox, oy = (int(v) for v in row[:4])
    drop, seed = int(row[4]) & M32, int(row[5]) & M32
    d = t - int(sample[4])
    ok = (d >= 0) & (d < T * int(step_us)) & (y >= 0) & (y < H) & ((p == 0) | (p == 1))
    x = np.clip(x, 0, W - 1)
    ok &= ~(drop_hash(j, seed) < np.uint64(drop))
    if flip:
        x = W - 1 - x
    xo = (((2 * x + 1) * a) >> 17) + ox
    yo = (((2 * y + 1) * a) >> 17) + oy
    ok &= (xo >= 0) & (xo < W) & (yo >= 0) & (yo < H)
    return d[ok], p[ok], yo[ok], xo[ok]


def voxel_weights(d, T, step_us):
    """``(k, 65536 - q, q)`` per event: the lower bin (-1 .. T-1) and the Q16 weights of bins ``k`` and ``k + 1``."""
    d = np.asarray(d, dtype=np.int64)
    step = int(step_us)
    u = 2 * d - step
    k = np.floor_divide(u, 2 * step)
    rem = u - k * 2 * step
    q = np.floor_divide(rem * 65536, 2 * step)
    return k, 65536 - q, q


def accumulators_ref(samples, table, T, B, H, W, step_us, rep):
    """uint64 ``[T, B, 2, H, W]``: the per-cell accumulators reduced mod 2^32 (binary: 0 / 1)."""
    acc = np.zeros((T, B, 2, H, W), dtype=np.uint64)
    step = int(step_us)
    assert len(samples) == B
    for b, sample in enumerate(samples):
        d, p, yo, xo = select_events(sample, table[b], T, H, W, step)
        t = np.floor_divide(d, step)
        bb = np.full_like(t, b)
        if rep == BINARY:
            acc[t, bb, p, yo, xo] = 1
        elif rep == COUNT:
            np.add.at(acc, (t, bb, p, yo, xo), np.uint64(1))
        elif rep == TIME:
            np.maximum.at(acc, (t, bb, p, yo, xo), (d - t * step + 1).astype(np.uint64))
        elif rep == VOXEL:
            k, w0, w1 = voxel_weights(d, T, step)
            lo = k >= 0
            np.add.at(acc, (k[lo], bb[lo], p[lo], yo[lo], xo[lo]), w0[lo].astype(np.uint64))
            hi = (k + 1 <= T - 1) & (w1 > 0)
            np.add.at(acc, (k[hi] + 1, bb[hi], p[hi], yo[hi], xo[hi]), w1[hi].astype(np.uint64))
        else:
            raise ValueError(rep)
    return acc & np.uint64(M32)


def finalize_ref(acc, step_us, rep, clip, scale):
    """The finalize pass on uint64 accumulators (< 2^32): one ``np.float32`` rounding per operation."""
    acc = np.asarray(acc, dtype=np.uint64)
    scale = np.float32(scale)
    if rep == BINARY:
        return acc.astype(np.float32)
    if rep == COUNT:
        a = np.minimum(acc, np.uint64(clip)) if clip else acc
        return a.astype(np.float32) * scale
    if rep == TIME:
        return (acc.astype(np.float32) / np.float32(int(step_us))) * scale
    a = np.minimum(acc, np.uint64(clip * 65536)) if clip else acc
    return (a.astype(np.float32) * np.float32(2.0 ** -16)) * scale


def frames_rep_ref(samples, table, T, B, H, W, step_us, rep, clip=0, scale=1.0):
    """``samples[b] = (t_us, x, y, p, t0)``, ``table`` int32 ``[B, 8]`` -> float32 ``[T, B, 2, H, W]``."""
    out = finalize_ref(accumulators_ref(samples, table, T, B, H, W, step_us, rep), step_us, rep, clip, scale)
    assert out.dtype == np.float32
    return out
