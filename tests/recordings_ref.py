"""TEST INFRASTRUCTURE ONLY - seeded synthetic recordings for the tests of ``snn_for_object_detection_amd.recordings``:
event streams with a dense background and a sparse stretch, and label rows chosen so that a single-target walk meets an
accepted sample, a sparse window, a label step whose boxes are all under the area threshold, and the end of the labels.
Nothing here is product code and the product imports nothing from here."""
import numpy as np

GEN1_BOX_DTYPE = [("ts", "<u8"), ("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("class_id", "u1"),
                  ("confidence", "<f4"), ("track_id", "<u4")]


def stream(rng, width, height, duration_us, per_ms, sparse=(), sparse_per_ms=2):
    """Sorted events ``(t int64, x, y, p int32)``: ``per_ms`` events in every millisecond, ``sparse_per_ms`` in the
    milliseconds of the ``sparse`` ranges ``(lo_ms, hi_ms)``."""
    ts = []
    for ms in range(duration_us // 1000):
        n = sparse_per_ms if any(lo <= ms < hi for lo, hi in sparse) else per_ms
        ts.append(np.sort(rng.integers(ms * 1000, (ms + 1) * 1000, n)))
    t = np.concatenate(ts).astype(np.int64)
    n = t.size
    return (t, rng.integers(0, width, n).astype(np.int32), rng.integers(0, height, n).astype(np.int32),
            rng.integers(0, 2, n).astype(np.int32))


def walk_boxes(step_us, width, height, steps=(10, 20, 30, 40, 50), small=(40,)):
    """A structured gen1 box array with two boxes at each of ``steps`` (timestamps inside the step, not on its boundary);
    the boxes of the ``small`` steps are under 1 % of the frame, the others well above, and every other label step also
    carries a small box that the area threshold removes from the sample."""
    rows = []
    for k, s in enumerate(steps):
        ts = s * step_us + 37 * (k + 1)
        if s in small:
            rows += [(ts, 0.10 * width, 0.10 * height, 0.05 * width, 0.05 * height, 0),
                     (ts, 0.50 * width, 0.40 * height, 0.09 * width, 0.09 * height, 1)]
        else:
            rows += [(ts, 0.10 * width + k, 0.20 * height, 0.40 * width, 0.50 * height, k % 2),
                     (ts, 0.30 * width, 0.25 * height + k, 0.45 * width, 0.35 * height, (k + 1) % 2)]
            if k % 2:
                rows.append((ts, 0.70 * width, 0.70 * height, 0.04 * width, 0.04 * height, 0))
    b = np.zeros(len(rows), dtype=GEN1_BOX_DTYPE)
    for i, (ts, x, y, w, h, c) in enumerate(rows):
        b[i]["ts"], b[i]["x"], b[i]["y"], b[i]["w"], b[i]["h"], b[i]["class_id"] = ts, x, y, w, h, c
    b["confidence"] = 1.0
    return b
