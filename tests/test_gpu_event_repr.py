"""Event representations on the GPU: ``snn_events_to_frames_aug_rep`` / ``snn_events_to_frames_packed_rep`` bit for bit
(frames compared as uint32) against the integer reference of ``tests/event_repr_ref.py``, and through ``EventBatcher``,
``PropheseeFeed`` and one training step."""
import numpy as np
import pytest
import torch

from tests import event_aug_ref as R
from tests import event_repr_ref as E
from tests import recordings_ref as S

pytestmark = pytest.mark.gpu

T, B, H, W = 4, 3, 6, 10
STEPS = (1000, 16667)
REPS = {"binary": (0, 1.0), "count": (0, 1.0), "count_clip": (2, 0.25), "time": (0, 1.0), "time_scaled": (0, 3.0),
        "voxel": (0, 1.0), "voxel_clip": (1, 1.0 / 3.0)}


@pytest.fixture(scope="module")
def pkg(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import snn_for_object_detection_amd as p
    return p


def _kind(name):
    return name.split("_")[0]


def _table(n, flip=0, a=65536, ox=0, oy=0, drop=0, seeds=None):
    t = R.identity_table(n)
    t[:, 0], t[:, 1], t[:, 2], t[:, 3] = flip, a, ox, oy
    t[:, 4] = np.array([drop], dtype=np.uint32).view(np.int32)[0]
    if seeds is not None:
        t[:, 5] = np.array(seeds, dtype=np.uint32).view(np.int32)
    return t


def _bits(X):
    """Device frames ``[T, B, 2, H, W]`` (any strides) -> host uint32 of the same logical shape."""
    return X.contiguous().cpu().numpy().view(np.uint32)


def _batch_vectors(samples):
    offsets = torch.tensor(np.cumsum([0] + [len(s[0]) for s in samples]), dtype=torch.int64).cuda()
    t0 = torch.tensor([int(s[-1]) for s in samples], dtype=torch.int64).cuda()
    return offsets, t0


def _tuple_frames(pkg, samples, table, T_, H_, W_, step, kind, clip=0, scale=1.0):
    """The tuple entry through ``functional.events_to_frames_aug`` -> uint32 ``[T, B, 2, H, W]``."""
    from snn_for_object_detection_amd import functional as HF
    cat = [np.concatenate([np.asarray(s[k]) for s in samples]) for k in range(4)]
    dev = [torch.from_numpy(cat[0].astype(np.int64)).cuda()] + [torch.from_numpy(v.astype(np.int32)).cuda() for v in cat[1:]]
    offsets, t0 = _batch_vectors(samples)
    aug = None if table is None else torch.from_numpy(table).cuda()
    X = HF.events_to_frames_aug(*dev, offsets, t0, aug, T_, H_, W_, step,
                                representation=pkg.EventRepresentation(kind, clip=clip, scale=scale))
    assert X.shape == (T_, len(samples), 2, H_, W_) and HF.is_channels_last(X)
    return _bits(X)


def _packed_frames(pkg, samples, table, T_, H_, W_, step, kind, clip=0, scale=1.0):
    """The same samples as DAT records through ``functional.events_to_frames_packed``."""
    from snn_for_object_detection_amd import functional as HF
    words = np.concatenate([pkg.pack_events(*(np.asarray(v) for v in s[:4])).reshape(-1, 2) for s in samples])
    offsets, t0 = _batch_vectors(samples)
    aug = None if table is None else torch.from_numpy(table).cuda()
    X = HF.events_to_frames_packed(torch.from_numpy(words.view(np.int32)).cuda(), offsets, t0, aug, T_, len(samples), H_, W_,
                                   step, representation=pkg.EventRepresentation(kind, clip=clip, scale=scale))
    return _bits(X)


def _packable(samples):
    """The events of ``samples`` that a DAT record can hold: no negative field or time, a polarity of one bit."""
    out = []
    for s in samples:
        t, x, y, p = (np.asarray(v) for v in s[:4])
        ok = (t >= 0) & (x >= 0) & (y >= 0) & (p >= 0) & (p <= 1)
        out.append((t[ok], x[ok], y[ok], p[ok], s[4]))
    return out


def _want(samples, table, T_, H_, W_, step, kind, clip=0, scale=1.0):
    n = len(samples)
    table = R.identity_table(n) if table is None else table
    return E.frames_rep_ref(samples, table, T_, n, H_, W_, step, E.NAMES[kind], clip, np.float32(scale)).view(np.uint32)


# ------------------------------------------------------------------------------------------- 1. every rule, per rep
def _all_rules_batch(step):
    """B = 3: ~200 events with every skip / clip rule in them (the batch of the augmented feed's test, here with raw
    times of any offset inside a bin and four events in one cell and bin), an empty sample, 50 events."""
    rng = np.random.default_rng(3)
    t0 = 20_000
    n = 190
    t = rng.integers(t0 - 300, t0 + T * step + 300, n)
    x, y, p = rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)
    end = t0 + T * step
    edge = [  # (t, x, y, p)
        (t0 - 1, 1, 1, 0), (t0, 2, 1, 1), (end - 1, 3, 2, 0), (end, 4, 2, 1),
        (t0 + 10, -2, 3, 0), (t0 + step + 10, W + 3, 3, 1), (t0 + 20, 3, -1, 0), (t0 + 30, 3, H, 1), (t0 + 40, 5, 4, 2),
        (t0 - step, 6, 0, 1),
        # four events in cell (x 4, y 4, p 1) of bin 2, in both halves of the bin and not in time order
        (t0 + 2 * step + step // 2 + 7, 4, 4, 1), (t0 + 2 * step + 3, 4, 4, 1), (t0 + 3 * step - 1, 4, 4, 1),
        (t0 + 2 * step + step // 3, 4, 4, 1)]
    e = np.array(edge, dtype=np.int64)
    s0 = (np.concatenate([t, e[:, 0]]), np.concatenate([x, e[:, 1]]), np.concatenate([y, e[:, 2]]),
          np.concatenate([p, e[:, 3]]), t0)
    empty = tuple(np.zeros(0, dtype=np.int64) for _ in range(4)) + (123,)
    t2 = 90_000
    s2 = (rng.integers(t2, t2 + T * step, 50), rng.integers(-1, W + 1, 50), rng.integers(0, H, 50),
          rng.integers(0, 2, 50), t2)
    return [s0, empty, s2]


ALL_RULES = {
    "identity": dict(),
    "flip": dict(flip=1),
    "zoom_out": dict(a=32768, ox=3, oy=2),
    "zoom_in": dict(a=98304, ox=-2, oy=-1),
    "odd_flip": dict(flip=1, a=40000, ox=-1, oy=1),
    "drop": dict(drop=1 << 31, seeds=[0xDEADBEEF, 12345, 0xFFFFFFFF]),
}


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("rep", list(REPS))
def test_every_rule_per_representation(pkg, rep, step):
    kind, (clip, scale) = _kind(rep), REPS[rep]
    samples = _all_rules_batch(step)
    plain = _want(samples, _table(3), T, H, W, step, kind, clip, scale)
    count = E.accumulators_ref(samples, _table(3), T, 3, H, W, step, E.COUNT)
    assert count[2, 0, 1, 4, 4] >= 4 and count[:, 1].sum() == 0          # the crowded cell; the empty sample
    for case, kw in ALL_RULES.items():
        table = _table(3, **kw)
        want = _want(samples, table, T, H, W, step, kind, clip, scale)
        got = _tuple_frames(pkg, samples, table, T, H, W, step, kind, clip, scale)
        assert want.any() and not want[:, 1].any()
        assert np.array_equal(got, want), (rep, case)
        if case != "identity":
            assert not np.array_equal(want, plain), case                 # the transform is visible in the expected frames
    # without a table: the identity, through both forms (the packed form cannot hold the negative fields)
    assert np.array_equal(_tuple_frames(pkg, samples, None, T, H, W, step, kind, clip, scale), plain)
    packable = _packable(samples)
    for table in (None, _table(3, **ALL_RULES["odd_flip"])):
        assert np.array_equal(_packed_frames(pkg, packable, table, T, H, W, step, kind, clip, scale),
                              _want(packable, table, T, H, W, step, kind, clip, scale)), rep


# ------------------------------------------------------------------------------------------- 2. contention
def _contended(n, hot, H_, W_, step, seed=11):
    """One sample of ``n`` events in a window of T bins; those at the indices ``hot`` fall into cell (x 0, y 1, p 1) of
    bin 1 at different offsets, no other event has x = 0."""
    rng = np.random.default_rng(seed)
    t0 = 2000
    t = t0 + rng.integers(0, T * step, n)
    x, y, p = rng.integers(1, W_, n), rng.integers(0, H_, n), rng.integers(0, 2, n)
    hot = np.asarray(hot)
    t[hot] = t0 + step + (np.arange(hot.size) * 131 + 17) % step
    x[hot], y[hot], p[hot] = 0, 1, 1
    return [(t, x, y, p, t0)]


@pytest.mark.parametrize("kind", ["count", "time", "voxel"])
def test_contended_cell_across_lanes_waves_and_blocks(pkg, kind):
    n, step, H_, W_ = 70_001, 1000, 16, 24
    hot = [0, 63, 64, 255, 256, 70_000]
    samples = _contended(n, hot, H_, W_, step)
    acc = E.accumulators_ref(samples, R.identity_table(1), T, 1, H_, W_, step, E.NAMES[kind])
    r = (np.arange(6) * 131 + 17) % step
    if kind == "count":
        assert acc[1, 0, 1, 1, 0] == 6
    elif kind == "time":
        assert acc[1, 0, 1, 1, 0] == r.max() + 1
    else:
        assert acc[:, 0, 1, 1, 0].sum() == 6 * 65536 and (acc[:3, 0, 1, 1, 0] > 0).sum() >= 2
    for packed in (False, True):
        run = _packed_frames if packed else _tuple_frames
        assert np.array_equal(run(pkg, samples, None, T, H_, W_, step, kind), _want(samples, None, T, H_, W_, step, kind))


@pytest.mark.parametrize("kind", ["count", "time", "voxel"])
def test_grid_stride_loop_reaches_the_tail(pkg, kind):
    """256 * (the launcher's block cap: 8 per compute unit) + 5 events: the last five run in the second trip of the loop
    and land in the cell the first and the 64th event hit.  All but a few events lie before the window."""
    H_, W_, step = 2, 33, 1000
    cap = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    n = 256 * cap + 5
    rng = np.random.default_rng(23)
    t0 = 10_000
    t = np.full(n, t0 - 1, dtype=np.int64)
    live = np.concatenate([[0, 63], rng.choice(np.arange(64, n - 5), 40, replace=False), np.arange(n - 5, n)])
    t[live] = t0 + rng.integers(0, T * step, live.size)
    x, y, p = rng.integers(1, W_, n), rng.integers(0, H_, n), rng.integers(0, 2, n)
    same = np.concatenate([[0, 63], np.arange(n - 5, n)])
    t[same] = t0 + 2 * step + np.array([5, 900, 450, 451, 999, 0, 600])
    x[same], y[same], p[same] = 0, 1, 0
    samples = [(t, x, y, p, t0)]
    assert E.accumulators_ref(samples, R.identity_table(1), T, 1, H_, W_, step, E.COUNT)[2, 0, 0, 1, 0] == 7
    table = _table(1, flip=1, a=50000, ox=4)
    for tab in (None, table):
        assert np.array_equal(_tuple_frames(pkg, samples, tab, T, H_, W_, step, kind), _want(samples, tab, T, H_, W_, step, kind))


# ------------------------------------------------------------------------------------------- 3. order independence
@pytest.mark.parametrize("kind", ["count", "time", "voxel"])
def test_any_order_of_a_samples_events_and_two_runs_give_the_same_bits(pkg, kind):
    step = 16667
    samples = _all_rules_batch(step)
    rng = np.random.default_rng(8)
    shuffled = []
    for s in samples:
        order = rng.permutation(len(s[0]))
        shuffled.append(tuple(np.asarray(v)[order] for v in s[:4]) + (s[4],))
    table = _table(3, **ALL_RULES["odd_flip"])                            # (drop off: the drop hashes the index)
    scale = 1.0 / 3.0
    a = _tuple_frames(pkg, samples, table, T, H, W, step, kind, 0, scale)
    b = _tuple_frames(pkg, shuffled, table, T, H, W, step, kind, 0, scale)
    again = _tuple_frames(pkg, samples, table, T, H, W, step, kind, 0, scale)
    assert a.any() and np.array_equal(a, b) and np.array_equal(a, again)
    assert np.array_equal(a, _want(samples, table, T, H, W, step, kind, 0, scale))


# ------------------------------------------------------------------------------------------- 4. binary = the old entries
def test_binary_through_the_new_entries_equals_the_old_entries(pkg):
    from snn_for_object_detection_amd import _hip
    step = 1000
    samples = _all_rules_batch(step)
    packable = _packable(samples)
    offsets, t0 = _batch_vectors(packable)
    cat = [np.concatenate([np.asarray(s[k]) for s in packable]) for k in range(4)]
    dev = [torch.from_numpy(cat[0].astype(np.int64)).cuda()] + [torch.from_numpy(v.astype(np.int32)).cuda() for v in cat[1:]]
    words = torch.from_numpy(np.concatenate([pkg.pack_events(*s[:4]).reshape(-1, 2) for s in packable]).view(np.int32)).cuda()
    n = int(dev[0].numel())
    shape = (T, 3, H, W, 2)

    def run(entry, events, aug, *rep_args):
        buf = torch.full(shape, float("nan"), device="cuda")
        _hip.call(entry, *(v.data_ptr() for v in events), offsets.data_ptr(), t0.data_ptr(),
                  aug.data_ptr() if aug is not None else None, n, buf.data_ptr(), T, 3, H, W, step, *rep_args, 0)
        return buf.cpu().numpy().view(np.uint32)

    identity = torch.from_numpy(_table(3)).cuda()
    for name in ("identity", "odd_flip", "drop"):
        table = torch.from_numpy(_table(3, **ALL_RULES[name])).cuda()
        old = run("snn_events_to_frames_aug", dev, table)
        assert old.any() and set(np.unique(old)) == {0, np.float32(1.0).view(np.uint32)}
        assert np.array_equal(run("snn_events_to_frames_aug_rep", dev, table, 0, 0, 1.0), old), name
        assert np.array_equal(run("snn_events_to_frames_packed", [words], table), old), name
        assert np.array_equal(run("snn_events_to_frames_packed_rep", [words], table, 0, 0, 1.0), old), name
    old = run("snn_events_to_frames_aug", dev, identity)
    assert np.array_equal(run("snn_events_to_frames_aug_rep", dev, None, 0, 0, 1.0), old)         # NULL table: the identity
    assert np.array_equal(run("snn_events_to_frames_packed", [words], None), old)
    assert np.array_equal(run("snn_events_to_frames_packed_rep", [words], None, 0, 0, 1.0), old)


# ------------------------------------------------------------------------------------------- 5. clip edges
def _cells_with_counts(counts, d):
    """One sample: cell x = i of row 0 gets ``counts[i]`` events at window offset ``d`` (t0 = 0)."""
    x = np.concatenate([np.full(c, i) for i, c in enumerate(counts)])
    return [(np.full(x.size, d), x, np.zeros_like(x), np.ones_like(x), 0)]


def test_clip_edges_and_the_single_rounding_of_the_scale(pkg):
    step, third = 1000, float(np.float32(1.0) / np.float32(3.0))
    f32 = lambda v: np.float32(v).view(np.uint32)                         # noqa: E731
    # count with clip 3: cells of 2, 3, 4 and 7 events; voxel with clip 2: cells of 1, 2, 3 events on a bin centre
    for kind, clip, counts, d in (("count", 3, [2, 3, 4, 7, 0, 1], 10), ("voxel", 2, [1, 2, 3, 0, 5], step + step // 2)):
        samples = _cells_with_counts(counts, d)
        t_bin = d // step
        for scale in (1.0, third):
            got = _tuple_frames(pkg, samples, None, T, H, W, step, kind, clip, scale)
            assert np.array_equal(got, _want(samples, None, T, H, W, step, kind, clip, scale))
            row = got[t_bin, 0, 1, 0, :len(counts)]
            # fl(fl(min(n, clip)) * scale), written out: one rounding of the product
            assert row.tolist() == [int(f32(np.float32(min(c, clip)) * np.float32(scale))) for c in counts], (kind, scale)
            free = _tuple_frames(pkg, samples, None, T, H, W, step, kind, 0, scale)       # clip = 0: unclipped
            assert free[t_bin, 0, 1, 0, :len(counts)].tolist() == [int(f32(np.float32(c) * np.float32(scale))) for c in counts]
            assert np.count_nonzero(got) == np.count_nonzero(counts)                      # empty cells stay +0.0f bits
    assert np.float32(3.0) * np.float32(third) == np.float32(1.0) and f32(np.float32(7) * np.float32(third)) != f32(7 / 3)


# ------------------------------------------------------------------------------------------- 6. time edges
def test_time_surface_edges(pkg):
    f32 = lambda v: int(np.float32(v).view(np.uint32))                    # noqa: E731
    for step in STEPS:
        t0 = 300
        # x 0: r = 0; x 1: r = step - 1; x 2 / x 3: two events, the later first / last in memory; x 4: three equal times
        ev = [(t0 + step, 0), (t0 + 2 * step - 1, 1), (t0 + step + 700, 2), (t0 + step + 30, 2), (t0 + step + 30, 3),
              (t0 + step + 700, 3), (t0 + step + 5, 4), (t0 + step + 5, 4), (t0 + step + 5, 4)]
        t, x = (np.array(v) for v in zip(*ev))
        samples = [(t, x, np.full(t.size, 2), np.zeros_like(t), t0)]
        got = _tuple_frames(pkg, samples, None, T, H, W, step, "time")
        assert np.array_equal(got, _want(samples, None, T, H, W, step, "time"))
        s = np.float32(step)
        assert got[1, 0, 0, 2, :5].tolist() == [f32(np.float32(1) / s), f32(1.0), f32(np.float32(701) / s),
                                                 f32(np.float32(701) / s), f32(np.float32(6) / s)]
        assert np.count_nonzero(got) == 5
    # fl(m) past 2^24: one bin of 2^25 + 3 microseconds
    step = (1 << 25) + 3
    r = np.array([0, (1 << 24), (1 << 24) + 1, (1 << 24) + 2, (1 << 25) - 2, (1 << 25) + 1, step - 1])
    samples = [(7 + r, np.arange(r.size), np.zeros_like(r), np.ones_like(r), 7)]
    got = _tuple_frames(pkg, samples, None, 1, H, W, step, "time")
    want = _want(samples, None, 1, H, W, step, "time")
    assert np.array_equal(got, want)
    m = (r + 1).astype(np.uint64)
    assert any(int(np.float32(v)) != int(v) for v in m)                   # some m are not fp32 numbers
    assert got[0, 0, 1, 0, :r.size].tolist() == [f32(np.float32(v) / np.float32(step)) for v in m]
    assert got[0, 0, 1, 0, r.size - 1] == f32(1.0)                        # fl(step) / fl(step)


# ------------------------------------------------------------------------------------------- 7. voxel edges
@pytest.mark.parametrize("T_", [4, 1])
def test_voxel_edges(pkg, T_):
    for step in STEPS + (2,):
        half = step // 2
        ds = sorted({0, max(half - 1, 0), half, half + 1, step - 1, T_ * step - 1, (T_ - 1) * step + half,
                     min(T_ * step - 1, step + half + 1)})
        ds = [v for v in ds if v < T_ * step]
        d = np.array(ds)
        samples = [(50 + d, np.arange(d.size) % W, np.arange(d.size) // W, np.ones_like(d), 50)]
        got = _tuple_frames(pkg, samples, None, T_, H, W, step, "voxel")
        assert np.array_equal(got, _want(samples, None, T_, H, W, step, "voxel")), step
        acc = E.accumulators_ref(samples, R.identity_table(1), T_, 1, H, W, step, E.VOXEL)
        # fp32 holds every weight <= 2^16 exactly: the frames are the accumulators times 2^-16
        assert np.array_equal(got.view(np.float32) * np.float32(65536), acc.astype(np.float32))
        for i, di in enumerate(ds):
            k, w0, w1 = (int(v[0]) for v in E.voxel_weights(np.array([di]), T_, step))
            col = acc[:, 0, 1, i // W, i % W]
            kept = (w0 if k >= 0 else 0) + (w1 if k + 1 <= T_ - 1 else 0)
            assert int(col.sum()) == kept and (kept == 65536 or k == -1 or k == T_ - 1), (step, di)
            if T_ == 1:
                assert kept < 65536 or 2 * di == step                     # only an event on the one centre keeps it all


# ------------------------------------------------------------------------------------------- 8. B past the LDS tables
@pytest.mark.parametrize("kind", ["count", "time", "voxel"])
def test_sample_lookup_over_many_short_samples(pkg, kind):
    """B = 70 (offsets, window starts and tables are read from global memory), 0 to 9 events each, the first and the last
    sample empty, a different table per sample; the same batch in two halves takes the LDS-staged path."""
    n_b, H_, W_, step = 70, 2, 9, 1000
    rng = np.random.default_rng(17)
    counts = rng.integers(0, 10, n_b)
    counts[[0, 5, 6, n_b - 1]] = 0
    samples = []
    for b in range(n_b):
        n, t0 = int(counts[b]), 1000 * b - 7000
        samples.append((rng.integers(t0 - 100, t0 + T * step + 100, n), rng.integers(-1, W_ + 1, n),
                        rng.integers(0, H_, n), rng.integers(0, 2, n), t0))
    table = R.identity_table(n_b)
    table[:, 0] = rng.integers(0, 2, n_b)
    table[:, 1] = rng.integers(40000, 100000, n_b)
    table[:, 2] = rng.integers(-3, 4, n_b)
    table[:, 3] = rng.integers(-1, 2, n_b)
    table[::3, 4] = np.array([1 << 30], dtype=np.uint32).view(np.int32)[0]
    table[:, 5] = rng.integers(0, 1 << 32, n_b, dtype=np.uint64).astype(np.uint32).view(np.int32)
    want = _want(samples, table, T, H_, W_, step, kind)
    assert np.count_nonzero(want) > 50
    assert np.array_equal(_tuple_frames(pkg, samples, table, T, H_, W_, step, kind), want)
    assert np.array_equal(_tuple_frames(pkg, samples, None, T, H_, W_, step, kind), _want(samples, None, T, H_, W_, step, kind))
    for lo in (0, 35):
        part = _tuple_frames(pkg, samples[lo:lo + 35], table[lo:lo + 35], T, H_, W_, step, kind)
        assert np.array_equal(part, want[:, lo:lo + 35])


# ------------------------------------------------------------------------------------------- 9. finalize tails
@pytest.mark.parametrize("kind", ["count", "time", "voxel"])
def test_finalize_head_tail_and_unaligned_frames(pkg, kind):
    """30 elements at every 4-byte offset inside a sentinel-filled buffer (a 16-byte aligned allocation): scalar head, whole
    uint4s and scalar tail of every length, through the packed entry; the guard elements come back untouched."""
    from snn_for_object_detection_amd import _hip
    T_, H_, W_, step, guard = 1, 3, 5, 1000, 8
    rng = np.random.default_rng(4)
    n = 120
    samples = [(rng.integers(0, step, n), rng.integers(0, W_, n), rng.integers(0, H_, n), rng.integers(0, 2, n), 0)]
    want = _want(samples, None, T_, H_, W_, step, kind, 0, 0.5)
    assert np.count_nonzero(want) >= 25
    words = torch.from_numpy(pkg.pack_events(*samples[0][:4]).view(np.int32)).cuda()
    offsets, t0 = _batch_vectors(samples)
    sentinel = np.float32(-123.25)
    for lead in range(guard - 3, guard + 1):                               # the frames start 4 * lead bytes into the buffer
        buf = torch.full((2 * guard + 30,), float(sentinel), device="cuda")
        assert buf.data_ptr() % 16 == 0
        _hip.call("snn_events_to_frames_packed_rep", words.data_ptr(), offsets.data_ptr(), t0.data_ptr(), None, n,
                  buf.data_ptr() + 4 * lead, T_, 1, H_, W_, step, E.NAMES[kind], 0, 0.5, 0)
        host = buf.cpu().numpy()
        assert (host[:lead] == sentinel).all() and (host[lead + 30:] == sentinel).all(), lead
        got = host[lead:lead + 30].view(np.uint32).reshape(1, 1, H_, W_, 2).transpose(0, 1, 4, 2, 3)
        assert np.array_equal(got, want), lead


# ------------------------------------------------------------------------------------------- 10. no events
@pytest.mark.parametrize("kind", ["binary", "count", "time", "voxel"])
def test_no_events_zero_fills(pkg, kind):
    from snn_for_object_detection_amd import _hip
    offsets = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
    t0 = torch.zeros(B, dtype=torch.int64, device="cuda")
    for entry, lead_ptrs in (("snn_events_to_frames_aug_rep", 4), ("snn_events_to_frames_packed_rep", 1)):
        buf = torch.full((T, B, H, W, 2), float("nan"), device="cuda")
        _hip.call(entry, *([None] * lead_ptrs), offsets.data_ptr(), t0.data_ptr(), None, 0, buf.data_ptr(), T, B, H, W, 1000,
                  E.NAMES[kind], 0, 1.0, 0)
        assert not buf.cpu().numpy().view(np.uint32).any(), entry           # +0.0f bits everywhere
    empty = tuple(np.zeros(0, dtype=np.int64) for _ in range(4)) + (5,)
    assert not _tuple_frames(pkg, [empty] * 2, None, T, H, W, 1000, kind).any()


# ------------------------------------------------------------------------------------------- 11. refusals
def test_refusals_by_name_from_the_library(pkg):
    from snn_for_object_detection_amd import _hip
    i64 = torch.zeros(8, dtype=torch.int64, device="cuda")
    i32 = torch.zeros(16, dtype=torch.int32, device="cuda")
    buf = torch.full((T * 2 * H * W * 2,), 7.0, device="cuda")
    tuple_args = [i64.data_ptr(), i32.data_ptr(), i32.data_ptr(), i32.data_ptr(), i64.data_ptr(), i64.data_ptr(),
                  i32.data_ptr(), 4, buf.data_ptr(), T, 2, H, W, 1000, 1, 0, 1.0, 0]
    packed_args = [i32.data_ptr(), i64.data_ptr(), i64.data_ptr(), i32.data_ptr(), 4, buf.data_ptr(), T, 2, H, W, 1000, 1,
                   0, 1.0, 0]
    for entry, args, first in (("snn_events_to_frames_aug_rep", tuple_args, 7), ("snn_events_to_frames_packed_rep", packed_args, 4)):
        n_at, frames_at, T_at, step_at, rep_at, clip_at, scale_at = first, first + 1, first + 2, first + 6, first + 7, first + 8, first + 9

        def refused(match, **change):
            a = list(args)
            for k, v in change.items():
                a[int(k[1:])] = v
            with pytest.raises(RuntimeError, match=entry + ".*" + match):
                _hip.call(entry, *a)

        rep = lambda r, **kw: {f"_{rep_at}": r, **kw}                      # noqa: E731
        refused("unknown representation", **rep(4))
        refused("unknown representation", **rep(-1))
        refused("clip", **rep(0, **{f"_{clip_at}": 1}))
        refused("clip", **rep(1, **{f"_{clip_at}": (1 << 24) + 1}))
        refused("clip", **rep(1, **{f"_{clip_at}": -1}))
        refused("clip", **rep(2, **{f"_{clip_at}": 1}))
        refused("clip", **rep(3, **{f"_{clip_at}": 65536}))
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused("scale", **rep(1, **{f"_{scale_at}": bad}))
        refused("scale 1 only", **rep(0, **{f"_{scale_at}": 2.0}))
        refused("step_us .* too large", **rep(2, **{f"_{step_at}": 1 << 32, f"_{T_at}": 1}))
        refused("step_us .* too large", **rep(3, **{f"_{step_at}": 1 << 40, f"_{T_at}": 1}))
        for r in (1, 2, 3):
            refused("n_events", **rep(r, **{f"_{n_at}": 1 << 32}))
        # the checks the entries share with the entries without a representation, under the new names
        refused("step_us must be positive", **{f"_{step_at}": 0})
        refused("step_us must be positive", **{f"_{step_at}": -5})
        refused("null pointer", **{f"_{frames_at}": None})
        refused("null pointer", **{f"_{first - 3}": None})                  # offsets
        refused("null pointer", **{f"_{first - 2}": None})                  # t0
        refused("null event", _0=None)
        refused("bad shape", **{f"_{T_at}": 0})
        refused("bad shape", **{f"_{n_at}": -1})
        refused("2\\^31 elements", **{f"_{T_at}": 1 << 14, f"_{T_at + 1}": 1 << 14, f"_{T_at + 2}": 2, f"_{T_at + 3}": 2})
        refused("overflows", **{f"_{step_at}": 1 << 62, f"_{rep_at}": 1})
    refused_packed = list(packed_args)
    refused_packed[0] = i32.data_ptr() + 4
    with pytest.raises(RuntimeError, match="snn_events_to_frames_packed_rep.*8-byte aligned"):
        _hip.call("snn_events_to_frames_packed_rep", *refused_packed)
    other = torch.zeros_like(buf)
    no_table = list(tuple_args)
    no_table[6], no_table[8] = None, other.data_ptr()
    _hip.call("snn_events_to_frames_aug_rep", *no_table)                     # aug NULL is no refusal
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())                                          # every refusal came before any launch or fill


# ------------------------------------------------------------------------------------------- 12. API
def _api_batch(n_b, T_, H_, W_, step, n=1500, seed=9):
    rng = np.random.default_rng(seed)
    samples, labels = [], []
    for b in range(n_b):
        t0 = 4000 * (b + 1)
        ev = (np.sort(rng.integers(max(t0 - 200, 0), t0 + T_ * step + 200, n)), rng.integers(0, W_ + 2, n),
              rng.integers(0, H_, n), rng.integers(0, 2, n))
        samples.append(ev + (t0,))
        labels.append(torch.tensor([[0, 0.2, 0.2, 0.5, 0.6], [1, 0.5, 0.4, 0.9, 0.8], [1, 0.0, 0.1, 0.3, 1.0]][:b + 1]))
    return samples, labels


def _host(samples):
    return [tuple(torch.from_numpy(np.asarray(v)) for v in s[:4]) + (s[4],) for s in samples]


def test_batcher_count_frames_equal_the_reference(pkg):
    n_b, T_, H_, W_, step = 3, 4, 12, 20, 1000
    samples, labels = _api_batch(n_b, T_, H_, W_, step)
    rep = pkg.EventRepresentation("count", clip=3, scale=0.5)
    batcher = pkg.EventBatcher(T_, H_, W_, step, representation=rep)
    assert batcher.representation is rep and pkg.EventBatcher(T_, H_, W_, step).representation.is_binary
    plain = pkg.EventBatcher(T_, H_, W_, step, representation="count")
    binary = pkg.EventBatcher(T_, H_, W_, step)
    X0, lab0 = binary(_host(samples), labels)
    # un-augmented tuple samples (no table is read), with and without labels
    X, lab = plain(_host(samples), labels)
    want = _want(samples, None, T_, H_, W_, step, "count")
    assert X.shape == (T_, n_b, 2, H_, W_) and X.stride() == X0.stride()
    assert np.array_equal(_bits(X), want) and want.view(np.float32).max() >= 2 and plain.last_aug_table is None
    assert torch.equal(lab, lab0) and torch.equal(X != 0, X0 != 0)
    assert np.array_equal(_bits(batcher(_host(samples))), _want(samples, None, T_, H_, W_, step, "count", 3, 0.5))
    # an explicit table: events and boxes under the same transform as the binary batcher's
    table = pkg.EventAugment.identity(n_b)
    table[:, 0] = 1
    table[1, 1:4] = torch.tensor([50000, 3, 2], dtype=torch.int32)
    X1, lab1 = batcher(_host(samples), labels, aug_table=table)
    X1b, lab1b = binary(_host(samples), labels, aug_table=table)
    assert np.array_equal(_bits(X1), _want(samples, table.numpy(), T_, H_, W_, step, "count", 3, 0.5))
    assert torch.equal(lab1, lab1b) and torch.equal(X1 != 0, X1b != 0) and torch.equal(batcher.last_aug_table, table)
    # packed samples, with and without a table; an EventAugment draws as it does for the binary batcher
    packed = [(pkg.pack_events(*s[:4]), s[4]) for s in samples]
    assert np.array_equal(_bits(batcher(packed)), _want(samples, None, T_, H_, W_, step, "count", 3, 0.5))
    X2, lab2 = batcher(packed, labels, aug_table=table)
    assert torch.equal(X2, X1) and torch.equal(lab2, lab1)
    kw = dict(hflip=0.5, zoom=(0.75, 1.25), drop=(0.0, 0.2), seed=3)
    drawn = pkg.EventBatcher(T_, H_, W_, step, augment=pkg.EventAugment(**kw), representation="voxel")
    drawn_b = pkg.EventBatcher(T_, H_, W_, step, augment=pkg.EventAugment(**kw))
    X3, X3b = drawn(packed), drawn_b(packed)
    assert torch.equal(drawn.last_aug_table, drawn_b.last_aug_table)
    assert np.array_equal(_bits(X3), _want(samples, drawn.last_aug_table.numpy(), T_, H_, W_, step, "voxel"))
    assert np.array_equal(_bits(drawn(_host(samples), augment=False)), _want(samples, None, T_, H_, W_, step, "voxel"))
    assert float(X3b.sum()) > 0


FEED = dict(dataset="gen1", split="train", batch_size=2, num_steps=4, time_step=1, time_shift=2, events_threshold=10,
            files_in_flight=2, seed=4)


def test_prophesee_feed_time_surface_on_synthetic_recordings(pkg, tmp_path):
    d = tmp_path / "gen1" / "train"
    d.mkdir(parents=True)
    for i in range(2):
        rng = np.random.default_rng(40 + i)
        ev = S.stream(rng, 304, 240, 60_000, per_ms=60 + 20 * i)
        pkg.write_dat(str(d / f"r{i}_td.dat"), pkg.pack_events(*ev), 304, 240)
        np.save(str(d / f"r{i}_bbox.npy"), S.walk_boxes(1000, 304, 240, steps=(10, 20, 30, 40, 50), small=()))
    rep = pkg.EventRepresentation("time", scale=2.0)
    feed = pkg.PropheseeFeed(str(tmp_path), representation=rep, **FEED)
    binary = pkg.PropheseeFeed(str(tmp_path), **FEED)
    order = pkg.PropheseeFeed(str(tmp_path), **FEED).samples()                # the same seed: the same samples
    for _ in range(2):
        X, labels = next(feed)
        Xb, labels_b = next(binary)
        batch = [next(order) for _ in range(FEED["batch_size"])]
        samples = [pkg.unpack_events(np.asarray(w)) + (int(t0),) for w, t0, _ in batch]
        want = _want(samples, None, 4, 240, 304, 1000, "time", 0, 2.0)
        assert X.shape == (4, 2, 2, 240, 304) and np.array_equal(_bits(X), want)
        assert torch.equal(labels, labels_b) and torch.equal(X != 0, Xb != 0) and float(X.max()) <= 2.0
        assert np.count_nonzero(want) > 100


def test_a_training_step_sees_the_frames_alone(pkg):
    """The representation is the feed's business only: the step on ``count`` frames from the batcher and the step on the
    same values handed in as a plain tensor give the same loss bits."""
    n_b, T_, H_, W_, step = 2, 2, 32, 48, 1000
    samples, labels = _api_batch(n_b, T_, H_, W_, step, n=2500)
    X, lab = pkg.EventBatcher(T_, H_, W_, step, representation="count")(_host(samples), labels)
    want = _want(samples, None, T_, H_, W_, step, "count")
    assert np.array_equal(_bits(X), want) and want.view(np.float32).max() >= 2
    plain = torch.from_numpy(want.view(np.float32).copy()).cuda()              # a dense NCHW tensor of the same values
    losses = []
    for frames in (X, plain):
        torch.manual_seed(2)
        model = pkg.TinyYolo(num_classes=2, time_window=0).cuda().train()
        loss = model.training_step((frames, lab))
        loss.backward()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss))
        losses.append(loss.detach().cpu().numpy().view(np.uint32).copy())
    assert np.array_equal(losses[0], losses[1])
