"""The packed event feed on the GPU: ``snn_events_to_frames_packed`` bit for bit against the integer reference of
``tests/event_aug_ref.py`` on the unpacked events and against ``snn_events_to_frames_aug`` on the same events,
``EventBatcher`` with packed samples against its 5-tuple paths, and ``PropheseeFeed`` end to end against
``oracle/events.py``.  Frames are binary and every rule is an integer rule: all comparisons are exact."""
import numpy as np
import pytest
import torch

from oracle import events as O
from tests import event_aug_ref as R
from tests import recordings_ref as S

pytestmark = pytest.mark.gpu

T, H, W, STEP = 3, 6, 9, 1000


@pytest.fixture(scope="module")
def pkg(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import snn_for_object_detection_amd as p
    return p


def _dev_words(words, lead=0):
    """Host records -> a device int32 [n, 2] tensor that starts ``lead`` records into its allocation."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    pad = np.full((lead, 2), 0xFFFFFFFF, dtype=np.uint32)
    return torch.from_numpy(np.concatenate([pad, words]).view(np.int32)).cuda()[lead:]


def _table(B, flip=0, a=65536, ox=0, oy=0, drop=0, seeds=None):
    t = R.identity_table(B)
    t[:, 0], t[:, 1], t[:, 2], t[:, 3] = flip, a, ox, oy
    t[:, 4] = np.array([drop], dtype=np.uint32).view(np.int32)[0]
    if seeds is not None:
        t[:, 5] = np.array(seeds, dtype=np.uint32).view(np.int32)
    return t


def _check(pkg, words_list, t0s, table, T=T, H=H, W=W, step=STEP, lead=0, against_aug=True):
    """The packed kernel on samples given as record arrays: equal to ``frames_ref`` of the unpacked events, and to the
    tuple kernel ``snn_events_to_frames_aug`` on them.  ``table`` None launches without a table.  -> the uint8 frames."""
    from snn_for_object_detection_amd import functional as HF
    B = len(words_list)
    words = np.concatenate([np.asarray(w, dtype=np.uint32).reshape(-1, 2) for w in words_list])
    offsets = torch.tensor(np.cumsum([0] + [len(w) for w in words_list]), dtype=torch.int64).cuda()
    t0 = torch.tensor([int(v) for v in t0s], dtype=torch.int64).cuda()
    aug = None if table is None else torch.from_numpy(table).cuda()
    X = HF.events_to_frames_packed(_dev_words(words, lead), offsets, t0, aug, T, B, H, W, step)
    assert X.shape == (T, B, 2, H, W) and HF.is_channels_last(X)
    assert all(float(v) in (0.0, 1.0) for v in torch.unique(X))
    unpacked = [pkg.unpack_events(w) + (int(t),) for w, t in zip(words_list, t0s)]
    ref_table = R.identity_table(B) if table is None else table
    want = R.frames_ref(unpacked, ref_table, T, B, H, W, step)
    got = X.cpu().numpy().astype(np.uint8)
    assert np.array_equal(got, want)
    if against_aug:
        cat = [np.concatenate([u[k] for u in unpacked]) for k in range(4)]
        dev = [torch.from_numpy(cat[0]).cuda()] + [torch.from_numpy(v).cuda() for v in cat[1:]]
        Y = HF.events_to_frames_aug(*dev, offsets, t0, torch.from_numpy(ref_table).cuda(), T, H, W, step)
        assert torch.equal(X, Y)
    return got


def _sample(pkg, rng, n, t0, T=T, H=H, W=W, step=STEP, x_hi=None, y_hi=None):
    """``n`` records around the window of ``t0`` (some before and after it), x past the frame, y past it."""
    t = np.sort(rng.integers(max(t0 - step // 2, 0), t0 + T * step + step // 2, n))
    x = rng.integers(0, (W + 3) if x_hi is None else x_hi, n)
    y = rng.integers(0, (H + 2) if y_hi is None else y_hi, n)
    return pkg.pack_events(t, x, y, rng.integers(0, 2, n))


# ------------------------------------------------------------------------------------------- batch layout
@pytest.mark.parametrize("empty", [(0,), (1,), (2,), (0, 2), (0, 1, 2)])
def test_empty_samples_first_middle_last(pkg, empty):
    rng = np.random.default_rng(1)
    counts = [0 if b in empty else 41 + 10 * b for b in range(3)]
    t0s = [5000, 70_000, 1000]
    got = _check(pkg, [_sample(pkg, rng, c, t0) for c, t0 in zip(counts, t0s)], t0s, None)
    for b in range(3):
        assert (got[:, b].sum() == 0) == (b in empty)


def test_more_samples_than_the_lds_table_holds(pkg):
    rng = np.random.default_rng(2)
    B = 65
    counts = [int(c) for c in rng.integers(0, 9, B)]
    counts[64] = 7
    t0s = [1000 * (b + 1) for b in range(B)]
    words = [_sample(pkg, rng, c, t0) for c, t0 in zip(counts, t0s)]
    got = _check(pkg, words, t0s, None)
    assert got[:, 64].sum() > 0
    table = _table(B, flip=1, a=50000, ox=1, oy=1, drop=1 << 30, seeds=list(range(B)))
    _check(pkg, words, t0s, table)


def test_no_events_zero_fills(pkg):
    from snn_for_object_detection_amd import functional as HF
    offsets, t0 = torch.zeros(3, dtype=torch.int64).cuda(), torch.zeros(2, dtype=torch.int64).cuda()
    stale = torch.ones((T, 2, H, W, 2), device="cuda")                          # freed memory full of ones
    del stale
    X = HF.events_to_frames_packed(torch.zeros((0, 2), dtype=torch.int32).cuda(), offsets, t0, None, T, 2, H, W, STEP)
    assert X.shape == (T, 2, 2, H, W) and float(X.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------- alignment and grid
@pytest.mark.parametrize("lead", [0, 1, 3])
def test_slices_at_odd_event_indices_and_an_odd_total(pkg, lead):
    rng = np.random.default_rng(3)
    counts, t0s = [33, 1, 57, 0, 14], [2000, 3000, 0, 9, 40_000]                 # slices start at 33, 34, 91, 91; n = 105
    assert sum(counts) % 2 == 1
    words = [_sample(pkg, rng, c, t0) for c, t0 in zip(counts, t0s)]
    _check(pkg, words, t0s, None, lead=lead)
    _check(pkg, words, t0s, _table(5, flip=1, ox=1), lead=lead)


def test_more_events_than_one_pass_of_the_grid(pkg):
    """``snn_grid_for`` caps the grid at 8 blocks of 256 threads per compute unit: the events behind that many are reached
    by the grid-stride loop alone.  Everything in the first pass lies before the window, so every set cell comes from
    the second pass."""
    rng = np.random.default_rng(4)
    one_pass = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    tail = 1001
    t0 = 1 << 20
    head = pkg.pack_events(np.sort(rng.integers(0, t0, one_pass)), rng.integers(0, W, one_pass),
                           rng.integers(0, H, one_pass), rng.integers(0, 2, one_pass))
    late = _sample(pkg, rng, tail, t0)
    late = late[pkg.unpack_events(late)[0] >= t0]
    words = np.concatenate([head, late])
    split = one_pass // 3                                                       # two samples: the second spans the pass boundary
    got = _check(pkg, [words[:split], words[split:]], [t0, t0], None)
    assert got[:, 0].sum() == 0 and got[:, 1].sum() > 50
    _check(pkg, [words[:split], words[split:]], [t0, t0], _table(2, drop=1 << 31, seeds=[5, 6]))


# ------------------------------------------------------------------------------------------- timestamps and time step
def test_timestamps_and_window_starts_past_2_to_the_31(pkg):
    rng = np.random.default_rng(5)
    t0s = [(1 << 31) + 12_345, (1 << 32) - T * STEP, (1 << 31) - STEP]          # the last window straddles 2^31
    words = [_sample(pkg, rng, 200, t0) for t0 in t0s[:1]]
    t = np.sort(rng.integers((1 << 32) - 2 * T * STEP, 1 << 32, 200))           # up to the last timestamp of the field
    t[-1] = (1 << 32) - 1
    words.append(pkg.pack_events(t, rng.integers(0, W, 200), rng.integers(0, H, 200), rng.integers(0, 2, 200)))
    words.append(_sample(pkg, rng, 200, t0s[2]))
    got = _check(pkg, words, t0s, None)
    assert all(got[:, b].sum() > 20 for b in range(3)) and got[T - 1, 1].sum() > 0


def test_window_starts_below_zero_and_after_every_event(pkg):
    rng = np.random.default_rng(6)
    early = pkg.pack_events(np.sort(rng.integers(0, 2 * STEP, 150)), rng.integers(0, W, 150), rng.integers(0, H, 150),
                            rng.integers(0, 2, 150))
    t0s = [-STEP - 1, -(1 << 40), 10 * STEP, (1 << 32) + 5, 0]
    got = _check(pkg, [early] * 5, t0s, None)
    assert got[:, 0].sum() > 0 and got[0, 0].sum() == 0                         # bins 1 and 2 only (bin 0 lies below t = 0)
    assert got[:, 1].sum() == 0 and got[:, 2].sum() == 0 and got[:, 3].sum() == 0
    assert got[:2, 4].sum() > 0 and got[2, 4].sum() == 0


@pytest.mark.parametrize("step", [(1 << 32) // 3 + 1, 1 << 31, (1 << 33) + 7])
def test_windows_longer_than_2_to_the_32_take_the_wide_division(pkg, step):
    assert T * step > 1 << 32
    rng = np.random.default_rng(7)
    n = 300
    t = np.sort(rng.integers(0, 1 << 32, n))
    t[0], t[-1] = 0, (1 << 32) - 1
    words = pkg.pack_events(t, rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n))
    t0s = [0, -step, -(T - 1) * step - 5, 1 << 31]
    got = _check(pkg, [words] * 4, t0s, None, step=step)
    assert got[0, 0].sum() > 0 and got[1, 1].sum() > 0 and got[T - 1, 2].sum() > 0 and got[0, 3].sum() > 0
    _check(pkg, [words] * 4, t0s, _table(4, flip=1, a=40000, oy=2), step=step)


# ------------------------------------------------------------------------------------------- field edges
def test_field_edges(pkg):
    t0 = 4000
    #        t          x      y      p
    rows = [(t0,        16383, 0,     1),       # x field full: clipped to W - 1
            (t0 + 1,    W,     1,     0),       # one past the frame: clipped
            (t0 + 2,    W - 1, H - 1, 1),       # the last cell
            (t0 + 3,    2,     H,     0),       # y == H: dropped
            (t0 + 4,    3,     16383, 1),       # y field full: dropped
            (t0 + 1000, 0,     0,     0),
            (t0 + 2999, 4,     2,     1),       # the last microsecond of the window
            (t0 + 3000, 5,     3,     1),       # the first after it: dropped
            (t0 - 1,    6,     4,     0)]       # the last before it: dropped
    rows.sort()
    e = np.array(rows, dtype=np.int64)
    words = pkg.pack_events(e[:, 0], e[:, 1], e[:, 2], e[:, 3])
    got = _check(pkg, [words], [t0], None)
    want = np.zeros((T, 1, 2, H, W), dtype=np.uint8)
    want[0, 0, 1, 0, W - 1] = want[0, 0, 0, 1, W - 1] = want[0, 0, 1, H - 1, W - 1] = 1
    want[1, 0, 0, 0, 0] = want[2, 0, 1, 2, 4] = 1
    assert np.array_equal(got, want)
    high = words.copy()
    high[:, 1] |= np.uint32(0xE0000000)                                         # bits 29-31 are not read
    high[::2, 1] ^= np.uint32(0x40000000)
    assert np.array_equal(_check(pkg, [high], [t0], None), want)
    assert np.array_equal(_check(pkg, [high], [t0], _table(1, flip=1))[..., ::-1], want)


# ------------------------------------------------------------------------------------------- random words
@pytest.mark.parametrize("step,H,W", [(1 << 30, 6, 9), (1 << 31, 6, 9), (1 << 30, 1 << 14, 9)])
def test_random_words_and_an_out_of_range_shift_stay_inside_the_frames(pkg, step, H, W):
    """All 32 bits of both words random, a table whose shifts and zooms are out of any sensible range: the frames equal
    the reference and the guard elements on both sides of them keep their value.  (A random y field lies inside six
    rows once in 2 700 events; the frame as high as the field takes every y.)"""
    from snn_for_object_detection_amd import _hip
    rng = np.random.default_rng(8)
    B, n = 4, 4096
    words = rng.integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(np.uint32)
    bounds = [0, 1000, 1001, 3000, n]
    table = _table(B, seeds=[1, 2, 3, 4])
    table[0, :5] = (1, 1 << 18, 0x7FFFFFFF, -0x80000000, 1 << 29)
    table[1, :5] = (0, 0x7FFFFFFF, -5, 3, 0)
    table[2, :5] = (7, -65536, W, H, -1)
    table[3, :5] = (0, 1 << 14, 2, 1, 1 << 30)
    t0s = [0, -step, 1 << 31, 12345]
    offsets = torch.tensor(bounds, dtype=torch.int64).cuda()
    t0 = torch.tensor(t0s, dtype=torch.int64).cuda()
    cells, guard = T * B * H * W * 2, 4096
    unpacked = [pkg.unpack_events(words[bounds[b]:bounds[b + 1]]) + (t0s[b],) for b in range(B)]
    for tab in (table, None):
        mem = torch.full((guard + cells + guard,), 7.0, device="cuda")
        frames = mem[guard:guard + cells]
        dev = _dev_words(words, lead=1)
        aug = None if tab is None else torch.from_numpy(tab).cuda()
        _hip.call("snn_events_to_frames_packed", dev.data_ptr(), offsets.data_ptr(), t0.data_ptr(),
                  None if aug is None else aug.data_ptr(), n, frames.data_ptr(), T, B, H, W, step,
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        host = mem.cpu().numpy()
        assert (host[:guard] == 7.0).all() and (host[guard + cells:] == 7.0).all()
        got = host[guard:guard + cells].reshape(T, B, H, W, 2).transpose(0, 1, 4, 2, 3).astype(np.uint8)
        want = R.frames_ref(unpacked, R.identity_table(B) if tab is None else tab, T, B, H, W, step)
        assert np.array_equal(got, want)
        if H == 1 << 14:
            assert want.sum() > 100


# ------------------------------------------------------------------------------------------- augmentation
def test_flip_zoom_shift_drop_and_null_is_the_identity(pkg):
    rng = np.random.default_rng(9)
    H2, W2 = 24, 37
    t0s = [1000, 50_000, 7]
    words = [_sample(pkg, rng, 1500, t0, H=H2, W=W2) for t0 in t0s]
    plain = _check(pkg, words, t0s, None, H=H2, W=W2)
    assert np.array_equal(_check(pkg, words, t0s, _table(3), H=H2, W=W2), plain)
    table = _table(3, seeds=[11, 12, 13])
    table[0, :5] = (1, 45000, 3, 2, 1 << 30)
    table[1, :5] = (0, 100000, -9, -4, -(1 << 31))                             # the bits of 2^31: half the events
    table[2, :5] = (1, 65536, -3, 1, 0)
    got = _check(pkg, words, t0s, table, H=H2, W=W2)
    assert all(0 < got[:, b].sum() and not np.array_equal(got[:, b], plain[:, b]) for b in range(3))


def test_bad_arguments_raise_by_name(pkg):
    from snn_for_object_detection_amd import _hip, functional as HF
    w = torch.zeros((4, 2), dtype=torch.int32).cuda()
    off, t0 = torch.tensor([0, 2, 4]).cuda(), torch.zeros(2, dtype=torch.int64).cuda()
    with pytest.raises(ValueError, match="step_us"):
        HF.events_to_frames_packed(w, off, t0, None, T, 2, H, W, 0)
    for bad in (w.cpu(), w.long(), w.reshape(-1), w.reshape(2, 4), w.t()):
        with pytest.raises(ValueError, match="words"):
            HF.events_to_frames_packed(bad, off, t0, None, T, 2, H, W, STEP)
    for kw in (dict(offsets=off[:2]), dict(t0=t0.int()), dict(aug=torch.zeros(8, dtype=torch.int32).cuda())):
        args = dict(offsets=off, t0=t0, aug=None)
        args.update(kw)
        with pytest.raises(ValueError, match="offsets int64"):
            HF.events_to_frames_packed(w, args["offsets"], args["t0"], args["aug"], T, 2, H, W, STEP)
    buf = torch.empty((T, 2, H, W, 2), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    good = [w.data_ptr(), off.data_ptr(), t0.data_ptr(), None, 4, buf.data_ptr(), T, 2, H, W, STEP, st]
    for at, value, name in ((10, 0, "step_us"), (10, -5, "step_us"), (1, None, "null"), (2, None, "null"),
                            (5, None, "null"), (0, None, "null event words"), (6, 0, "bad shape"), (4, -1, "bad shape"),
                            (10, (1 << 62), "overflows"), (9, 1 << 30, "2\\^31"), (0, w.data_ptr() + 4, "aligned")):
        a = list(good)
        a[at] = value
        with pytest.raises(RuntimeError, match="snn_events_to_frames_packed.*" + name):
            _hip.call("snn_events_to_frames_packed", *a)


# ------------------------------------------------------------------------------------------- EventBatcher
def _tuple_and_packed(pkg, rng, B, n, H2, W2, t_base):
    tuples, packed = [], []
    for b in range(B):
        c = 0 if b == 1 else n + 17 * b
        t0 = t_base + 10_000 * b
        w = _sample(pkg, rng, c, t0, H=H2, W=W2)
        t, x, y, p = pkg.unpack_events(w)
        tuples.append(tuple(torch.from_numpy(v) for v in (t, x, y, p)) + (t0,))
        packed.append((w if b % 2 else torch.from_numpy(w.view(np.int32)), t0))   # numpy and torch forms
    labels = [torch.tensor([[0, 0.2, 0.2, 0.5, 0.6], [1, 0.5, 0.4, 0.9, 0.8]][:1 + b % 2]) for b in range(B)]
    return tuples, packed, labels


def test_batcher_packed_samples_equal_tuple_samples_on_consecutive_calls(pkg):
    rng = np.random.default_rng(10)
    H2, W2, B = 20, 31, 4
    plain = pkg.EventBatcher(T, H2, W2, STEP)
    aug_a = pkg.EventBatcher(T, H2, W2, STEP, augment=pkg.EventAugment(hflip=0.5, zoom=(0.75, 1.25), drop=(0.0, 0.2), seed=3))
    aug_b = pkg.EventBatcher(T, H2, W2, STEP, augment=pkg.EventAugment(hflip=0.5, zoom=(0.75, 1.25), drop=(0.0, 0.2), seed=3))
    kept = []
    for call, n in enumerate((900, 300, 70_000, 500)):                          # the third call grows the staging buffers
        tuples, packed, labels = _tuple_and_packed(pkg, rng, B, n, H2, W2, 1000 * (call + 1))
        X0, L0 = plain(tuples, labels)
        X1, L1 = plain(packed, labels)
        assert torch.equal(X0, X1) and torch.equal(L0, L1) and float(X1.sum()) > 0
        assert torch.equal(plain(packed), X0)                                   # without labels
        Xa, La = aug_a(tuples, labels)
        Xb, Lb = aug_b(packed, labels)
        assert torch.equal(aug_a.last_aug_table, aug_b.last_aug_table)
        assert torch.equal(Xa, Xb) and torch.equal(La, Lb) and not torch.equal(Xa, X0)
        Xi = aug_b(packed, augment=False)
        assert torch.equal(Xi, X0)                                              # the identity table
        table = aug_a.last_aug_table
        assert torch.equal(plain(packed, aug_table=table), plain(tuples, aug_table=table))
        kept.append((X1, X0))
    torch.cuda.synchronize()
    for X1, X0 in kept:                                                         # earlier batches were not disturbed by later staging
        assert torch.equal(X1, X0)
    slots = plain._slots
    assert all(s["words"] is not None and s["words"].is_pinned() and s["done"] is not None for s in slots)
    assert max(int(s["words"].shape[0]) for s in slots) >= 3 * 70_000


def test_batcher_refuses_mixed_sample_forms(pkg):
    rng = np.random.default_rng(12)
    tuples, packed, _ = _tuple_and_packed(pkg, rng, 2, 50, H, W, 1000)
    batcher = pkg.EventBatcher(T, H, W, STEP)
    with pytest.raises(ValueError, match="mixed"):
        batcher([tuples[0], packed[1]])
    with pytest.raises(ValueError, match=r"uint32 \[n, 2\]"):
        batcher([(np.zeros((4, 3), np.uint32), 0)])
    with pytest.raises(ValueError, match=r"uint32 \[n, 2\]"):
        batcher([(np.zeros((4, 2), np.int64), 0)])


# ------------------------------------------------------------------------------------------- end to end
FEED = dict(dataset="gen1", split="train", batch_size=2, num_steps=4, time_step=1, time_shift=2, events_threshold=10,
            files_in_flight=2, seed=4)


@pytest.fixture(scope="module")
def recordings(tmp_path_factory, pkg):
    """Two synthetic GEN1 recordings of 60 ms: ``(root, events per file, box rows per file)``."""
    root = tmp_path_factory.mktemp("data")
    d = root / "gen1" / "train"
    d.mkdir(parents=True)
    events, boxes = [], []
    for i in range(2):
        rng = np.random.default_rng(40 + i)
        ev = S.stream(rng, 304, 240, 60_000, per_ms=60 + 20 * i, sparse=((26, 34),) if i == 0 else ())
        ev = (ev[0], np.where(np.arange(ev[1].size) % 97 == 0, 310, ev[1]).astype(np.int32), ev[2], ev[3])   # x past the frame
        pkg.write_dat(str(d / f"r{i}_td.dat"), pkg.pack_events(*ev), 304, 240)
        b = S.walk_boxes(1000, 304, 240, steps=(10, 20, 30, 40, 50), small=(40,) if i == 0 else ())
        np.save(str(d / f"r{i}_bbox.npy"), b)
        events.append(ev)
        boxes.append(pkg.load_boxes(b, "gen1", 1000))
    return str(root), events, boxes


def test_feed_batches_equal_the_oracle_single_target(pkg, recordings):
    root, events, boxes = recordings
    feed = pkg.PropheseeFeed(root, **FEED)
    order = pkg.PropheseeFeed(root, **FEED).samples(with_file=True)              # the same seed: the same visits
    clocks = [0, 0]
    Tn, step = FEED["num_steps"], 1000
    for _ in range(3):
        X, labels = next(feed)
        want = []
        for b in range(FEED["batch_size"]):
            k, (_, t0, _) = next(order)
            while True:                                                          # the oracle's walk of file k up to its next sample
                sample, more, clocks[k], t0_ref = O.st_sample(boxes[k], *events[k], clocks[k], Tn, FEED["time_shift"], step,
                                                              240, 304, FEED["events_threshold"])
                assert more
                if sample is not None:
                    break
            assert t0_ref == t0
            want.append(sample)
        feats, labs = O.stack_batch(want)
        assert X.shape == (Tn, 2, 2, 240, 304) and np.array_equal(X.cpu().numpy(), feats)
        assert np.array_equal(labels.cpu().numpy(), labs)


def test_feed_multi_target_labels_equal_the_oracle(pkg, recordings):
    root, events, boxes = recordings
    args = dict(FEED, one_label=False)
    feed = pkg.PropheseeFeed(root, **args)
    order = pkg.PropheseeFeed(root, **args).samples(with_file=True)
    clocks = [0, 0]
    rows = 0
    for _ in range(4):
        X, labels = next(feed)
        want = []
        for b in range(2):
            k, _ = next(order)
            feats, lab, clocks[k] = O.mt_sample(boxes[k], *(v if i != 1 else np.minimum(v, 303) for i, v in enumerate(events[k])),
                                                clocks[k], FEED["num_steps"], 1000, 240, 304)
            want.append((feats, lab))
        feats, labs = O.stack_batch(want)
        assert np.array_equal(X.cpu().numpy(), feats)                            # (x past the frame is clipped: the stated difference)
        got = labels.cpu().numpy()
        if labs.shape[1]:
            assert got.shape[2] == 6 and np.array_equal(got, labs)
            rows += int((labs[:, :, 1] >= 0).sum())
        else:
            assert got.shape[1] == 0
    assert rows > 0


def test_two_training_steps_fed_by_recordings_give_finite_losses(pkg, recordings):
    from snn_for_object_detection_amd.trainer import FlatTrainer
    root, _, _ = recordings
    feed = pkg.PropheseeFeed(root, **dict(FEED, augment=pkg.EventAugment(hflip=0.5, drop=0.05, seed=1)))
    torch.manual_seed(2)
    model = pkg.TinyYolo(num_classes=2, time_window=0).cuda().train()
    trainer = FlatTrainer(model)
    losses = []
    for _ in range(2):
        batch = next(feed)
        trainer.zero_grad()
        loss = model.training_step(batch)
        loss.backward()
        trainer.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(v) for v in losses), losses
