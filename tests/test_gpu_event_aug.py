"""The augmented event feed on the GPU: ``snn_events_to_frames_aug`` bit for bit against the integer reference of
``tests/event_aug_ref.py``, ``snn_labels_augment`` against its float64 reference, and both through ``EventBatcher``."""
import os

import numpy as np
import pytest
import torch

from tests import event_aug_ref as R

pytestmark = pytest.mark.gpu

T, H, W, STEP = 3, 5, 7, 1000


@pytest.fixture(scope="module")
def pkg(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import snn_for_object_detection_amd as p
    return p


def _table(B, flip=0, a=65536, ox=0, oy=0, drop=0, seeds=None):
    t = R.identity_table(B)
    t[:, 0], t[:, 1], t[:, 2], t[:, 3] = flip, a, ox, oy
    t[:, 4] = np.array([drop], dtype=np.uint32).view(np.int32)[0]
    if seeds is not None:
        t[:, 5] = np.array(seeds, dtype=np.uint32).view(np.int32)
    return t


def _frames(pkg, samples, table, T, H, W, step):
    """The kernel on a batch given as numpy samples -> uint8 [T, B, 2, H, W] on the host (and the fp32 device tensor)."""
    from snn_for_object_detection_amd import functional as HF
    B = len(samples)
    cat = [np.concatenate([np.asarray(s[k]) for s in samples]) for k in range(4)]
    dev = [torch.from_numpy(cat[0].astype(np.int64)).cuda()] + [torch.from_numpy(v.astype(np.int32)).cuda() for v in cat[1:]]
    offsets = torch.tensor(np.cumsum([0] + [len(s[0]) for s in samples]), dtype=torch.int64).cuda()
    t0 = torch.tensor([int(s[4]) for s in samples], dtype=torch.int64).cuda()
    aug = HF.check_aug_table(torch.from_numpy(table), B).cuda()
    X = HF.events_to_frames_aug(*dev, offsets, t0, aug, T, H, W, step)
    assert X.shape == (T, B, 2, H, W) and HF.is_channels_last(X)
    vals = torch.unique(X)
    assert all(float(v) in (0.0, 1.0) for v in vals)            # flags, not counts; the buffer was zero-filled
    return X.cpu().numpy().astype(np.uint8), X


def _all_rules_batch():
    """B = 3: ~200 events with every skip / clip rule in them, an empty sample, 50 events."""
    rng = np.random.default_rng(3)
    t0 = 5000
    n = 190
    t = rng.integers(t0 - 300, t0 + T * STEP + 300, n)
    x = rng.integers(0, W, n)
    y = rng.integers(0, H, n)
    p = rng.integers(0, 2, n)
    edge = [  # (t, x, y, p)
        (t0 - 1, 1, 1, 0), (t0, 2, 1, 1), (t0 + T * STEP - 1, 3, 2, 0), (t0 + T * STEP, 4, 2, 1),
        (t0 + 10, -2, 3, 0), (t0 + 1010, W + 3, 3, 1), (t0 + 20, 3, -1, 0), (t0 + 30, 3, H, 1), (t0 + 40, 5, 4, 2),
        (t0 - STEP, 6, 0, 1)]
    e = np.array(edge, dtype=np.int64)
    s0 = (np.concatenate([t, e[:, 0]]), np.concatenate([x, e[:, 1]]), np.concatenate([y, e[:, 2]]),
          np.concatenate([p, e[:, 3]]), t0)
    empty = tuple(np.zeros(0, dtype=np.int64) for _ in range(4)) + (123,)
    t2 = 90_000
    s2 = (rng.integers(t2, t2 + T * STEP, 50), rng.integers(-1, W + 1, 50), rng.integers(0, H, 50),
          rng.integers(0, 2, 50), t2)
    return [s0, empty, s2]


ALL_RULES = {
    "identity": dict(),
    "flip": dict(flip=1),
    "zoom_out": dict(a=32768, ox=3, oy=2),
    "zoom_in": dict(a=98304, ox=-2, oy=-1),
    "odd_flip": dict(flip=1, a=40000, ox=-1, oy=1),
    "drop_a": dict(drop=1 << 31, seeds=[1, 2, 3]),
    "drop_b": dict(drop=1 << 31, seeds=[0xDEADBEEF, 12345, 0xFFFFFFFF]),
}


# ------------------------------------------------------------------------------------------- 1. every rule at once
@pytest.mark.parametrize("case", list(ALL_RULES))
def test_every_rule_against_the_integer_reference(pkg, case):
    samples = _all_rules_batch()
    table = _table(3, **ALL_RULES[case])
    got, _ = _frames(pkg, samples, table, T, H, W, STEP)
    want = R.frames_ref(samples, table, T, 3, H, W, STEP)
    assert want.sum() > 0 and want[:, 1].sum() == 0             # the empty sample stays empty
    assert np.array_equal(got, want), case
    plain = R.frames_ref(samples, _table(3), T, 3, H, W, STEP)
    if case != "identity":
        assert not np.array_equal(want, plain)                  # the transform is visible in the expected frames
    if case.startswith("drop"):
        assert 0 < got.sum() < plain.sum()                      # some events dropped, some kept
        for b in (0, 2):
            u = R.drop_hash(np.arange(len(samples[b][0]), dtype=np.int64), int(table[b, 5]))
            assert (u < np.uint64(1 << 31)).any() and (u >= np.uint64(1 << 31)).any()


def test_the_two_drop_seeds_differ(pkg):
    samples = _all_rules_batch()
    a, _ = _frames(pkg, samples, _table(3, **ALL_RULES["drop_a"]), T, H, W, STEP)
    b, _ = _frames(pkg, samples, _table(3, **ALL_RULES["drop_b"]), T, H, W, STEP)
    assert not np.array_equal(a, b)


# ------------------------------------------------------------------------------------------- 2. identity = old path
def test_identity_table_equals_the_plain_batcher_on_the_reference_fixture(pkg, golden_dir):
    z = np.load(os.path.join(golden_dir, "events.npz"))
    for tag in ("st_gen1", "st_1mpx", "mt"):
        T_, shift, step_us, clock, H_, W_, _ = (int(v) for v in z[f"{tag}_params"])
        ev = tuple(torch.from_numpy(z[f"{tag}_events_{k}"].astype(np.int64)).pin_memory() for k in "txyp")
        if tag == "mt":
            t0 = (clock // step_us) * step_us
        else:
            gt = z[f"{tag}_gt"]
            first = gt[gt[:, 0] >= clock // step_us + T_][0, 0]
            t0 = int(first) * step_us - step_us * (T_ - shift)
        labels = [torch.from_numpy(z[f"{tag}_labels"])]
        X0, lab0 = pkg.EventBatcher(T_, H_, W_, step_us)([ev + (t0,)], labels)
        new = pkg.EventBatcher(T_, H_, W_, step_us, augment=pkg.EventAugment(hflip=1.0, zoom=(0.5, 2.0), drop=0.5))
        X1, lab1 = new([ev + (t0,)], labels, augment=False)
        assert X1.shape == X0.shape and X1.stride() == X0.stride()
        assert torch.equal(X1, X0), tag
        assert torch.equal(lab1, lab0), tag
        assert torch.equal(new.last_aug_table, pkg.EventAugment.identity(1))
        got = np.flatnonzero(X1[:, 0].contiguous().cpu().numpy().reshape(-1))
        assert np.array_equal(got, z[f"{tag}_nonzero"]), tag
        X2 = new([ev + (t0,)])                                   # and the drawn transform does change the batch
        assert not torch.equal(X2, X0)


# ------------------------------------------------------------------------------------------- 3. metamorphic: flips
def _api_batch(B, T_, H_, W_, step, n=1500, seed=9):
    rng = np.random.default_rng(seed)
    samples, labels = [], []
    for b in range(B):
        t0 = 4000 * (b + 1)
        ev = (rng.integers(t0 - 200, t0 + T_ * step + 200, n), rng.integers(0, W_ + 2, n), rng.integers(0, H_, n),
              rng.integers(0, 2, n))
        samples.append(tuple(torch.from_numpy(v) for v in ev) + (t0,))
        labels.append(torch.tensor([[0, 0.2, 0.2, 0.5, 0.6], [1, 0.5, 0.4, 0.9, 0.8], [1, 0.0, 0.1, 0.3, 1.0]][:b + 1]))
    return samples, labels


def test_pure_flip_mirrors_frames_and_boxes(pkg):
    B, T_, H_, W_ = 3, 4, 12, 20
    samples, labels = _api_batch(B, T_, H_, W_, STEP)
    X0, lab0 = pkg.EventBatcher(T_, H_, W_, STEP)(samples, labels)
    table = pkg.EventAugment.identity(B)
    table[:, 0] = 1
    batcher = pkg.EventBatcher(T_, H_, W_, STEP)                 # no EventAugment: the explicit table alone
    X1, lab1 = batcher(samples, labels, aug_table=table)
    assert torch.equal(X1, torch.flip(X0, dims=[-1]))
    assert float(X0.sum()) > 0 and not torch.equal(X1, X0)
    assert torch.equal(batcher.last_aug_table, table)
    lab0, lab1 = lab0.cpu(), lab1.cpu()
    valid = lab0[:, :, 0] >= 0
    assert torch.equal(lab1[:, :, 0], lab0[:, :, 0]) and int(valid.sum()) == 6
    assert torch.equal(lab1[:, :, 1][valid], (1.0 - lab0[:, :, 3])[valid])
    assert torch.equal(lab1[:, :, 3][valid], (1.0 - lab0[:, :, 1])[valid])
    assert torch.equal(lab1[:, :, [2, 4]], lab0[:, :, [2, 4]])
    assert torch.equal(lab1[~valid], lab0[~valid])
    # one flipped sample in a batch leaves the others alone
    table[1:, 0] = 0
    X2 = batcher(samples, aug_table=table)
    assert torch.equal(X2[:, 0], torch.flip(X0[:, 0], dims=[-1])) and torch.equal(X2[:, 1:], X0[:, 1:])


# ------------------------------------------------------------------------------------------- 4. lookup, grid stride
def test_sample_lookup_over_many_short_samples(pkg):
    """B = 70 (the offsets are searched in global memory, past the LDS staging), 0 to 9 events each, the first and the
    last sample empty, a different table per sample."""
    B, H_, W_ = 70, 2, 33
    rng = np.random.default_rng(17)
    counts = rng.integers(0, 10, B)
    counts[[0, 5, 6, B - 1]] = 0
    samples = []
    for b in range(B):
        n, t0 = int(counts[b]), 1000 * b - 7000                  # negative window starts as well
        samples.append((rng.integers(t0 - 100, t0 + T * STEP + 100, n), rng.integers(-1, W_ + 1, n),
                        rng.integers(0, H_, n), rng.integers(0, 2, n), t0))
    table = R.identity_table(B)
    table[:, 0] = rng.integers(0, 2, B)
    table[:, 1] = rng.integers(40000, 100000, B)
    table[:, 2] = rng.integers(-6, 7, B)
    table[:, 3] = rng.integers(-1, 2, B)
    table[::3, 4] = np.array([1 << 30], dtype=np.uint32).view(np.int32)[0]
    table[:, 5] = rng.integers(0, 1 << 32, B, dtype=np.uint64).astype(np.uint32).view(np.int32)
    got, _ = _frames(pkg, samples, table, T, H_, W_, STEP)
    want = R.frames_ref(samples, table, T, B, H_, W_, STEP)
    assert want.sum() > 50
    assert np.array_equal(got, want)
    # the same batch in 64 samples or fewer takes the LDS-staged path: sample by sample it must agree
    for lo in (0, 35):
        part, _ = _frames(pkg, samples[lo:lo + 35], table[lo:lo + 35], T, H_, W_, STEP)
        assert np.array_equal(part, want[:, lo:lo + 35])


def test_grid_stride_loop_reaches_the_tail(pkg):
    """One sample of 256 * (the launcher's block cap: 8 per compute unit) + 5 events: the last five run in the second
    trip of the loop.  All but a few events lie before the window, so the expected frames stay sparse."""
    H_, W_ = 2, 33
    cap = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    n = 256 * cap + 5
    rng = np.random.default_rng(23)
    t0 = 10_000
    t = np.full(n, t0 - 1, dtype=np.int64)
    live = np.concatenate([rng.choice(n - 5, 40, replace=False), np.arange(n - 5, n)])
    t[live] = t0 + rng.integers(0, T * STEP, live.size)
    x = rng.integers(0, W_, n)
    x[n - 5:] = [0, 8, 16, 24, 32]
    samples = [(t, x, rng.integers(0, H_, n), rng.integers(0, 2, n), t0)]
    for table in (_table(1), _table(1, flip=1, a=50000, ox=4, drop=1 << 30, seeds=[77])):
        got, _ = _frames(pkg, samples, table, T, H_, W_, STEP)
        want = R.frames_ref(samples, table, T, 1, H_, W_, STEP)
        assert 5 <= want.sum() <= 45
        assert np.array_equal(got, want)
    tail_only = [tuple(v[n - 5:] for v in samples[0][:4]) + (t0,)]
    assert R.frames_ref(tail_only, _table(1), T, 1, H_, W_, STEP).sum() == 5   # the tail is visible in the identity case


def test_windows_longer_than_2_to_the_32_take_the_wide_division(pkg):
    """``T * step`` past 2^32 microseconds: ``t - t0`` no longer fits the 32-bit division, the tuple source takes the
    64-bit one.  The first and the last microsecond of the window are among the events of both samples."""
    B, H_, W_, n = 2, 2, 33, 200
    step = (1 << 32) // T + 1
    assert T * step > 1 << 32
    rng = np.random.default_rng(31)
    samples = []
    for t0 in (7000, -(1 << 33)):
        t = rng.integers(t0, t0 + T * step, n)
        t[0], t[-1] = t0, t0 + T * step - 1
        x, y = rng.integers(-1, W_ + 1, n), rng.integers(0, H_, n)
        x[[0, -1]], y[[0, -1]] = 16, 0                           # (stays inside the frame under the second row)
        samples.append((t, x, y, rng.integers(0, 2, n), t0))
    table = _table(B, seeds=[5, 6])
    table[1, :5] = [1, 50000, 4, 0, 1 << 30]                     # flip + zoom + drop beside the identity row
    want = R.frames_ref(samples, table, T, B, H_, W_, step)
    for b in range(B):
        assert want[0, b].sum() > 0 and want[T - 1, b].sum() > 0, b   # both ends of the window hold events
        ends = [tuple(v[[0, -1]] for v in samples[b][:4]) + (samples[b][4],)]
        no_drop = table[b:b + 1].copy()
        no_drop[0, 4] = 0
        assert R.frames_ref(ends, no_drop, T, 1, H_, W_, step).sum(axis=(1, 2, 3, 4)).tolist() == [1, 0, 1]
        assert (R.drop_hash(np.array([0, n - 1], dtype=np.int64), int(table[b, 5])) >= np.uint64(int(table[b, 4]))).all()
    got, _ = _frames(pkg, samples, table, T, H_, W_, step)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------- 5. labels
LW, LH, MIN_VISIBLE, MIN_SIZE = 64, 48, 0.25, 2.0
MARGIN = 1e-3

HAND_BOXES = [  # x1, y1, x2, y2
    (0.30, 0.30, 0.60, 0.70),        # wholly inside
    (-0.10, 0.30, 0.30, 0.60),       # cut by the left border, 3/4 visible
    (0.70, 0.20, 1.10, 0.50),        # right border, 3/4 visible
    (0.20, -0.10, 0.50, 0.30),       # top border
    (0.20, 0.80, 0.50, 1.20),        # bottom border, half visible
    (-0.50, 0.30, 0.05, 0.60),       # left border, 1/11 visible: dropped at identity
    (1.20, 0.20, 1.50, 0.50),        # wholly outside
    (0.50, 0.50, 0.50 + 1.0 / 64, 0.50 + 1.0 / 48),   # one pixel: under min_size_px
    (0.10, 0.10, 0.20, 0.25),        # 6.4 x 7.2 px: under min_size_px only after the zoom-out by 4
    (0.00, 0.00, 1.00, 1.00),        # exactly the whole frame
]

LABEL_TABLES = np.array([            # flip, a_q16, ox, oy
    [0, 65536, 0, 0], [1, 65536, 0, 0], [0, 16384, 20, 11], [1, 98304, -17, -9], [0, 49152, 5, 3], [1, 81920, -9, 2]])


def _robust(margins, by):
    """A row's decision stands clear of rounding: kept with every compared quantity at least ``by`` above its threshold,
    or dropped by a quantity at least ``by`` below it."""
    return (margins >= by).all(axis=-1) | (margins <= -by).any(axis=-1)


def _label_case(width, N):
    """fp32 labels [B, N, width] whose every keep / drop decision has a margin of at least MARGIN (float64)."""
    B = len(LABEL_TABLES)
    table = R.identity_table(B)
    table[:, :4] = LABEL_TABLES
    rng = np.random.default_rng(100 * width + N)
    lab = np.full((B, N, width), -1.0, dtype=np.float32)
    # N = 70: hand-built boxes 0..2 in rows 0..2, padding in rows 3 and 4, hand-built boxes 3..9 in rows 5..11, random
    # boxes behind them with more padding rows in the middle and at the end
    pad = set() if N < 10 else {3, 4, 20, 41, N - 1}
    hand = {} if N < 10 else {**{i: i for i in range(3)}, **{i: i - 2 for i in range(5, 12)}}
    for b in range(B):
        for i in range(N):
            if i in pad:
                continue
            while True:
                if i in hand:
                    box = HAND_BOXES[hand[i]]
                else:
                    c = rng.uniform(-0.2, 1.2, 2)
                    half = rng.uniform(0.01, 0.35, 2)
                    box = (c[0] - half[0], c[1] - half[1], c[0] + half[0], c[1] + half[1])
                row = np.full((1, 1, width), 0.0, dtype=np.float32)
                row[0, 0, width - 5] = float(rng.integers(0, 3))
                row[0, 0, width - 4:] = box
                if width == 6:
                    row[0, 0, 0] = float(rng.integers(0, 8))
                _, _, _, m = R.label_decisions(row, table[b:b + 1], LW, LH, MIN_VISIBLE, MIN_SIZE)
                if _robust(m, 2 * MARGIN).all():
                    break
                assert i not in hand, ("a hand-built box sits on a threshold", b, i, m)
            lab[b, i] = row[0, 0]
    return lab, table


@pytest.mark.parametrize("width", [5, 6])
@pytest.mark.parametrize("N", [0, 1, 70])
def test_labels_against_float64(pkg, width, N):
    from snn_for_object_detection_amd import functional as HF
    lab, table = _label_case(width, N)
    B = lab.shape[0]
    aug = torch.from_numpy(table).cuda()
    got = HF.labels_augment(torch.from_numpy(lab).cuda(), aug, LW, LH, MIN_VISIBLE, MIN_SIZE).cpu().numpy()
    assert got.shape == (B, N, width) and got.dtype == np.float32
    if N == 0:
        return
    valid, keep, _, margins = R.label_decisions(lab, table, LW, LH, MIN_VISIBLE, MIN_SIZE)
    assert _robust(margins[valid], MARGIN).all()                 # no decision rests on rounding
    want = R.labels_ref(lab, table, LW, LH, MIN_VISIBLE, MIN_SIZE)
    assert np.array_equal(got == -1.0, want == -1.0)             # the positions of the -1 rows (and no -1 elsewhere)
    assert np.array_equal(got[:, :, :width - 4].astype(np.float64), want[:, :, :width - 4])   # ts, class, row order
    assert np.abs(got[:, :, width - 4:] - want[:, :, width - 4:]).max() <= 1e-6
    if N == 70:
        for b in range(B):
            k = int(keep[b].sum())
            assert 0 < k < int(valid[b].sum()) < N, b             # kept, dropped and padding rows in every sample
            assert (got[b, :k, width - 5] >= 0).all() and (got[b, k:] == -1.0).all()
        # identity sample: the hand-built boxes decide as their comments say
        assert list(keep[0, :3]) == [True, True, True] and list(keep[0, 5:10]) == [True, True, False, False, False]
        assert bool(keep[0, 10]) and bool(keep[0, 11])            # 6.4 x 7.2 px box and the whole frame at identity
        assert not keep[2, 10]                                    # the small box after the zoom-out by 4
        assert np.allclose(got[0, :3, width - 4:], [[0.3, 0.3, 0.6, 0.7], [0.0, 0.3, 0.3, 0.6], [0.7, 0.2, 1.0, 0.5]],
                           rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------- 6. one training step
def test_one_training_step_from_an_augmenting_batcher(pkg):
    from snn_for_object_detection_amd.trainer import FlatTrainer
    B, T_, H_, W_ = 2, 2, 32, 48
    samples, labels = _api_batch(B, T_, H_, W_, STEP, n=2500)
    kw = dict(hflip=0.5, zoom=(0.75, 1.25), drop=(0.0, 0.1))
    first = pkg.EventBatcher(T_, H_, W_, STEP, augment=pkg.EventAugment(seed=5, **kw))
    again = pkg.EventBatcher(T_, H_, W_, STEP, augment=pkg.EventAugment(seed=5, **kw))
    X, lab = first(samples, labels)
    X2, lab2 = again(samples, labels)
    assert first.last_aug_table.shape == (2, 8) and first.last_aug_table.dtype == torch.int32
    assert torch.equal(first.last_aug_table, again.last_aug_table)
    assert torch.equal(X, X2) and torch.equal(lab, lab2)
    assert X.shape == (T_, B, 2, H_, W_) and lab.shape == (B, 2, 5) and float(X.sum()) > 0
    assert int((lab[:, :, 0] >= 0).sum()) >= 1
    X3, _ = first(samples, labels)                               # the next draw is another transform
    assert not torch.equal(first.last_aug_table, again.last_aug_table) and not torch.equal(X3, X)
    torch.manual_seed(2)
    model = pkg.TinyYolo(num_classes=2, time_window=0).cuda().train()
    trainer = FlatTrainer(model)
    trainer.zero_grad()
    loss = model.training_step((X, lab))
    loss.backward()
    trainer.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


# ------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_by_name(pkg, hip_lib):
    from snn_for_object_detection_amd import _hip
    from snn_for_object_detection_amd import functional as HF
    samples, labels = _api_batch(2, T, H, W, STEP, n=20)
    batcher = pkg.EventBatcher(T, H, W, STEP)
    good = pkg.EventAugment.identity(2)
    for a in ((1 << 14) - 1, (1 << 18) + 1):
        bad = good.clone()
        bad[1, 1] = a
        with pytest.raises(ValueError, match="a_q16"):
            batcher(samples, labels, aug_table=bad)
    with pytest.raises(ValueError, match="shape"):
        batcher(samples, aug_table=pkg.EventAugment.identity(3))
    with pytest.raises(ValueError, match="shape"):
        batcher(samples, aug_table=good[:, :4].contiguous())
    with pytest.raises(ValueError, match="int32"):
        batcher(samples, aug_table=good.long())
    with pytest.raises(ValueError, match="host"):
        batcher(samples, aug_table=good.cuda())
    with pytest.raises(ValueError, match="time_step_us"):
        pkg.EventBatcher(T, H, W, 0)(samples, aug_table=good)
    assert batcher.last_aug_table is None                        # nothing ran
    i64 = torch.zeros(8, dtype=torch.int64, device="cuda")
    i32 = torch.zeros(16, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="step_us"):
        HF.events_to_frames_aug(i64[:4], i32[:4], i32[:4], i32[:4], i64[:3], i64[:2], i32, T, H, W, 0)
    buf = torch.zeros(T * 2 * H * W * 2, device="cuda")
    args = [i64.data_ptr(), i32.data_ptr(), i32.data_ptr(), i32.data_ptr(), i64.data_ptr(), i64.data_ptr(),
            i32.data_ptr(), 4, buf.data_ptr(), T, 2, H, W, STEP, 0]

    def refused(match, **change):
        a = list(args)
        for k, v in change.items():
            a[int(k[1:])] = v
        with pytest.raises(RuntimeError, match=match):
            _hip.call("snn_events_to_frames_aug", *a)

    refused("step_us", _13=0)
    refused("step_us", _13=-5)
    refused("null", _8=None)
    refused("null", _4=None)
    refused("null", _6=None)
    refused("null event", _0=None)
    refused("2\\^31 elements", _9=1 << 14, _10=1 << 14, _11=2, _12=2)     # 2 T B H W = 2^31
    refused("2\\^31 elements", _9=8, _10=8, _11=1 << 12, _12=1 << 12)
    with pytest.raises(RuntimeError, match="5 or 6"):
        _hip.call("snn_labels_augment", buf.data_ptr(), buf.data_ptr() + 1024, i32.data_ptr(), 2, 3, 4, W, H, 0.25, 2.0, 0)
    with pytest.raises(RuntimeError, match="in place"):
        _hip.call("snn_labels_augment", buf.data_ptr(), buf.data_ptr(), i32.data_ptr(), 2, 3, 5, W, H, 0.25, 2.0, 0)
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0                         # every refusal came before any launch
