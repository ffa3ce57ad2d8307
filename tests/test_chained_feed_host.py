"""``PropheseeFeed(chained=True)`` on the host (no GPU): every batch slot is bound to one recording and walks its windows
in time order, ``first`` marks the first window of a recording in its slot, the slot's augmentation row lives as long as
the recording does.  Five tiny recordings of unequal length (one shorter than a window), ``B = 3``, windows of 4 steps of
1 ms.  Every comparison is exact.  Also the refusals by name: ``one_label=True``, and ``SODa(carry_state=True)`` with a
random prefix."""
import numpy as np
import pytest
import torch

from tests import recordings_ref as S

import snn_for_object_detection_amd as P

B, T, STEP_US = 3, 4, 1000
WINDOW_US = T * STEP_US
DURATIONS_MS = (10, 17, 3, 9, 12)                       # 3, 5, 1 (shorter than a window), 3, 3 windows
LABEL_STEPS = ((1, 5, 6), (0, 3, 4, 11, 16), (2,), (7, 8), (1, 2, 3, 10, 11))


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    top = tmp_path_factory.mktemp("chained")
    d = top / "gen1" / "train"
    d.mkdir(parents=True)
    for i, (ms, steps) in enumerate(zip(DURATIONS_MS, LABEL_STEPS)):
        ev = S.stream(np.random.default_rng(200 + i), 304, 240, ms * 1000, per_ms=6 + i)
        P.write_dat(str(d / f"rec_{i:02d}_td.dat"), P.pack_events(*ev), 304, 240)
        np.save(str(d / f"rec_{i:02d}_bbox.npy"), S.walk_boxes(STEP_US, 304, 240, steps=steps, small=()))
    return str(top)


def _feed(root, **kw):
    args = dict(dataset="gen1", split="train", batch_size=B, num_steps=T, time_step=1, one_label=False, chained=True,
                seed=5)
    args.update(kw)
    return P.PropheseeFeed(root, **args)


def _files(feed):
    """Per file: its events' timestamps, its label rows (absolute steps) and its number of windows, worked out here."""
    out = []
    for gt_path, dat_path in feed.files:
        ts = P.unpack_events(P.DatRecording(dat_path).words)[0]
        out.append((ts, P.load_boxes(gt_path, "gen1", STEP_US), int(ts[-1]) // WINDOW_US + 1))
    return out


def _run(feed, n_batches):
    """``n_batches`` batches of ``samples(with_file=True)`` as rows ``(batch, slot, file, sample)``."""
    it = feed.samples(with_file=True)
    return [(n, b, *next(it)) for n in range(n_batches) for b in range(B)]


def test_slots_walk_their_recording_in_time_order_and_first_marks_every_file_change(root):
    feed = _feed(root)
    files = _files(feed)
    assert [f[2] for f in files] == [3, 5, 1, 3, 3]
    per_cycle = sum(f[2] for f in files)
    rows = _run(feed, 2 * per_cycle)                    # 6 * per_cycle windows: every file is gone through several times
    held = [None] * B                                   # per slot: (file, index of the window it showed last)
    opens, visits = [], {i: [] for i in range(len(files))}
    for n, b, i, (words, t0, labels, first, aug_row) in rows:
        ts, gt, n_win = files[i]
        fresh = held[b] is None or held[b][1] == files[held[b][0]][2] - 1
        assert first == (1 if fresh else 0), (n, b)
        if n == 0:
            assert first == 1
        if fresh:
            w = 0
            opens.append(i)
        else:
            assert i == held[b][0]                      # the slot stays with its recording until it is done
            w = held[b][1] + 1
        assert t0 == w * WINDOW_US                      # consecutive windows of one file abut; a new file starts at 0
        held[b] = (i, w)
        visits[i].append(w)
        # the events of exactly [t0, t0 + window), as a slice of the recording
        got = P.unpack_events(words)[0]
        assert np.array_equal(got, ts[(ts >= t0) & (ts < t0 + WINDOW_US)])
        # the label rows of the window's steps, their step made window-relative
        s0 = t0 // STEP_US
        want = gt[(gt[:, 0] >= s0) & (gt[:, 0] < s0 + T)].copy()
        want[:, 0] -= s0
        assert labels.shape[1] == 6 and np.array_equal(labels, want)
        assert ((labels[:, 0] >= 0) & (labels[:, 0] < T)).all()
        assert aug_row is None
    # the files are opened in one shuffled order, over and over: every window of every file once per cycle
    n_files = len(files)
    assert sorted(opens[:n_files]) == list(range(n_files))
    assert all(i == opens[k % n_files] for k, i in enumerate(opens))
    for i, seen in visits.items():
        n_win = files[i][2]
        assert len(seen) >= 2 * n_win
        assert seen == [k % n_win for k in range(len(seen))]
    passes = [len(v) // files[i][2] for i, v in visits.items()]
    assert max(passes) - min(passes) <= 1
    # every label row of a file is shown once per pass (none lies behind the last window here)
    assert all(int(f[1][:, 0].max()) < f[2] * T for f in files)


def test_two_feeds_with_one_seed_agree_and_the_order_follows_the_seed(root):
    a, b, c = _run(_feed(root), 8), _run(_feed(root), 8), _run(_feed(root, seed=6), 8)
    assert [(r[2], r[3][1], r[3][3]) for r in a] == [(r[2], r[3][1], r[3][3]) for r in b]
    assert [r[2] for r in a] != [r[2] for r in c]


def test_the_augmentation_row_lives_as_long_as_the_recording_in_its_slot(root):
    kw = dict(hflip=0.5, zoom=(0.75, 1.25), drop=(0.0, 0.1), seed=3)
    rows = _run(_feed(root, augment=P.EventAugment(**kw)), 14)
    stub = P.EventAugment(**kw)                         # the same generator: the rows in the order the slots open files
    held = [None] * B
    marks = 0
    for n, b, i, (words, t0, labels, first, aug_row) in rows:
        assert aug_row.dtype == torch.int32 and tuple(aug_row.shape) == (8,)
        if first:
            want = stub.draw(1, 304, 240)[0]
            assert torch.equal(aug_row, want)           # redrawn at a mark ...
            held[b] = want
            marks += 1
        else:
            assert torch.equal(aug_row, held[b])        # ... and constant until the next one
    assert marks > B                                    # (files changed during the run)
    assert len({tuple(r.tolist()) for r in held}) == B  # different slots, different transforms


def test_chained_needs_six_column_labels_and_carry_state_no_random_prefix(root):
    with pytest.raises(ValueError, match="chained=True needs one_label=False"):
        _feed(root, one_label=True)
    with pytest.raises(ValueError, match="carry_state=True needs time_window=0"):
        P.TinyYolo(num_classes=2, carry_state=True, time_window=3)
    model = P.TinyYolo(num_classes=2, carry_state=True, time_window=0, label_steps=2)
    assert model.hparams.carry_state is True and model._carried == {}
    assert P.TinyYolo(num_classes=2).hparams.carry_state is False
    with pytest.raises(ValueError, match="stage must be"):
        model.reset_carried_state("fit")
    model.reset_carried_state()
    model.reset_carried_state("val")
