"""The recording reader on the host (no GPU): the DAT format against hand-computed fields, the reader contract, the
samplers against the reference's own outputs (``tests/golden/events.npz``) and step by step beside ``oracle/events.py``,
``load_boxes`` against the reference's label conversion (``tests/golden/boxes.npz``), file discovery / rank split /
sample order of ``PropheseeFeed``.  Every comparison is exact."""
import os
import re

import numpy as np
import pytest

from oracle import events as O
from tests import event_aug_ref as R
from tests import recordings_ref as S

import snn_for_object_detection_amd as P
from snn_for_object_detection_amd import recordings as REC

HEADER = b"% Data file containing CD events.\n% Version 2\n% Width 304\n% Height 240\n"
# three little-endian records (ts, data), written out by hand:
#   ts 5          data 0x10008003: x = 3,     y = 2,     p = 1
#   ts 7          data 0xE0000001: x = 1,     y = 0,     p = 0, bits 29-31 set
#   ts 0xFFFFFFFF data 0x0FFFFFFF: x = 16383, y = 16383, p = 0
RECORDS = (b"\x05\x00\x00\x00\x03\x80\x00\x10" b"\x07\x00\x00\x00\x01\x00\x00\xe0" b"\xff\xff\xff\xff\xff\xff\xff\x0f")


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


# ------------------------------------------------------------------------------------------- format
def test_a_dat_file_written_by_hand_decodes_to_the_hand_computed_fields(tmp_path):
    rec = P.DatRecording(_write(tmp_path / "a_td.dat", HEADER + b"\x0c\x08" + RECORDS))
    assert (rec.width, rec.height, rec.event_size, len(rec)) == (304, 240, 8, 3)
    assert rec.words.dtype == np.uint32 and rec.words.shape == (3, 2) and isinstance(rec.words, np.memmap)
    t, x, y, p = P.unpack_events(rec.words)
    assert t.dtype == np.int64 and x.dtype == y.dtype == p.dtype == np.int32
    assert t.tolist() == [5, 7, 0xFFFFFFFF]
    assert x.tolist() == [3, 1, 16383] and y.tolist() == [2, 0, 16383] and p.tolist() == [1, 0, 0]
    assert rec.total_time() == 0xFFFFFFFF and rec.current_time == 0 and not rec.done


def test_header_without_dimensions_partial_tail_and_event_size(tmp_path):
    rec = P.DatRecording(_write(tmp_path / "b_td.dat", b"% Version 2\n% Date 2020-01-01\n\x00\x08" + RECORDS + b"\x09\x00\x00"))
    assert rec.width is None and rec.height is None and len(rec) == 3          # the 3-byte tail is ignored
    assert P.unpack_events(rec.words)[0].tolist() == [5, 7, 0xFFFFFFFF]
    none = P.DatRecording(_write(tmp_path / "c_td.dat", b"\x0c\x08"))           # no header, no events
    assert len(none) == 0 and none.done and none.total_time() == 0 and none.load_delta_t(100).shape == (0, 2)
    with pytest.raises(ValueError, match="event size 16"):
        P.DatRecording(_write(tmp_path / "d_td.dat", HEADER + b"\x0c\x10" + RECORDS))
    with pytest.raises(ValueError, match="event size"):
        P.DatRecording(_write(tmp_path / "e_td.dat", HEADER))


def test_write_dat_round_trip_and_field_ranges(tmp_path):
    rng = np.random.default_rng(1)
    n = 1000
    t = np.sort(rng.integers(0, 1 << 32, n))
    x, y, p = rng.integers(0, 1 << 14, n), rng.integers(0, 1 << 14, n), rng.integers(0, 2, n)
    words = P.pack_events(t, x, y, p)
    assert words.dtype == np.uint32 and words.shape == (n, 2)
    path = str(tmp_path / "r_td.dat")
    P.write_dat(path, words, width=1280, height=720)
    rec = P.DatRecording(path)
    assert (rec.width, rec.height, len(rec)) == (1280, 720, n)
    for got, want in zip(P.unpack_events(rec.words), (t, x, y, p)):
        assert np.array_equal(got, want)
    P.write_dat(path, words)                                                    # no dimensions in the header
    rec = P.DatRecording(path)
    assert rec.width is None and np.array_equal(np.asarray(rec.words), words)
    for bad, name in (((-1, 0, 0, 0), "t"), ((1 << 32, 0, 0, 0), "t"), ((0, 1 << 14, 0, 0), "x"),
                      ((0, 0, 1 << 14, 0), "y"), ((0, 0, 0, 2), "p"), ((0, -1, 0, 0), "x")):
        with pytest.raises(ValueError, match=f"pack_events: {name} "):
            P.pack_events(*([v] for v in bad))


# ------------------------------------------------------------------------------------------- reader contract
def test_load_delta_t_done_reset_seek(tmp_path):
    t = np.array([10, 20, 20, 30, 45, 50, 50, 50, 70, 99])
    words = P.pack_events(t, np.arange(10), np.arange(10) + 100, np.arange(10) % 2)
    path = str(tmp_path / "ten_td.dat")
    P.write_dat(path, words, 304, 240)
    rec = P.DatRecording(path)
    a = rec.load_delta_t(20)                        # [0, 20): the event AT 20 is excluded
    assert P.unpack_events(a)[0].tolist() == [10] and rec.current_time == 20 and not rec.done
    assert isinstance(a, np.memmap) and np.shares_memory(a, rec.words)           # a slice of the map, not a copy
    b = rec.load_delta_t(25)                        # [20, 45)
    assert P.unpack_events(b)[0].tolist() == [20, 20, 30] and P.unpack_events(b)[1].tolist() == [1, 2, 3]
    c = rec.load_delta_t(5)                         # [45, 50)
    assert P.unpack_events(c)[0].tolist() == [45]
    d = rec.load_delta_t(1)                         # [50, 51): the three simultaneous events
    assert P.unpack_events(d)[0].tolist() == [50, 50, 50]
    e = rec.load_delta_t(10)                        # [51, 61): empty
    assert e.shape == (0, 2) and rec.current_time == 61 and not rec.done
    f = rec.load_delta_t(38)                        # [61, 99): 99 excluded
    assert P.unpack_events(f)[0].tolist() == [70] and not rec.done
    g = rec.load_delta_t(1)
    assert P.unpack_events(g)[0].tolist() == [99] and rec.done and rec.current_time == 100
    assert rec.load_delta_t(1000).shape == (0, 2) and rec.done
    rec.reset()
    assert rec.current_time == 0 and not rec.done and rec.total_time() == 99
    assert P.unpack_events(rec.load_delta_t(21))[0].tolist() == [10, 20, 20]
    rec.seek_time(50)
    assert rec.current_time == 50 and P.unpack_events(rec.load_delta_t(50))[0].tolist() == [50, 50, 50, 70, 99]
    rec.seek_time(31)
    assert P.unpack_events(rec.load_delta_t(14))[0].tolist() == []
    assert REC.lower_bound(rec.words[:, 0], 50) == 5 and REC.lower_bound(rec.words[:, 0], 51) == 8
    assert REC.lower_bound(rec.words[:, 0], 0) == 0 and REC.lower_bound(rec.words[:, 0], 100) == 10


# ------------------------------------------------------------------------------------------- reference outputs
def _golden_recording(z, tag, tmp_path):
    t, x, y, p = (z[f"{tag}_events_{k}"] for k in "txyp")
    assert (np.diff(t) >= 0).all() and 0 <= t.min() and t.max() < 1 << 32       # sorted, inside the 32-bit field
    assert x.min() >= 0 and y.min() >= 0 and max(x.max(), y.max()) < 1 << 14 and set(np.unique(p)) <= {0, 1}
    path = str(tmp_path / f"{tag}_td.dat")
    P.write_dat(path, P.pack_events(t, x, y, p))
    return P.DatRecording(path)


def _cells(words, t0, T, H, W, step_us):
    t, x, y, p = P.unpack_events(words)
    frames = R.frames_ref([(t, x, y, p, t0)], R.identity_table(1), T, 1, H, W, step_us)
    return np.flatnonzero(frames[:, 0].reshape(-1))


@pytest.mark.parametrize("tag", ["st_gen1", "st_1mpx", "st_sparse"])
def test_st_sampler_gives_what_the_reference_parse_data_gave(tag, tmp_path, golden_dir):
    z = np.load(os.path.join(golden_dir, "events.npz"))
    T, shift, step_us, start_us, H, W, threshold = (int(v) for v in z[f"{tag}_params"])
    rec = _golden_recording(z, tag, tmp_path)
    rec.seek_time(start_us)
    sampler = P.STSampler(T, shift, step_us, threshold, float(z[f"{tag}_box_size_threshold"]))
    sample, more = sampler(z[f"{tag}_gt"], rec)
    assert more == bool(z[f"{tag}_more"]) and rec.current_time == int(z[f"{tag}_clock_after"])
    assert (sample is None) == bool(z[f"{tag}_rejected"])
    if tag == "st_sparse":
        assert sample is None and more
        return
    words, t0, labels = sample
    assert np.shares_memory(words, rec.words)
    assert labels.dtype == np.float32 and np.array_equal(labels, z[f"{tag}_labels"])
    if tag == "st_1mpx":
        assert P.unpack_events(words)[1].max() >= W                             # the clip of x is exercised
    assert np.array_equal(_cells(words, t0, T, H, W, step_us), z[f"{tag}_nonzero"])


def test_mt_sampler_gives_what_the_reference_parse_data_gave(tmp_path, golden_dir):
    z = np.load(os.path.join(golden_dir, "events.npz"))
    T, _, step_us, start_us, H, W, _ = (int(v) for v in z["mt_params"])
    rec = _golden_recording(z, "mt", tmp_path)
    rec.seek_time(start_us)
    words, t0, labels = P.MTSampler(T, step_us)(z["mt_gt"], rec)
    assert rec.current_time == int(z["mt_clock_after"]) and t0 == start_us
    assert labels.shape[1] == 6 and np.array_equal(labels, z["mt_labels"])
    assert np.array_equal(_cells(words, t0, T, H, W, step_us), z["mt_nonzero"])
    # an empty window: no events, and an EMPTY label set of the same width
    P.write_dat(str(tmp_path / "empty_td.dat"), np.zeros((0, 2), np.uint32))
    words, t0, labels = P.MTSampler(T, step_us)(z["mt_gt"], P.DatRecording(str(tmp_path / "empty_td.dat")))
    assert words.shape == (0, 2) and int(z["mt_empty_nonzero_count"]) == 0
    assert tuple(labels.shape) == tuple(int(v) for v in z["mt_empty_labels_shape"])


# ------------------------------------------------------------------------------------------- walks beside the oracle
WALK = dict(T=4, shift=2, step_us=1000, H=240, W=304, threshold=50, duration_us=60_000)


def _walk_recording(tmp_path):
    rng = np.random.default_rng(11)
    ev = S.stream(rng, WALK["W"], WALK["H"], WALK["duration_us"], per_ms=80, sparse=((26, 34),), sparse_per_ms=3)
    path = str(tmp_path / "walk_td.dat")
    P.write_dat(path, P.pack_events(*ev), WALK["W"], WALK["H"])
    gt = P.load_boxes(S.walk_boxes(WALK["step_us"], WALK["W"], WALK["H"]), "gen1", WALK["step_us"])
    return ev, gt, P.DatRecording(path)


def test_st_sampler_walks_a_recording_beside_the_oracle(tmp_path):
    ev, gt, rec = _walk_recording(tmp_path)
    T, shift, step_us, H, W, thr = (WALK[k] for k in ("T", "shift", "step_us", "H", "W", "threshold"))
    sampler = P.STSampler(T, shift, step_us, events_threshold=thr)
    clock, seen = 0, dict(accepted=0, sparse=0, small=0, end=0)
    for _ in range(20):
        want, want_more, want_clock, want_t0 = O.st_sample(gt, *ev, clock, T, shift, step_us, H, W, thr)
        assert rec.current_time == clock
        got, more = sampler(gt, rec)
        assert more == want_more and rec.current_time == want_clock and (got is None) == (want is None)
        if got is not None:
            words, t0, labels = got
            assert t0 == want_t0 and np.array_equal(labels, want[1]) and labels.shape[0] >= 2
            t, x, y, p = P.unpack_events(words)
            assert t.min() >= t0 and words.shape[0] // T >= thr
            frames = R.frames_ref([(t, x, y, p, t0)], R.identity_table(1), T, 1, H, W, step_us)[:, 0]
            assert np.array_equal(frames, want[0].astype(np.uint8))
            seen["accepted"] += 1
        elif more:
            seen["sparse"] += 1
        else:
            left = gt[gt[:, 0] >= clock // step_us + T]
            if left.size == 0:
                seen["end"] += 1
                break
            seen["small"] += 1                       # every box of the next label step is under the area threshold
            want_clock = (int(left[0, 0]) + 1) * step_us    # the file would be dropped here; the walk steps over the label
            rec.seek_time(want_clock)
        clock = want_clock
    assert seen == dict(accepted=3, sparse=1, small=1, end=1), seen
    assert P.STSampler(T, shift, step_us, events_threshold=thr)(gt, _done(rec)) == (None, False)


def _done(rec):
    rec.seek_time(1 << 33)
    assert rec.done
    return rec


def test_mt_sampler_walks_a_recording_beside_the_oracle_and_wraps(tmp_path):
    ev, gt, rec = _walk_recording(tmp_path)
    T, step_us, H, W = (WALK[k] for k in ("T", "step_us", "H", "W"))
    sampler = P.MTSampler(T, step_us)
    clock, labelled, wrapped = 0, 0, 0
    for _ in range(WALK["duration_us"] // (T * step_us) + 3):
        if rec.done:
            clock, wrapped = 0, wrapped + 1
        want_feats, want_labels, want_clock = O.mt_sample(gt, *ev, clock, T, step_us, H, W)
        words, t0, labels = sampler(gt, rec)
        assert rec.current_time == want_clock and t0 == (clock // step_us) * step_us
        assert labels.shape[1] == 6 and np.array_equal(labels, want_labels)
        t, x, y, p = P.unpack_events(words)
        frames = R.frames_ref([(t, x, y, p, t0)], R.identity_table(1), T, 1, H, W, step_us)[:, 0]
        assert np.array_equal(frames, want_feats.astype(np.uint8))
        labelled += int(labels.shape[0] > 0)
        clock = want_clock
    assert wrapped == 1 and labelled >= 5


# ------------------------------------------------------------------------------------------- boxes
@pytest.mark.parametrize("dataset", ["gen1", "1mpx"])
def test_load_boxes_equals_the_reference_label_conversion_bit_for_bit(dataset, tmp_path, golden_dir):
    z = np.load(os.path.join(golden_dir, "boxes.npz"))
    boxes, want, step_us = z[f"{dataset}_boxes"], z[f"{dataset}_labels"], int(z[f"{dataset}_time_step_us"])
    assert ("ts" if dataset == "gen1" else "t") in boxes.dtype.names and want.shape == (boxes.shape[0], 6)
    got = P.load_boxes(boxes, dataset, step_us)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    path = str(tmp_path / "x_bbox.npy")
    np.save(path, boxes)
    assert np.array_equal(P.load_boxes(path, dataset, step_us).view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError, match="dataset"):
        P.load_boxes(boxes, "gen4", step_us)


# ------------------------------------------------------------------------------------------- feed (host side)
def _dataset_dir(tmp_path, n_files, split="train"):
    d = tmp_path / "gen1" / split
    d.mkdir(parents=True)
    for i in range(n_files):
        rng = np.random.default_rng(100 + i)
        ev = S.stream(rng, 304, 240, 60_000, per_ms=20 + i)
        P.write_dat(str(d / f"rec_{i:02d}_td.dat"), P.pack_events(*ev), 304, 240)
        np.save(str(d / f"rec_{i:02d}_bbox.npy"), S.walk_boxes(1000, 304, 240, steps=(10, 20, 30, 40, 50), small=()))
    return str(tmp_path)


def _feed(root, **kw):
    args = dict(dataset="gen1", split="train", batch_size=2, num_steps=4, time_step=1, time_shift=2, events_threshold=10)
    args.update(kw)
    return P.PropheseeFeed(root, **args)


def test_feed_finds_files_and_splits_them_among_ranks(tmp_path):
    root = _dataset_dir(tmp_path, 5)
    feed = _feed(root)
    names = [os.path.basename(g) for g, _ in feed.files]
    assert names == [f"rec_{i:02d}_bbox.npy" for i in range(5)]
    assert all(d == g.replace("_bbox.npy", "_td.dat") and os.path.exists(d) for g, d in feed.files)
    assert feed.get_labels() == ["car", "person"] and len(_feed(root, dataset="gen1").get_labels()) == 2
    parts = [_feed(root, rank=r, world=2).files for r in range(2)]
    assert [len(p) for p in parts] == [2, 2] and not set(parts[0]) & set(parts[1])
    assert parts[0] + parts[1] == feed.files[:4]                                 # per * world files, in order
    os.remove(feed.files[3][1])
    with pytest.raises(RuntimeError, match="does not contain data or data is invalid"):
        _feed(root)
    with pytest.raises(RuntimeError, match="does not contain data or data is invalid"):
        _feed(root, split="val")
    with pytest.raises(ValueError, match="dataset"):
        _feed(root, dataset="gen4")
    assert P.PropheseeFeed.__init__.__defaults__[:8] == ("gen1", "train", 4, 42, 16, 16, True, 8)


def test_feed_sample_order_is_a_function_of_its_seed_alone(tmp_path):
    import random
    root = _dataset_dir(tmp_path, 5)

    def order(seed, n=24, **kw):
        it = _feed(root, seed=seed, files_in_flight=4, **kw).samples(with_file=True)
        out = []
        for _ in range(n):
            k, (words, t0, labels) = next(it)
            out.append((k, int(t0), int(words.shape[0]), int(labels.shape[0])))
        return out

    random.seed(5)
    a = order(0)
    random.seed(6)                                                               # the global generator plays no part
    assert order(0) == a and order(1) != a
    assert len({k for k, *_ in a}) >= 4 and all(n // 4 >= 10 and rows >= 2 for _, _, n, rows in a)
    # five accepted samples per file (labels at steps 10 .. 50), a file leaves the round when its labels run out
    firsts = [k for k, *_ in a[:4]]
    assert sorted(firsts) == sorted(set(firsts))                                 # the first round visits each open file once
    mt = order(0, n=8, one_label=False)
    assert mt == order(0, n=8, one_label=False) and all(t0 % 4000 == 0 for _, t0, _, _ in mt)


def test_the_symbol_is_declared_and_abi_stays_20():
    from snn_for_object_detection_amd import _hip
    header = open(os.path.join(os.path.dirname(_hip._HERE), "include", "snn_hip.h")).read()
    assert re.search(r"#define\s+SNN_ABI_VERSION\s+20\b", header) and _hip.ABI_VERSION == 20
    assert re.search(r"\bint\s+snn_events_to_frames_packed\s*\(", header)
    assert len(_hip.SIGNATURES["snn_events_to_frames_packed"][1]) == 12
    for name in ("DatRecording", "PropheseeFeed", "STSampler", "MTSampler", "load_boxes", "pack_events", "unpack_events",
                 "write_dat"):
        assert hasattr(P, name), name
