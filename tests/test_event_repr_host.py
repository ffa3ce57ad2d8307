"""Event representations on the host (no GPU): properties of the integer reference ``tests/event_repr_ref.py``, the
header / binding / ABI, ``snn_events_rep_supported`` over its table of legal and illegal arguments, and every Python
refusal of ``EventRepresentation``, ``EventBatcher``, ``PropheseeFeed`` and the two ``event_ops`` functions by name, on
CPU tensors, before a device is needed."""
import os
import re

import numpy as np
import pytest
import torch

from tests import event_aug_ref as R
from tests import event_repr_ref as E

T, B, H, W = 4, 3, 6, 10


def _batch(step, seed=5, n=300):
    rng = np.random.default_rng(seed)
    samples = []
    for b in range(B):
        t0 = 7000 * b - 3000
        samples.append((rng.integers(t0 - step, t0 + (T + 1) * step, n), rng.integers(-2, W + 2, n),
                        rng.integers(-1, H + 1, n), rng.integers(-1, 3, n), t0))
    table = R.identity_table(B)
    table[1, :4] = [1, 50000, 2, 1]
    table[2, 4] = np.array([1 << 30], dtype=np.uint32).view(np.int32)[0]
    table[2, 5] = 77
    return samples, table


# ------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("step", [1000, 16667])
def test_reference_properties(step):
    samples, table = _batch(step)
    binary = E.frames_rep_ref(samples, table, T, B, H, W, step, E.BINARY)
    want = R.frames_ref(samples, table, T, B, H, W, step)
    assert want.sum() > 100 and np.array_equal(binary, want.astype(np.float32))
    count = E.frames_rep_ref(samples, table, T, B, H, W, step, E.COUNT)
    time = E.frames_rep_ref(samples, table, T, B, H, W, step, E.TIME)
    assert np.array_equal(count > 0, binary == 1) and np.array_equal(time > 0, binary == 1)
    assert count.max() >= 3 and float(count.sum()) > want.sum()              # cells with several events
    assert time.max() <= 1.0 and time[time > 0].min() >= np.float32(1.0) / np.float32(step)
    clipped = E.frames_rep_ref(samples, table, T, B, H, W, step, E.COUNT, clip=1, scale=1.0)
    assert np.array_equal(clipped, binary)
    # voxel keeps every event's 65536 but what the two edge half-bins lose
    acc = E.accumulators_ref(samples, table, T, B, H, W, step, E.VOXEL)
    lost = 0
    for b in range(B):
        d = E.select_events(samples[b], table[b], T, H, W, step)[0]
        k, w0, w1 = E.voxel_weights(d, T, step)
        assert k.min() == -1 and k.max() == T - 1 and ((w0 > 0) & (w0 <= 65536)).all() and (w1 >= 0).all()
        lost += int(w0[k < 0].sum()) + int(w1[k + 1 > T - 1].sum())
    assert lost > 0 and int(acc.sum()) == 65536 * int(count.sum()) - lost


def test_voxel_weights_at_bin_centres_and_edges():
    for step in (1000, 16667, 2):
        # a bin centre is d = step/2 + j step; for an odd step no integer time lies on it
        if step % 2 == 0:
            for j in range(T):
                sample = ([step // 2 + j * step], [3], [2], [1], 0)
                acc = E.accumulators_ref([sample], R.identity_table(1), T, 1, H, W, step, E.VOXEL)
                assert acc[j, 0, 1, 2, 3] == 65536 and acc.sum() == 65536, (step, j)
        # d = 0: the first half-bin, k = -1; bin 0 gets q = floor(step 2^16 / (2 step)) = 2^15, the rest is lost
        acc = E.accumulators_ref([([0], [3], [2], [0], 0)], R.identity_table(1), T, 1, H, W, step, E.VOXEL)
        assert acc[0, 0, 0, 2, 3] == 32768 and acc.sum() == 32768
        # the last microsecond: k = T - 1, q = floor((step - 2) 2^16 / (2 step)) is lost, bin T-1 keeps 65536 - q
        q = ((step - 2) * 65536) // (2 * step)
        acc = E.accumulators_ref([([T * step - 1], [3], [2], [0], 0)], R.identity_table(1), T, 1, H, W, step, E.VOXEL)
        assert acc[T - 1, 0, 0, 2, 3] == 65536 - q and acc.sum() == 65536 - q
    # between two centres the two weights sum to 65536 and follow the distance
    k, w0, w1 = E.voxel_weights(np.array([1500 + 250]), T, 1000)
    assert (int(k[0]), int(w0[0]), int(w1[0])) == (1, 49152, 16384)


def test_finalize_rounds_once_per_operation():
    acc = np.array([0, 1, 2, 3, 5, (1 << 24) + 1, (1 << 32) - 1], dtype=np.uint64)
    third = np.float32(1.0) / np.float32(3.0)
    got = E.finalize_ref(acc, 1000, E.COUNT, 0, third)
    assert got.dtype == np.float32 and got[0] == 0 and not np.signbit(got[0])
    assert got[3] == np.float32(3.0) * third and got[5] == np.float32(1 << 24) * third
    assert np.array_equal(E.finalize_ref(acc, 1000, E.COUNT, 3, 1.0), np.float32([0, 1, 2, 3, 3, 3, 3]))
    t = E.finalize_ref(np.array([1, 1000], dtype=np.uint64), 1000, E.TIME, 0, 1.0)
    assert t[0] == np.float32(1) / np.float32(1000) and t[1] == 1.0
    v = E.finalize_ref(np.array([65536, 3 * 65536, 32768], dtype=np.uint64), 1000, E.VOXEL, 2, 1.0)
    assert np.array_equal(v, np.float32([1.0, 2.0, 0.5]))


# ------------------------------------------------------------------------------------------- ABI, header
def test_symbols_constants_and_abi():
    import snn_for_object_detection_amd as P
    from snn_for_object_detection_amd import _hip
    header = open(os.path.join(os.path.dirname(_hip._HERE), "include", "snn_hip.h")).read()
    assert re.search(r"#define\s+SNN_ABI_VERSION\s+20\b", header) and _hip.ABI_VERSION == 20
    for name, n_args in (("snn_events_rep_supported", 3), ("snn_events_to_frames_aug_rep", 18),
                         ("snn_events_to_frames_packed_rep", 15)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert len(_hip.SIGNATURES[name][1]) == n_args, name
    for name, value in (("BINARY", 0), ("COUNT", 1), ("TIME", 2), ("VOXEL", 3)):
        assert re.search(r"#define\s+SNN_EVREP_" + name + r"\s+" + str(value) + r"\b", header), name
        assert _hip.EVENT_REPS[name.lower()] == value == E.NAMES[name.lower()]
    # the three older entry points keep their signatures
    assert [len(_hip.SIGNATURES[n][1]) for n in ("snn_events_to_frames", "snn_events_to_frames_aug",
                                                 "snn_events_to_frames_packed")] == [10, 15, 12]
    assert hasattr(P, "EventRepresentation") and P.EventRepresentation.KINDS == ("binary", "count", "time", "voxel")


SUPPORTED = [  # rep, step_us, clip, answer
    (0, 1000, 0, 1), (0, 1 << 45, 0, 1), (0, 1000, 1, 0), (0, 0, 0, 0), (0, -5, 0, 0),
    (1, 1000, 0, 1), (1, 1000, 1, 1), (1, 1 << 45, 1 << 24, 1), (1, 1000, (1 << 24) + 1, 0), (1, 1000, -1, 0), (1, 0, 0, 0),
    (2, 1000, 0, 1), (2, (1 << 32) - 1, 0, 1), (2, 1 << 32, 0, 0), (2, 1000, 1, 0), (2, -1, 0, 0),
    (3, 1000, 0, 1), (3, 1000, 65535, 1), (3, 1000, 65536, 0), (3, 1000, -1, 0), (3, (1 << 40) - 1, 2, 1), (3, 1 << 40, 0, 0),
    (3, 0, 0, 0), (4, 1000, 0, 0), (-1, 1000, 0, 0),
]


def test_rep_supported_table(hip_lib):
    assert hip_lib.snn_abi_version() == 20
    for rep, step, clip, want in SUPPORTED:
        assert hip_lib.snn_events_rep_supported(rep, step, clip) == want, (rep, step, clip)


# ------------------------------------------------------------------------------------------- Python refusals
def test_event_representation_refusals_and_values(hip_lib):
    import snn_for_object_detection_amd as P
    Rp = P.EventRepresentation
    r = Rp("count", clip=3, scale=0.5)
    assert (r.kind, r.rep, r.clip, r.scale, r.is_binary) == ("count", 1, 3, 0.5, False)
    assert Rp("voxel").clip == 0 and Rp("binary").is_binary and Rp().kind == "binary"
    assert Rp("count", 3, 0.5) == r and Rp("count", 4, 0.5) != r and "count" in repr(r)
    assert Rp.of(None).is_binary and Rp.of("time").rep == 2 and Rp.of(r) is r
    assert Rp("count", scale=1 / 3).scale == float(np.float32(1 / 3))       # the fp32 value the kernel multiplies by
    with pytest.raises(ValueError, match="kind"):
        Rp("counts")
    with pytest.raises(ValueError, match="kind"):
        Rp(1)
    for bad in (-1, 2.5, "3", True):
        with pytest.raises(ValueError, match="clip"):
            Rp("count", clip=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-60, 1e60, "1", None):
        with pytest.raises(ValueError, match="scale"):
            Rp("count", scale=bad)
    with pytest.raises(ValueError, match="binary"):
        Rp("binary", clip=1)
    with pytest.raises(ValueError, match="binary"):
        Rp("binary", scale=2.0)
    with pytest.raises(ValueError, match="time surface"):
        Rp("time", clip=1)
    with pytest.raises(ValueError, match="representation"):
        Rp.of(3)
    # what the library refuses, asked through check()
    assert Rp("count", clip=1 << 24).check(1000) is not None and Rp("time").check((1 << 32) - 1) is not None
    for rep, step in ((Rp("count", clip=(1 << 24) + 1), 1000), (Rp("voxel", clip=65536), 1000), (Rp("time"), 1 << 32),
                      (Rp("voxel"), 1 << 40), (Rp("count", clip=1 << 40), 1000), (Rp("count"), 1 << 70)):
        with pytest.raises(ValueError, match="does not take"):
            rep.check(step)
    with pytest.raises(ValueError, match="step_us"):
        Rp("count").check(0)


def test_batcher_feed_and_op_refusals_come_before_any_device(hip_lib, tmp_path):
    import snn_for_object_detection_amd as P
    from snn_for_object_detection_amd import functional as HF
    # EventBatcher: the representation is checked before the device is asked for
    with pytest.raises(ValueError, match="EventBatcher: representation"):
        P.EventBatcher(T, H, W, 1000, device="cpu", representation=7)
    with pytest.raises(ValueError, match="kind"):
        P.EventBatcher(T, H, W, 1000, device="cpu", representation="histogram")
    with pytest.raises(ValueError, match="EventBatcher.*does not take"):
        P.EventBatcher(T, H, W, 1 << 32, device="cpu", representation="time")
    with pytest.raises(ValueError, match="EventBatcher.*does not take"):
        P.EventBatcher(T, H, W, 1000, device="cpu", representation=P.EventRepresentation("voxel", clip=1 << 16))
    with pytest.raises(ValueError, match="EventBatcher: step_us"):
        P.EventBatcher(T, H, W, 0, device="cpu", representation="count")
    with pytest.raises(RuntimeError, match="HIP device"):                   # a legal one reaches the device check
        P.EventBatcher(T, H, W, 1000, device="cpu", representation="count")
    # PropheseeFeed: before the directory is looked at
    with pytest.raises(ValueError, match="PropheseeFeed: representation"):
        P.PropheseeFeed(str(tmp_path), representation=1.5)
    with pytest.raises(ValueError, match="kind"):
        P.PropheseeFeed(str(tmp_path), representation="surface")
    with pytest.raises(ValueError, match="PropheseeFeed.*does not take"):
        P.PropheseeFeed(str(tmp_path), time_step=5_000_000, representation="time")     # 5e9 us per step
    with pytest.raises(RuntimeError, match="does not contain data"):
        P.PropheseeFeed(str(tmp_path), representation="voxel")
    # event_ops, on CPU tensors
    i64, i32 = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    off, t0, aug = torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(16, dtype=torch.int32)
    words = torch.zeros((4, 2), dtype=torch.int32)
    for name, call in (("events_to_frames_aug", lambda step, r: HF.events_to_frames_aug(i64, i32, i32, i32, off, t0, aug, T, H, W,
                                                                                        step, representation=r)),
                       ("events_to_frames_packed", lambda step, r: HF.events_to_frames_packed(words, off, t0, None, T, 2, H, W,
                                                                                              step, representation=r))):
        with pytest.raises(ValueError, match=name + ": representation"):
            call(1000, 3)
        with pytest.raises(ValueError, match="kind"):
            call(1000, "binary frames")
        with pytest.raises(ValueError, match=name + ".*does not take"):
            call(1 << 32, "time")
        with pytest.raises(ValueError, match=name + ".*does not take"):
            call(1000, P.EventRepresentation("count", clip=1 << 25))
        with pytest.raises(ValueError, match=name + ": step_us"):
            call(0, "count")
        with pytest.raises(ValueError, match=name + ".*HIP tensor"):        # a legal one reaches the tensor checks
            call(1000, "voxel")
    with pytest.raises(ValueError, match="aug may be None only"):
        HF.events_to_frames_aug(i64, i32, i32, i32, off, t0, None, T, H, W, 1000)
