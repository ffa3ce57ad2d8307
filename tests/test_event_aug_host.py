"""Host side of the augmented event feed: the numpy reference itself (hash known answers, the drop rate, the identity
against ``oracle.events``, the fixed-point zoom), ``EventAugment.draw`` and the C ABI declarations.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

from tests import event_aug_ref as R


def test_drop_hash_known_answers():
    cases = [(0, 0, 0x0), (1, 0, 0x514E28B7), (5, 12345, 0x40F1D0F0), ((1 << 32) + 7, 12345, 0xB4E2C78D)]
    for j, seed, want in cases:
        assert int(R.drop_hash(np.array([j], dtype=np.int64), seed)[0]) == want, (j, seed)


@pytest.mark.parametrize("seed", [12345, 0xDEADBEEF])
def test_drop_share_is_the_probability(seed):
    """40 000 consecutive indices at p = 0.25: a fair Bernoulli draw has sigma = sqrt(.25 * .75 / 40000) = 0.00217, the
    bound is 4 sigma rounded (0.2497 and 0.2493 for these two seeds)."""
    u = R.drop_hash(np.arange(40_000, dtype=np.int64), seed)
    share = float((u < np.uint64(1 << 30)).mean())
    assert 0.24 <= share <= 0.26, share


def test_identity_table_equals_the_oracle_voxelisation():
    from oracle import events as OE
    T, B, H, W, step = 4, 3, 6, 9, 1000
    rng = np.random.default_rng(11)
    samples, want = [], []
    for b in range(B):
        n, t0 = 300 + 50 * b, 7000 * (b + 1)
        t = rng.integers(t0 - 800, t0 + (T + 1) * step, n)
        x = rng.integers(-2, W + 3, n)
        y = rng.integers(0, H, n)
        p = rng.integers(0, 2, n)
        samples.append((t, x, y, p, t0))
        want.append(OE.voxelize(t, x, y, p, t0, step, T, H, W))
    got = R.frames_ref(samples, R.identity_table(B), T, B, H, W, step)
    assert np.array_equal(got, np.stack(want, axis=1).astype(np.uint8))
    assert got.sum() > 0


@pytest.mark.parametrize("a", [1 << 14, 1 << 18, 40001, 65537, 98303])
def test_fixed_point_zoom_maps_the_pixel_centre(a):
    """(((2x + 1) a) >> 17) == floor((x + 0.5) a / 65536), in exact rational arithmetic."""
    x = np.arange(4096, dtype=np.int64)
    assert np.array_equal(((2 * x + 1) * a) >> 17, ((2 * x + 1) * a) // (2 * 65536))
    import math
    from fractions import Fraction
    for xi in (0, 1, 2, 3, 1279, 4095):
        assert int(((2 * xi + 1) * a) >> 17) == math.floor(Fraction(2 * xi + 1, 2) * Fraction(a, 65536))


def test_draw_is_reproducible_per_seed():
    from snn_for_object_detection_amd import EventAugment
    kw = dict(hflip=0.5, zoom=(0.75, 1.25), drop=(0.0, 0.1))
    state = torch.random.get_rng_state()
    a, b, c = EventAugment(seed=7, **kw), EventAugment(seed=7, **kw), EventAugment(seed=8, **kw)
    ta = [a.draw(5, 304, 240) for _ in range(3)]
    tb = [b.draw(5, 304, 240) for _ in range(3)]
    tc = [c.draw(5, 304, 240) for _ in range(3)]
    assert all(torch.equal(u, v) for u, v in zip(ta, tb))
    assert not torch.equal(ta[0], ta[1])                        # the generator advances
    assert not any(torch.equal(u, v) for u, v in zip(ta, tc))
    assert ta[0].dtype == torch.int32 and ta[0].shape == (5, 8) and not ta[0].is_cuda
    assert torch.equal(torch.random.get_rng_state(), state)    # the global RNG is never touched
    assert len({int(s) for s in ta[0][:, 5]}) == 5              # a fresh seed per sample
    assert torch.equal(EventAugment.identity(2), torch.from_numpy(R.identity_table(2)))


@pytest.mark.parametrize("W,H", [(7, 5), (304, 240)])
def test_draw_stays_inside_its_ranges(W, H):
    from snn_for_object_detection_amd import EventAugment
    lo, hi = 0.25, 4.0
    aug = EventAugment(hflip=0.5, zoom=(lo, hi), drop=(0.05, 0.3), seed=1)
    t = torch.cat([aug.draw(50, W, H) for _ in range(20)]).numpy().astype(np.int64)   # 1 000 draws
    a = t[:, 1]
    assert a.min() >= round(lo * 65536) and a.max() <= round(hi * 65536)
    assert a.min() < 65536 < a.max()
    for col, size in ((2, W), (3, H)):
        room = size - -((-a * size) // 65536)                    # size - ceil(s size), s = a / 65536
        assert (t[:, col] >= np.minimum(0, room)).all() and (t[:, col] <= np.maximum(0, room)).all()
        # both ends of a range are reached somewhere in 1 000 draws of a small frame
        if size <= 7:
            assert (t[:, col] == np.minimum(0, room)).any() and (t[:, col] == np.maximum(0, room)).any()
        # a zoomed-out image lies wholly inside the frame: its first and last pixel centres do
        last = (((2 * (size - 1) + 1) * a) >> 17) + t[:, col]
        out = a <= 65536
        assert (t[out, col] >= 0).all() and (last[out] <= size - 1).all()
    drop = t[:, 4] & 0xFFFFFFFF
    assert drop.min() >= int(0.05 * 2 ** 32) and drop.max() <= int(0.3 * 2 ** 32)
    assert set(np.unique(t[:, 0])) == {0, 1}
    assert (t[:, 6:] == 0).all()
    plain = EventAugment(seed=1).draw(10, W, H).numpy()
    assert (plain[:, 1] == 65536).all() and (plain[:, [0, 2, 3, 4, 6, 7]] == 0).all()


def test_flip_probability_ends():
    from snn_for_object_detection_amd import EventAugment
    assert int(EventAugment(hflip=0.0, seed=3).draw(1000, 7, 5)[:, 0].sum()) == 0
    assert int(EventAugment(hflip=1.0, seed=3).draw(1000, 7, 5)[:, 0].sum()) == 1000


def test_bad_arguments_raise_by_name():
    from snn_for_object_detection_amd import EventAugment
    from snn_for_object_detection_amd import functional as HF
    for kw, name in ((dict(hflip=1.5), "hflip"), (dict(hflip=-0.1), "hflip"), (dict(zoom=(0.2, 1.0)), "zoom"),
                     (dict(zoom=(1.0, 4.5)), "zoom"), (dict(zoom=(1.5, 1.0)), "zoom"), (dict(zoom=(1.0,)), "zoom"),
                     (dict(drop=1.0), "drop"), (dict(drop=(0.3, 0.1)), "drop"), (dict(drop=-0.1), "drop"),
                     (dict(min_visible=1.5), "min_visible"), (dict(min_size_px=-1.0), "min_size_px")):
        with pytest.raises(ValueError, match=name):
            EventAugment(**kw)
    with pytest.raises(ValueError, match="W and H"):
        EventAugment().draw(2)
    good = EventAugment.identity(3)
    assert HF.check_aug_table(good, 3) is not None
    for bad, name in ((good[:2], "shape"), (good[:, :7], "shape"), (good.long(), "int32"), (good.float(), "int32")):
        with pytest.raises(ValueError, match=name):
            HF.check_aug_table(bad, 3)
    for a in ((1 << 14) - 1, (1 << 18) + 1, 0, -65536):
        t = good.clone()
        t[1, 1] = a
        with pytest.raises(ValueError, match="a_q16"):
            HF.check_aug_table(t, 3)
    t = good.clone()
    t[2, 0] = 2
    with pytest.raises(ValueError, match="flip"):
        HF.check_aug_table(t, 3)


def test_the_two_symbols_are_declared_and_abi_stays_20():
    from snn_for_object_detection_amd import _hip
    header = open(os.path.join(os.path.dirname(_hip._HERE), "include", "snn_hip.h")).read()
    assert re.search(r"#define\s+SNN_ABI_VERSION\s+20\b", header) and _hip.ABI_VERSION == 20
    for name, n_args in (("snn_events_to_frames_aug", 15), ("snn_labels_augment", 11)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name][1]) == n_args
