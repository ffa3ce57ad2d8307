"""Device mAP with area ranges, per-class output, the box-size filter and the cross-rank compute (csrc/metrics.hip behind
metrics.MeanAveragePrecision and SODa's hooks) against the fp64 restatement tests/coco_area_ref.py: matched / ignored
masks, ground-truth counts and scores exactly, summaries and per-class vectors to 1e-6 (the tolerance
tests/test_gpu_map.py holds for the same fp64-then-fp32 arithmetic)."""
import datetime
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.coco_area_ref import evaluate as evaluate_areas
from tests.coco_map_ref import IOU_THRESHOLDS, MAX_DETS, REC_THRESHOLDS
from tests.test_gpu_map import KEYS, pad
from tests.test_map_area_semantics import AREA_CASES, SIZE, area_set, area_set_reference, case_reference

pytestmark = pytest.mark.gpu

RANGE_KEYS = ("map_small", "mar_small", "map_medium", "mar_medium", "map_large", "mar_large")
FRAME = (240, 304)
EVERY = dict(class_metrics=True, area_ranges=True)


@pytest.fixture(scope="module")
def pkg(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import snn_for_object_detection_amd as p
    return p


def device_metric(pkg, images, C, batches=1, **kw):
    m = pkg.metrics.MeanAveragePrecision(C, **kw)
    for part in np.array_split(np.arange(len(images)), batches):
        if len(part):
            d, g = pad([images[i] for i in part])
            m.update_padded(torch.from_numpy(d).cuda(), torch.from_numpy(g).cuda())
    return m


def assert_result(got, want, C, per_class=True):
    for k in KEYS + RANGE_KEYS:
        assert got[k].is_cuda and got[k].dim() == 0 and got[k].dtype == torch.float32
        assert abs(float(got[k]) - want[k]) <= 1e-6, (k, float(got[k]), want[k])
    if per_class:
        assert got["classes"].dtype == torch.int32 and got["classes"].tolist() == list(range(C))
        for key, ref in (("map_per_class", "map_per_class"), ("mar_100_per_class", "mar_per_class")):
            assert got[key].is_cuda and got[key].shape == (C,) and got[key].dtype == torch.float32
            assert np.abs(got[key].cpu().numpy().astype(np.float64) - np.array(want[ref])).max() <= 1e-6, key


def assert_records(m, rec):
    """The metric's state against the restatement's records, exactly."""
    assert np.array_equal(torch.cat(m._scores).cpu().numpy(), rec["score"])
    assert np.array_equal(torch.cat(m._masks).cpu().numpy().view(np.uint32), rec["mask"])
    assert np.array_equal(torch.cat(m._area_matched).cpu().numpy().view(np.uint32), rec["matched"])
    assert np.array_equal(torch.cat(m._area_ignored).cpu().numpy().view(np.uint32), rec["ignored"])
    assert np.array_equal(m._npig.cpu().numpy(), rec["npig"])
    assert np.array_equal(m._npig_area.cpu().numpy(), rec["npig_area"])


@pytest.mark.parametrize("name", sorted(AREA_CASES))
def test_hand_cases_on_device(pkg, name):
    case = AREA_CASES[name]
    want, rec = case_reference(name)
    m = device_metric(pkg, case["images"], case["C"], image_size=SIZE, **EVERY, **case.get("kw", {}))
    assert_records(m, rec)
    got = m.compute()
    assert_result(got, want, case["C"])
    for k, v in case["expect"].items():
        assert abs(float(got[k]) - v) <= 1e-6, (k, float(got[k]), v)


def _abi_run(images, C, min_box_diag=0.0, min_box_side=0.0, old_match=True):
    """The new entry points called directly: row filter, host stable sort of its keys, match with areas, accumulate with
    areas; every output NaN-filled first.  ``old_match``: also snn_map_match on the same rows, for its mask."""
    from snn_for_object_detection_amd import _hip
    st = torch.cuda.current_stream().cuda_stream
    S, T, R, M, NR = MAX_DETS[-1], len(IOU_THRESHOLDS), len(REC_THRESHOLDS), len(MAX_DETS), 3
    dets, labels = pad(images)
    B, A, G = dets.shape[0], dets.shape[1], labels.shape[1]
    nan = float("nan")

    def nans(*shape, dtype=torch.float32):
        return torch.full(shape, nan, device="cuda").view(dtype)

    d, g = torch.from_numpy(dets).cuda(), torch.from_numpy(labels).cuda()
    key, label_cls = nans(B, A, dtype=torch.int32), nans(B, G)
    bad = torch.zeros((), device="cuda", dtype=torch.int64)
    _hip.call("snn_map_filter_rows", d.data_ptr(), g.data_ptr(), B, A, G, C, float(FRAME[0]), float(FRAME[1]),
              min_box_diag, min_box_side, key.data_ptr(), label_cls.data_ptr(), bad.data_ptr(), st)
    keys = key.cpu().numpy()
    assert int(bad) == 0 and keys.min() >= 0 and keys.max() <= C + 1
    order = np.zeros((B, A), dtype=np.int32)
    seg = np.zeros((B, C + 1), dtype=np.int32)
    for b in range(B):
        order[b] = np.lexsort((np.arange(A), -dets[b, :, 1], keys[b]))
        seg[b] = np.searchsorted(keys[b][order[b]], np.arange(C + 1), side="left")
    o, s = torch.from_numpy(order).cuda(), torch.from_numpy(seg).cuda()
    iou = torch.tensor(IOU_THRESHOLDS, dtype=torch.float64, device="cuda")
    score, mask = nans(B, C, S), nans(B, C, S, dtype=torch.int32)
    matched, ignored = nans(B, C, NR, S, dtype=torch.int32), nans(B, C, NR, S, dtype=torch.int32)
    npig = torch.zeros(C, device="cuda", dtype=torch.int32)
    npig_area = torch.zeros(NR, C, device="cuda", dtype=torch.int32)
    _hip.call("snn_map_match_areas", d.data_ptr(), g.data_ptr(), label_cls.data_ptr(), o.data_ptr(), s.data_ptr(), B, A, G,
              C, S, iou.data_ptr(), T, float(FRAME[0]), float(FRAME[1]), NR, score.data_ptr(), mask.data_ptr(),
              matched.data_ptr(), ignored.data_ptr(), npig.data_ptr(), npig_area.data_ptr(), st)
    out = dict(score=score.cpu().numpy(), mask=mask.cpu().numpy().view(np.uint32),
               matched=matched.cpu().numpy().view(np.uint32), ignored=ignored.cpu().numpy().view(np.uint32),
               npig=npig.cpu().numpy(), npig_area=npig_area.cpu().numpy(), label_cls=label_cls.cpu().numpy())
    if old_match:
        score0, mask0 = nans(B, C, S), nans(B, C, S, dtype=torch.int32)
        npig0 = torch.zeros(C, device="cuda", dtype=torch.int32)
        _hip.call("snn_map_match", d.data_ptr(), g.data_ptr(), o.data_ptr(), s.data_ptr(), B, A, G, C, S, iou.data_ptr(), T,
                  score0.data_ptr(), mask0.data_ptr(), npig0.data_ptr(), st)
        out["old_mask"] = mask0.cpu().numpy().view(np.uint32)
    sc = out["score"].transpose(1, 0, 2).reshape(C, B * S)
    ords = torch.from_numpy(np.stack([np.argsort(-sc[c], kind="stable") for c in range(C)]).astype(np.int32)).cuda()
    mt = mask.permute(1, 0, 2).reshape(C, B * S).contiguous()
    am = matched.permute(1, 2, 0, 3).reshape(C, NR, B * S).contiguous()
    ai = ignored.permute(1, 2, 0, 3).reshape(C, NR, B * S).contiguous()
    ws = torch.full((_hip.query("snn_map_areas_workspace_size", C, M, T, NR) // 8,), nan, device="cuda",
                    dtype=torch.float64)
    summary, per_class = nans(3 + M + 2 * NR), nans(2, C)
    md = torch.tensor(MAX_DETS, dtype=torch.int32, device="cuda")
    rec = torch.tensor(REC_THRESHOLDS, dtype=torch.float64, device="cuda")
    _hip.call("snn_map_accumulate_areas", ords.data_ptr(), mt.data_ptr(), am.data_ptr(), ai.data_ptr(), npig.data_ptr(),
              npig_area.data_ptr(), C, B * S, S, md.data_ptr(), M, rec.data_ptr(), R, T, 0, 5, NR, ws.data_ptr(),
              summary.data_ptr(), per_class.data_ptr(), st)
    torch.cuda.synchronize()
    out["summary"], out["per_class"] = summary.cpu().numpy(), per_class.cpu().numpy()
    return out


def assert_abi(got, want, rec):
    for k in ("npig", "npig_area", "mask", "matched", "ignored", "score"):      # -inf in the empty slots, no NaN left
        assert np.array_equal(got[k], rec[k]), k
    if "old_mask" in got:
        assert np.array_equal(got["mask"], got["old_mask"])
    assert IOU_THRESHOLDS[0] == 0.5 and IOU_THRESHOLDS[5] == 0.75
    for k, v in zip(KEYS + RANGE_KEYS, got["summary"]):
        assert abs(float(v) - want[k]) <= 1e-6, (k, float(v), want[k])
    assert np.abs(got["per_class"][0].astype(np.float64) - np.array(want["map_per_class"])).max() <= 1e-6
    assert np.abs(got["per_class"][1].astype(np.float64) - np.array(want["mar_per_class"])).max() <= 1e-6


SETS = [(1, 6, 2), (2, 16, 3), (3, 10, 1)]


@pytest.mark.parametrize("seed,n_images,C", SETS)
def test_random_sets_through_the_abi(pkg, seed, n_images, C):
    images, want, rec = area_set_reference(seed, n_images, C)
    # the restatement alone says that the set exercises the rules
    assert (rec["npig_area"] > 0).any(axis=1).all(), rec["npig_area"]
    assert rec["ignored_by_gt"] > 0 and rec["ignored_unmatched"] > 0 and rec["preferred"] > 0
    assert_abi(_abi_run(images, C), want, rec)
    # the metric object over several updates: the same records and summaries
    m = device_metric(pkg, images, C, batches=3, image_size=FRAME, **EVERY)
    assert_records(m, rec)
    assert_result(m.compute(), want, C)


def _crossing_set(seed, n_gt, n_det):
    """One class; image k has exactly n_gt[k] ground-truth rows and n_det[k] detections."""
    images = []
    for k, (ng, nd) in enumerate(zip(n_gt, n_det)):
        rng = np.random.default_rng(seed + k)
        side = 0.02 + rng.random((ng, 2)) ** 2 * 0.6
        lo = rng.random((ng, 2)) * (1 - side)
        boxes = np.concatenate([lo, lo + side], axis=1)
        gts = np.concatenate([np.zeros((ng, 1)), boxes], axis=1)
        dets = np.zeros((nd, 6))
        dets[:, 2:] = boxes[rng.integers(0, ng, nd)] + rng.normal(0, 0.01, (nd, 4))
        dets[:, 4:] = np.maximum(dets[:, 4:], dets[:, 2:4] + 1 / 512)
        dets[:, 1] = rng.integers(0, 65, nd) / 64
        images.append((dets.astype(np.float32), gts.astype(np.float32)))
    return images


def test_compaction_chunks_and_the_cut(pkg):
    """More than 64 and more than 128 ground-truth rows of one class (two and three ballot chunks, with their ignore
    bits) and more than 100 detections of the class (the cut to the largest maxDet before matching)."""
    images = _crossing_set(40, n_gt=(70, 140), n_det=(130, 90))
    want, rec = evaluate_areas(images, 1, FRAME)
    assert (rec["npig_area"] > 0).all() and rec["ignored_by_gt"] > 0
    assert_abi(_abi_run(images, 1), want, rec)


def test_filter_removes_rows_that_would_have_made_the_cut(pkg):
    """With min_box_side set, detections among an image's top 100 go and later ones move up into the cut: the kept
    scores differ from the unfiltered ones, which the restatement shows first."""
    images = _crossing_set(50, n_gt=(30,), n_det=(260,))
    side = 12.0
    want, rec = evaluate_areas(images, 1, FRAME, min_box_side=side, min_box_diag=25.0)
    _, plain = evaluate_areas(images, 1, FRAME)
    assert (np.isfinite(plain["score"]).sum(), np.isfinite(rec["score"]).sum()) == (100, 100)
    assert not np.array_equal(plain["score"], rec["score"]) and rec["npig"][0] < plain["npig"][0]
    got = _abi_run(images, 1, min_box_diag=25.0, min_box_side=side, old_match=False)
    assert_abi(got, want, rec)
    assert (got["label_cls"] < 0).sum() == 30 - rec["npig"][0]
    m = device_metric(pkg, images, 1, image_size=FRAME, min_box_side=side, min_box_diag=25.0)      # the filter alone
    assert not m._area_matched and np.array_equal(torch.cat(m._masks).cpu().numpy().view(np.uint32), rec["mask"])
    got = m.compute()
    assert set(got) == set(KEYS)
    for k in KEYS:
        assert abs(float(got[k]) - want[k]) <= 1e-6, (k, float(got[k]), want[k])


def test_defaults_are_untouched_and_bit_equal(pkg):
    images, want, _ = area_set_reference(1, 6, 2)
    plain = device_metric(pkg, images, 2, batches=2).compute()
    assert set(plain) == set(KEYS)
    full = device_metric(pkg, images, 2, batches=2, image_size=FRAME, **EVERY).compute()
    assert set(full) == set(KEYS + RANGE_KEYS) | {"map_per_class", "mar_100_per_class", "classes"}
    only_classes = device_metric(pkg, images, 2, batches=2, class_metrics=True).compute()
    for k in KEYS:
        assert torch.equal(plain[k], full[k]) and torch.equal(plain[k], only_classes[k]), k
    assert torch.equal(only_classes["map_per_class"], full["map_per_class"])
    with pytest.raises(ValueError, match="image_size"):
        device_metric(pkg, images, 2, area_ranges=True)
    with pytest.raises(ValueError, match="image_size"):
        device_metric(pkg, images, 2, min_box_side=4.0)
    empty = pkg.metrics.MeanAveragePrecision(2, image_size=FRAME, **EVERY).compute()
    assert set(empty) == set(full) and all(float(empty[k]) == -1.0 for k in KEYS + RANGE_KEYS)
    assert empty["map_per_class"].tolist() == [-1.0, -1.0]


def test_update_padded_with_every_option_does_not_synchronise(pkg):
    images, _, _ = area_set_reference(1, 6, 2)
    d, g = pad(images)
    d, g = torch.from_numpy(d).cuda(), torch.from_numpy(g).cuda()
    m = pkg.metrics.MeanAveragePrecision(2, min_box_diag=6.0, min_box_side=3.0, **EVERY)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            d.sum().item()                   # the mode is live
        m.update_padded(d, g, image_size=FRAME)          # the size given per batch
        m.update_padded(d[:3], g[:3], image_size=FRAME)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    want, _ = evaluate_areas(images + images[:3], 2, FRAME, min_box_diag=6.0, min_box_side=3.0)
    assert_result(m.compute(), want, 2)


@pytest.mark.parametrize("stage", ["validation", "test"])
def test_soda_hooks_log_the_selected_keys(pkg, stage):
    from tests.util import synthetic_events, synthetic_labels
    from torch.nn import functional as F
    opts = dict(area_ranges=True, class_metrics=True, min_box_side=2.0)
    torch.manual_seed(3)
    default = pkg.TinyYolo(num_classes=2, time_window=0)
    torch.manual_seed(3)
    model = pkg.TinyYolo(num_classes=2, time_window=0, map_options=opts)
    assert list(model.state_dict().keys()) == list(default.state_dict().keys())
    default, model = default.cuda().eval(), model.cuda().eval()
    images = []
    with torch.no_grad():
        for k in range(2):
            X = synthetic_events(4, 2, 32, 48, p=0.08, seed=10 + k).cuda()
            labels = synthetic_labels(2, n_boxes=3, seed=20 + k, pad_rows=1).cuda()
            anchors, cls, bbox = model.forward(X)
            dets = pkg.box.multibox_detection(F.softmax(cls, dim=2), bbox, anchors)
            getattr(model, f"{stage}_step")((X, labels), k)
            getattr(default, f"{stage}_step")((X, labels), k)
            images += [(dets[b].cpu().numpy(), labels[b].cpu().numpy()) for b in range(2)]
        getattr(model, f"on_{stage}_epoch_end")()
        getattr(default, f"on_{stage}_epoch_end")()
    loss = "val_loss" if stage == "validation" else "test_loss"
    five = {"map", "map_50", "mar_1", "mar_10", "mar_100"}
    assert set(default.logged) == five | {loss}
    added = set(RANGE_KEYS) | {f"{a}_class_{c}" for a in ("map", "mar") for c in range(2)}
    assert set(model.logged) == five | {loss} | added
    want, _ = evaluate_areas(images, 2, (32, 48), min_box_side=2.0)
    want.update({f"map_class_{c}": want["map_per_class"][c] for c in range(2)})
    want.update({f"mar_class_{c}": want["mar_per_class"][c] for c in range(2)})
    for k in five | added:
        assert abs(float(model.logged[k]) - want[k]) <= 1e-6, (k, float(model.logged[k]), want[k])
    assert not model.map_metric._scores and not model.map_metric._area_matched        # reset after the epoch
    with pytest.raises(TypeError):
        pkg.TinyYolo(num_classes=2, time_window=0, map_options=dict(no_such_option=1))


# ------------------------------------------------------------------------------------------ two ranks on one GPU
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


SHARDS = {"uneven": ([0, 1, 2, 3], [4, 5]), "rank1_empty": ([0, 1, 2], [])}


def _rank_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        from snn_for_object_detection_amd.metrics import MeanAveragePrecision
        torch.cuda.set_device(0)
        images = area_set(1, 6, 2)
        out = {}
        for name, shards in SHARDS.items():
            for sync in (True, False):
                m = MeanAveragePrecision(2, image_size=FRAME, sync_on_compute=sync, **EVERY)
                for i in shards[rank]:                       # one update per image: the ranks differ in update count
                    d, g = pad([images[i]])
                    m.update_padded(torch.from_numpy(d).cuda(), torch.from_numpy(g).cuda())
                out[name, sync] = {k: v.cpu() for k, v in m.compute().items()}
        torch.save(out, os.path.join(out_dir, f"map{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_two_ranks_compute_the_union(pkg, tmp_path):
    """``sync_on_compute=True``: both ranks return the bits of one metric fed rank 0's images, then rank 1's - with
    uneven shards and with a rank that never updated; the default stays each rank's own shard."""
    world = 2
    mp.spawn(_rank_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(tmp_path / f"map{k}.pt") for k in range(world)]
    images = area_set(1, 6, 2)

    def single(ids):
        m = pkg.metrics.MeanAveragePrecision(2, image_size=FRAME, **EVERY)
        for i in ids:
            d, g = pad([images[i]])
            m.update_padded(torch.from_numpy(d).cuda(), torch.from_numpy(g).cuda())
        return {k: v.cpu() for k, v in m.compute().items()}

    for name, shards in SHARDS.items():
        union = single(shards[0] + shards[1])
        assert float(union["map"]) > 0
        for k, v in union.items():
            assert torch.equal(r[0][name, True][k], v) and torch.equal(r[1][name, True][k], v), (name, k)
        for rank in range(world):
            own = single(shards[rank])
            for k, v in own.items():
                assert torch.equal(r[rank][name, False][k], v), (name, rank, k)
    assert not torch.equal(r[0]["uneven", False]["map"], r[1]["uneven", False]["map"])
