"""Batched detection decode (``box.multibox_detection_batched``: decode, greedy NMS and row assembly of ``csrc/detect.hip``
for N frames without a loop over them) against the per-frame device path, frame by frame and element for element,
and against the reference-generated goldens."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# frame kinds of frames(); the seed is chosen so that on the host path (multibox_detection on CPU tensors) every kind but
# "background" keeps at least one row and suppresses at least one
KINDS = ("general", "scattered", "background", "class_missing", "one_class", "duplicates", "ties")
SEED = 7


@pytest.fixture(scope="module")
def box(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from snn_for_object_detection_amd import box
    return box


def make_anchors(A, gen):
    """Random small anchors; the first 40 come in 20 identical pairs (the "duplicates" frame decodes them identically)."""
    centers = torch.rand(A, 2, generator=gen)
    wh = 0.02 + 0.1 * torch.rand(A, 2, generator=gen)
    anchors = torch.cat([centers - wh / 2, centers + wh / 2], dim=1)
    anchors[1:40:2] = anchors[0:40:2]
    return anchors


def frame(kind, anchors, K, gen):
    """``(probs[A,K], offsets[A,4])`` whose decoded boxes crowd around six centres (offset_boxes towards a jittered copy of
    the centre's box), so that greedy NMS suppresses most candidates of a class."""
    from snn_for_object_detection_amd import box
    A = anchors.shape[0]
    centre = 0.2 + 0.6 * torch.rand(6, 2, generator=gen)
    size = 0.1 + 0.1 * torch.rand(6, 2, generator=gen)
    which = torch.randint(0, 6, (A,), generator=gen)
    c = centre[which] + 0.01 * torch.randn(A, 2, generator=gen)
    s = size[which] * (1 + 0.05 * torch.randn(A, 2, generator=gen))
    offsets = box.offset_boxes(anchors, torch.cat([c - s / 2, c + s / 2], dim=1))
    logits = 4 * torch.randn(A, K, generator=gen)
    if kind == "scattered":              # boxes near their anchors: hundreds of kept rows per class, several 256-box tiles
        offsets = 0.3 * torch.randn(A, 4, generator=gen)
    elif kind == "background":
        logits[:, 0] += 40
    elif kind == "class_missing":        # class 0 (column 1) has no member
        logits[:, 1] -= 40
    probs = torch.softmax(logits, dim=1)
    if kind == "one_class":              # every anchor is class 1: one (class, frame) block walks all A candidates
        p = 0.5 + 0.5 * torch.rand(A, generator=gen)
        probs = ((1 - p) / (K - 1)).unsqueeze(1).repeat(1, K)
        probs[:, 2] = p
    elif kind == "duplicates":           # identical anchors, offsets and probabilities: identical boxes, equal confidences
        offsets[1:40:2] = offsets[0:40:2]
        probs[1:40:2] = probs[0:40:2]
    elif kind == "ties":                 # seven distinct probability rows: groups of exactly equal confidence
        table = torch.softmax(2 * torch.randn(7, K, generator=gen), dim=1)
        probs = table[torch.randint(0, 7, (A,), generator=gen)]
    return probs, offsets


def frames(kinds, A, K, seed=SEED):
    gen = torch.Generator().manual_seed(seed)
    anchors = make_anchors(A, gen)
    pairs = [frame(k, anchors, K, gen) for k in kinds]
    return torch.stack([p for p, _ in pairs]), torch.stack([o for _, o in pairs]), anchors


def kept_and_suppressed(probs, det):
    """Of one frame: rows kept (class >= 0; no confidence is below pos_threshold here) and foreground rows not kept."""
    foreground = int((probs.argmax(1) > 0).sum())
    kept = int((det[:, 0] >= 0).sum())
    return kept, foreground - kept


CASES = [
    # A = 700: three 256-candidate chunks, the last one partial
    (700, 3, ("general",)),
    (700, 8, ("general",)),
    (700, 3, ("one_class", "duplicates")),
    (700, 8, ("one_class", "duplicates")),
    (700, 3, ("background", "class_missing", "one_class", "duplicates", "ties")),
    (700, 8, ("background", "class_missing", "one_class", "duplicates", "ties")),
    # GEN1 anchor count: a kept list and a candidate list of many chunks
    (13545, 3, ("scattered", "one_class")),
]


@pytest.mark.parametrize("A,K,kinds", CASES, ids=[f"A{a}-K{k}-N{len(kd)}" for a, k, kd in CASES])
def test_batched_equals_per_frame(box, A, K, kinds):
    """Every frame of the batched result is torch.equal to the per-frame device path on that frame alone."""
    probs, offs, anchors = frames(kinds, A, K)
    pd, od, ad = probs.cuda(), offs.cuda(), anchors.cuda()
    for nms_thr, pos_thr in ((0.1, 0.009999999), (0.45, 0.5)):   # (the second: rows below pos_threshold, 1 - conf)
        want = [box._multibox_detection_device(pd[n:n + 1], od[n:n + 1], ad, nms_thr, pos_thr)[0]
                for n in range(len(kinds))]
        if pos_thr < 0.1:
            # not vacuous, judged on the yardstick: NMS keeps something and suppresses something in every frame
            for kind, p, w in zip(kinds, probs, want):
                kept, suppressed = kept_and_suppressed(p, w.cpu())
                if kind == "background":
                    assert kept == 0
                else:
                    assert kept >= 1 and suppressed >= 1, (kind, kept, suppressed)
                if kind == "one_class":
                    assert kept + suppressed == A and kept > 1
                if kind == "scattered":
                    assert kept > 600, kept
        got = box.multibox_detection_batched(pd, od, ad, nms_thr, pos_thr)
        assert got.shape == (len(kinds), A, 6)
        for n, kind in enumerate(kinds):
            assert torch.equal(got[n], want[n]), (kind, nms_thr, pos_thr)
        if len(kinds) > 1:   # the public entry point takes the batched path for B > 1
            assert torch.equal(box.multibox_detection(pd, od, ad, nms_thr, pos_thr), got)


@pytest.mark.parametrize("fixture,anchor_key", [("detect_nms.npz", None), ("detect_nms_mid.npz", "anchors")])
def test_batched_matches_reference_goldens(box, fixture, anchor_key):
    """The reference's own utils/box.py outputs, stacked three times with the frames in different positions: each frame
    of the batched result meets the comparison tests/test_gpu_detect.py makes for the single-frame path."""
    from tests.test_gpu_detect import _npz, _rows_equal_up_to_ties
    g = _npz(fixture)
    anchors = torch.from_numpy(g[anchor_key] if anchor_key else _npz("detect_anchors.npz")["anchors_tiny"])
    probs, offs, ref = (torch.from_numpy(g[k]) for k in ("probs", "offsets", "detections"))
    pick = torch.tensor([0, 1, 1, 0, 1, 0])                     # the fixture's two frames, three times
    det = box.multibox_detection_batched(probs[pick].cuda(), offs[pick].cuda(), anchors.cuda()).cpu()
    _rows_equal_up_to_ties(det, ref[pick])


def test_batched_does_not_synchronise(box):
    kinds = ("general", "one_class", "ties")
    probs, offs, anchors = frames(kinds, 700, 3)
    pd, od, ad = probs.cuda(), offs.cuda(), anchors.cuda()
    want = torch.stack([box._multibox_detection_device(pd[n:n + 1], od[n:n + 1], ad, 0.1, 0.009999999)[0]
                        for n in range(len(kinds))])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            pd.sum().item()                  # the mode is live: a host read of a device value raises
        got = box.multibox_detection_batched(pd, od, ad)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(got, want)
