"""``SODa.predict_sequence``: the detections of every timestep from ONE layer-major pass and one batched decode, against
the frame-by-frame ``predict`` loop (the reference's ``predict_step``), on the tiny detectors."""
import pytest
import torch
import torch.nn.functional as F

from tests.util import executor_net, synthetic_events

pytestmark = pytest.mark.gpu

T = 6
# description -> (classes, H, W): the sizes the existing tests run these descriptions at
NETS = {"executor": (3, 24, 32), "tinyyolo": (2, 32, 48)}


def build(pkg, name):
    torch.manual_seed(3)
    cls = executor_net(pkg) if name == "executor" else pkg.TinyYolo
    return cls(num_classes=NETS[name][0], time_window=0).cuda().eval()


def leaves(state):
    """The tensors of a nested detector state, in order."""
    if isinstance(state, torch.Tensor):
        return [state]
    if isinstance(state, (list, tuple)):
        return [t for s in state for t in leaves(s)]
    return []


class Run:
    """One model on one clip: the time-outer loop (raw predictions and detections of every step, computed once) and
    the model itself for the sequence calls."""

    def __init__(self, pkg, name, B):
        from snn_for_object_detection_amd import box
        _, H, W = NETS[name]
        self.model = build(pkg, name)
        self.X = synthetic_events(T, B, H, W, p=0.1, seed=11).cuda()
        self.cls, self.bbox, self.dets = [], [], []
        state = None
        with torch.no_grad():
            for t in range(T):
                (anchors, cls, bbox), state = self.model._forward_impl(self.X[t], state)
                self.cls.append(cls)
                self.bbox.append(bbox)
                # predict's tail (soda.py:202-233), sample by sample on the single-frame decode
                per_sample = []
                for b in range(B):
                    d = box._multibox_detection_device(F.softmax(cls, dim=2)[b:b + 1], bbox[b:b + 1], anchors,
                                                       0.1, 0.009999999)[0]
                    d = d[d[:, 0] >= 0]
                    d[:, 2:] = torch.clamp(d[:, 2:], min=0.0, max=1.0)
                    per_sample.append(d)
                self.dets.append(per_sample)
        self.anchors, self.state = anchors, state


@pytest.fixture(scope="module")
def pkg(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import snn_for_object_detection_amd as p
    return p


@pytest.fixture(scope="module")
def runs(pkg):
    cache = {}

    def get(name, B):
        if (name, B) not in cache:
            cache[name, B] = Run(pkg, name, B)
        return cache[name, B]
    return get


CASES = [(n, b) for n in NETS for b in (1, 2)]


@pytest.mark.parametrize("name,B", CASES)
def test_all_steps_head_outputs_equal_the_time_outer_loop(runs, name, B):
    """cls_preds[T,B,A,C+1] / bbox_preds[T,B,A,4] of one pass with all_steps=True, timestep by timestep, against the loop
    over single frames - the comparison test_gpu_model.py makes for layer-major against time-outer: torch.equal."""
    r = runs(name, B)
    with torch.no_grad():
        (anchors, cls, bbox), state = r.model._forward_impl(r.X, None, all_steps=True)
        _, cls_last, bbox_last = r.model(r.X)
    A = anchors.shape[0]
    assert cls.shape == (T, B, A, NETS[name][0] + 1) and bbox.shape == (T, B, A, 4)
    assert cls.dtype == torch.float32 and torch.equal(anchors, r.anchors)
    for t in range(T):
        assert torch.equal(cls[t], r.cls[t]) and torch.equal(bbox[t], r.bbox[t]), t
    assert torch.equal(cls[-1], cls_last) and torch.equal(bbox[-1], bbox_last)
    got, want = leaves(state), leaves(r.state)
    assert len(got) == len(want) > 0 and all(torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("name,B", CASES)
def test_detections_equal_the_predict_loop(runs, name, B):
    """predict_sequence(X)[0][t] filtered to class >= 0 is what predict returns for frame t: rows, row order, values."""
    r = runs(name, B)
    dets, _ = r.model.predict_sequence(r.X)
    assert dets.shape == (T, B, r.anchors.shape[0], 6)
    if name == "executor":   # the loop detects something (the freshly initialised spiking net leaves every anchor background)
        assert sum(d.shape[0] for per in r.dets for d in per) > 0
    for t in range(T):
        for b in range(B):
            got = dets[t, b][dets[t, b][:, 0] >= 0]
            assert torch.equal(got, r.dets[t][b]), (t, b)
    assert float(dets[..., 2:].min()) >= 0.0 and float(dets[..., 2:].max()) <= 1.0
    if B == 1:      # ... and predict itself, called frame by frame
        state = None
        with torch.no_grad():
            for t in range(T):
                det, state = r.model.predict(r.X[t, 0], state)
                assert torch.equal(det, r.dets[t][0]), t


@pytest.mark.parametrize("name,B", CASES)
def test_two_windows_with_the_state_handed_across_equal_one(runs, name, B):
    r = runs(name, B)
    whole, state_whole = r.model.predict_sequence(r.X)
    first, state = r.model.predict_sequence(r.X[:3])
    second, state = r.model.predict_sequence(r.X[3:], state)
    assert torch.equal(torch.cat([first, second]), whole)
    got, want = leaves(state), leaves(state_whole)
    assert len(got) == len(want) > 0 and all(torch.equal(g, w) for g, w in zip(got, want))


def test_skip_blanks_the_first_steps_only(runs):
    r = runs("executor", 2)     # (it detects from the first step on)
    whole, _ = r.model.predict_sequence(r.X)
    skipped, _ = r.model.predict_sequence(r.X, skip=2)
    assert bool((skipped[:2, ..., 0] == -1).all()) and bool((whole[:2, ..., 0] >= 0).any())
    assert torch.equal(skipped[2:], whole[2:])
    assert torch.equal(skipped[:2, ..., 1:], whole[:2, ..., 1:])


def test_training_mode_raises(runs):
    r = runs("tinyyolo", 1)
    r.model.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            r.model.predict_sequence(r.X)
    finally:
        r.model.eval()


@pytest.mark.parametrize("name", list(NETS))
def test_one_stream_without_the_batch_dimension(runs, name):
    r = runs(name, 1)
    a, _ = r.model.predict_sequence(r.X[:, 0])
    b, _ = r.model.predict_sequence(r.X)
    assert a.shape == (T, r.anchors.shape[0], 6) and torch.equal(a, b[:, 0])
