"""``SODa(carry_state=True)``: truncated BPTT over consecutive windows - the detached detector state of one step is the
initial state of the next, ``first`` puts single samples back to rest on the device.

The smallest TinyYolo of tests/test_gpu_seq_model.py (``T = 6, B = 2, 32 x 48``, two classes): one clip of 12 steps cut into
the windows ``[0:6]`` and ``[6:12]``.  The oracle runs frame by frame over window 1, detaches its state tree, runs window 2
from it and forms the loss as ``_oracle_loss`` does; functions and tolerances are those of that file (loss within 1e-4
relative, every parameter gradient within 1e-3, BatchNorm running statistics within 1e-5) - none of its own.
"""
import pytest
import torch

from tests.test_gpu_seq_model import B, H, T, TWO_STEPS, W, _compare_grads, _labels6, _oracle_loss
from tests.util import make_pair, rel_err, synthetic_events, synthetic_labels

pytestmark = pytest.mark.gpu

K = 2


@pytest.fixture(scope="module")
def S(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import snn_for_object_detection_amd as pkg
    return pkg


def _detached(tree):
    if isinstance(tree, torch.Tensor):
        return tree.detach()
    if isinstance(tree, tuple) and hasattr(tree, "_fields"):
        return type(tree)(*(_detached(t) for t in tree))
    if isinstance(tree, (list, tuple)):
        return type(tree)(_detached(t) for t in tree)
    return tree


class Clip:
    """The 12-step clip, its two windows with their labels, and the chained oracle step on window 2 (computed once)."""

    def __init__(self, S):
        self.X = synthetic_events(2 * T, B, H, W, p=0.08)
        self.w1, self.w2 = self.X[:T].cuda(), self.X[T:].cuda()
        self.lab1, self.lab2 = _labels6(TWO_STEPS, seed=3), _labels6(TWO_STEPS)
        self.ones = torch.ones(B, dtype=torch.int32).cuda()
        self.zeros = torch.zeros(B, dtype=torch.int32).cuda()
        self.product, oracle = make_pair(S.TinyYolo, num_classes=2, time_window=0, label_steps=K, carry_state=True)
        oracle.train()
        state = None
        with torch.no_grad():
            for frame in self.X[:T]:
                _, state = oracle._forward_impl(frame, state)
        carried = _detached(state)
        plain = oracle._forward_impl
        oracle._forward_impl = lambda frame, st: plain(frame, carried if st is None else st)
        try:
            loss, steps = _oracle_loss(oracle, self.X[T:], self.lab2, K, 0)
        finally:
            del oracle._forward_impl
        assert steps.tolist() == [[2, 5], [5, -1]]
        loss.backward()
        self.oracle, self.loss_ref = oracle, loss.detach()

    def model(self, S, **kw):
        """A fresh product model with the weights of ``self.product`` (same seed, same description)."""
        torch.manual_seed(2)
        args = dict(num_classes=2, time_window=0, label_steps=K, carry_state=True)
        args.update(kw)
        return S.TinyYolo(**args).cuda().train()


@pytest.fixture(scope="module")
def clip(S):
    return Clip(S)


def _preds_of(model):
    """Record the ``(cls_preds, bbox_preds)`` of every ``_forward_impl`` call, in order -> (list, undo)."""
    seen, plain = [], model._forward_impl

    def impl(*args, **kw):
        preds, state = plain(*args, **kw)
        seen.append((preds[1].detach().clone(), preds[2].detach().clone()))
        return preds, state
    model._forward_impl = impl
    return seen, lambda: delattr(model, "_forward_impl")


@pytest.fixture(scope="module")
def eval_chain(S, clip):
    """Eval mode, five-column labels (last-frame predictions): two chained validation steps, the per-sample reset, the
    12-step pass and the stateless pass of window 2 - each run once."""
    torch.manual_seed(2)
    model = S.TinyYolo(num_classes=2, time_window=0, carry_state=True).cuda().train()
    with torch.no_grad():
        model(clip.X.cuda())                                # warm the running statistics
    model.eval()
    lab = synthetic_labels(B).cuda()
    seen, undo = _preds_of(model)
    try:
        with torch.no_grad():
            model.validation_step((clip.w1, lab, clip.ones))
            model.validation_step((clip.w2, lab, clip.zeros))
            model.reset_carried_state()
            model.validation_step((clip.w1, lab, clip.ones))
            model.validation_step((clip.w2, lab, torch.tensor([0, 1], dtype=torch.int32).cuda()))
            model(clip.X.cuda())
            model(clip.w2)
    finally:
        undo()
    assert len(seen) == 6
    return dict(chained=seen[1], mixed=seen[3], whole=seen[4], stateless=seen[5])


def test_two_validation_steps_equal_one_pass_over_both_windows(eval_chain):
    for got, want in zip(eval_chain["chained"], eval_chain["whole"]):
        assert got.shape == want.shape and torch.equal(got, want)
    assert not torch.equal(eval_chain["chained"][0], eval_chain["stateless"][0])     # (the state matters on this clip)


def test_first_resets_one_sample_and_leaves_the_other_chained(eval_chain):
    for got, chained, stateless in zip(eval_chain["mixed"], eval_chain["chained"], eval_chain["stateless"]):
        assert torch.equal(got[0], chained[0])              # sample 0 went on
        assert torch.equal(got[1], stateless[1])            # sample 1 started from rest
        assert not torch.equal(got[1], chained[1])


@pytest.fixture(scope="module")
def second_step(S, clip):
    """Two training steps of the product on the two windows, ``zero_grad`` in between -> loss of the second step."""
    product = clip.product.train()
    loss1 = product.training_step((clip.w1, clip.lab1.cuda(), clip.ones))
    loss1.backward()
    product.zero_grad()
    loss2 = product.training_step((clip.w2, clip.lab2.cuda(), clip.zeros))
    loss2.backward()
    return loss2.detach()


def test_truncated_gradient_of_the_second_window_matches_the_oracle(S, clip, second_step):
    product, oracle, loss_ref = clip.product, clip.oracle, clip.loss_ref
    print(f"chained loss {second_step.item()!r} oracle {loss_ref.item()!r}")
    assert abs(second_step.item() - loss_ref.item()) <= 1e-4 * abs(loss_ref.item())
    _compare_grads(product, {n: p.grad for n, p in oracle.named_parameters()})
    bn_p, bn_r = product.base_net.net.net[0][1], oracle.base_net.net.net[0][1]
    assert rel_err(bn_p.running_mean, bn_r.running_mean) < 1e-5
    assert rel_err(bn_p.running_var, bn_r.running_var) < 1e-5
    assert int(bn_p.num_batches_tracked) == 2 * T
    # a silently dropped state would give the stateless step on window 2
    stateless = clip.model(S, carry_state=False).training_step((clip.w2, clip.lab2.cuda()))
    print(f"stateless loss {stateless.item()!r}")
    assert stateless.item() != second_step.item()
    assert abs(stateless.item() - loss_ref.item()) > 1e-4 * abs(loss_ref.item())
    # what is kept is detached: no gradient crosses the window boundary, nothing holds the step's graph
    key, kept = product._carried["train"]
    assert key == (B, H, W)
    leaves = []

    def walk(t):
        if isinstance(t, torch.Tensor):
            leaves.append(t)
        elif isinstance(t, (list, tuple)):
            for k in t:
                walk(k)
    walk(kept)
    assert leaves and all(t.grad_fn is None and not t.requires_grad and t.dtype == torch.float32 for t in leaves)
    assert "_carried" not in product.state_dict() and not any("carried" in k for k in product.state_dict())


def test_a_window_without_labels_still_advances_the_state(S, clip):
    model = clip.model(S)
    empty = torch.full((B, 3, 6), -1.0).cuda()
    loss1 = model.training_step((clip.w1, empty, clip.ones))
    loss1.backward()
    assert float(loss1.detach()) == 0.0
    model.zero_grad()
    loss2 = model.training_step((clip.w2, clip.lab2.cuda(), clip.zeros))
    print(f"after an empty window {loss2.item()!r} oracle {clip.loss_ref.item()!r}")
    assert abs(loss2.item() - clip.loss_ref.item()) <= 1e-4 * abs(clip.loss_ref.item())


def test_memory_does_not_grow_from_step_to_step(S, clip):
    HF = S.functional
    model = clip.model(S)
    batches = [(clip.w1, clip.lab1.cuda(), clip.ones), (clip.w2, clip.lab2.cuda(), clip.zeros)]
    held = []
    for n in range(4):
        loss = model.training_step(batches[n % 2])
        loss.backward()
        model.zero_grad()
        del loss
        HF.wgrad_stream_sync()
        torch.cuda.synchronize()
        held.append(torch.cuda.memory_allocated())
    print(f"allocated after each step {held}")
    assert held[3] == held[2]


def test_validation_between_training_steps_and_the_reset_of_the_kept_state(S, clip, second_step):
    model = clip.model(S)
    lab1, lab2 = clip.lab1.cuda(), clip.lab2.cuda()
    model.training_step((clip.w1, lab1, clip.ones))
    model.eval()
    with torch.no_grad():
        model.validation_step((clip.w2, lab2, clip.ones))
        model.validation_step((clip.w1, lab1))
    model.train()
    loss = model.training_step((clip.w2, lab2, clip.zeros)).detach()
    assert set(model._carried) == {"train", "val"}
    assert torch.equal(loss, second_step)                   # the validation stream did not disturb the training stream
    # a two-element batch means "no slot restarted"
    model.reset_carried_state()
    model.training_step((clip.w1, lab1))
    assert torch.equal(model.training_step((clip.w2, lab2)).detach(), second_step)
    # reset_carried_state() = the step with first all ones = the stateless step
    model.reset_carried_state("train")
    after_reset = model.training_step((clip.w2, lab2, clip.zeros)).detach()
    marked = model.training_step((clip.w2, lab2, clip.ones)).detach()
    assert torch.equal(after_reset, marked) and not torch.equal(marked, second_step)
    # another batch size drops the kept state: the step starts from rest instead of failing on the shapes
    one = model.training_step((clip.w2[:, :1], lab2[:1], clip.zeros[:1])).detach()
    assert bool(torch.isfinite(one)) and model._carried["train"][0] == (1, H, W)


def test_without_the_keyword_the_step_is_the_one_it_was(S, clip):
    model = clip.model(S, carry_state=False)
    batch = (clip.w2, clip.lab2.cuda())

    def step(fn):
        model.zero_grad()
        loss = fn(batch)
        loss.backward()
        S.functional.wgrad_stream_sync()
        return loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    loss_a, grads_a = step(model.training_step)
    model.reset_carried_state()
    loss_b, grads_b = step(model.training_step)
    loss_c, grads_c = step(model._step)
    assert model._carried == {}
    assert torch.equal(loss_a, loss_b) and torch.equal(loss_a, loss_c)
    assert grads_a.keys() == grads_b.keys() == grads_c.keys() and grads_a
    for n in grads_a:
        assert torch.equal(grads_a[n], grads_b[n]) and torch.equal(grads_a[n], grads_c[n]), n


def test_bf16_storage_chained_step_within_the_modes_tolerance(S, clip):
    """One chained training step in bf16 storage against the fp32 chained oracle, held to the mode's own tolerance (6 % of
    the loss, tests/test_gpu_bf16_storage.py); the carried tensors stay fp32."""
    HF = S.functional
    model = clip.model(S)
    HF.set_activation_storage("bf16")
    try:
        model.training_step((clip.w1, clip.lab1.cuda(), clip.ones)).backward()
        model.zero_grad()
        loss = model.training_step((clip.w2, clip.lab2.cuda(), clip.zeros))
        loss.backward()
    finally:
        HF.set_activation_storage("fp32")
    print(f"bf16 storage: chained loss {loss.item()!r} oracle {clip.loss_ref.item()!r}")
    assert loss.dtype == torch.float32 and bool(torch.isfinite(loss))
    assert abs(loss.item() - clip.loss_ref.item()) <= 0.06 * abs(clip.loss_ref.item())
    for p in model.parameters():
        assert p.grad is None or (p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()))


def test_the_reset_of_the_kept_state_does_not_synchronise(S, clip):
    """What the carried step adds to a step - the reset of the kept tree by ``first`` and the detaching of the new one -
    under ``set_sync_debug_mode("error")``: ``first`` is read on the device, the table goes up out of pinned memory."""
    HF = S.functional
    model = clip.model(S)
    lab1 = clip.lab1.cuda()
    mixed = torch.tensor([0, 1], dtype=torch.int32).cuda()
    model.training_step((clip.w1, lab1, clip.ones))
    kept = model._carried["train"][1]
    HF.reset_state_(kept, clip.zeros)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            lab1.sum().item()                # the mode is live: a host read of a device value raises
        for _ in range(6):                   # (more calls than there are pinned staging tables)
            tree = HF.detach_state(HF.reset_state_(kept, mixed))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    v = tree[0][0][2].v                      # the first Norm -> LIF layer of the backbone
    assert not v[1].any() and bool(v[0].any())


def test_chained_feed_batches_drive_the_carried_training_step(S, tmp_path):
    """``PropheseeFeed(chained=True)`` -> ``(X, labels[B, N, 6], first)`` on the device -> ``training_step``: ``first``
    and the frames are those of the host samples of a twin feed (the slot's augmentation row through ``aug_table=``), and
    a few chained steps train."""
    import numpy as np
    from tests import event_aug_ref as R
    from tests import recordings_ref as RR
    d = tmp_path / "gen1" / "train"
    d.mkdir(parents=True)
    for i, ms in enumerate((40, 24, 56, 32)):
        ev = RR.stream(np.random.default_rng(300 + i), 304, 240, ms * 1000, per_ms=40)
        S.write_dat(str(d / f"rec_{i:02d}_td.dat"), S.pack_events(*ev), 304, 240)
        np.save(str(d / f"rec_{i:02d}_bbox.npy"), RR.walk_boxes(2000, 304, 240, steps=(1, 5, 9, 11), small=()))
    Bf, Tf = 3, 4
    kw = dict(dataset="gen1", split="train", batch_size=Bf, num_steps=Tf, time_step=2, one_label=False, chained=True, seed=1)
    aug = dict(hflip=0.5, zoom=(0.8, 1.25), seed=4)
    feed = S.PropheseeFeed(str(tmp_path), augment=S.EventAugment(**aug), **kw)
    twin = S.PropheseeFeed(str(tmp_path), augment=S.EventAugment(**aug), **kw).samples()
    model = S.TinyYolo(num_classes=2, time_window=0, label_steps=2, carry_state=True).cuda().train()
    marks = 0
    for n in range(6):
        X, labels, first = next(feed)
        host = [next(twin) for _ in range(Bf)]
        assert tuple(X.shape) == (Tf, Bf, 2, 240, 304) and labels.dim() == 3 and labels.shape[0] == Bf and labels.shape[2] == 6
        assert first.is_cuda and first.dtype == torch.int32 and first.tolist() == [s[3] for s in host]
        assert n > 0 or first.tolist() == [1] * Bf
        marks += int(first.sum())
        table = torch.stack([s[4] for s in host])
        assert torch.equal(feed._batcher.last_aug_table, table)
        want = R.frames_ref([(*S.unpack_events(s[0]), s[1]) for s in host], table.numpy(), Tf, Bf, 240, 304, 2000)
        assert np.array_equal(X.cpu().numpy().astype(np.uint8), want.astype(np.uint8))
        loss = model.training_step((X, labels, first))
        loss.backward()
        model.zero_grad()
        assert bool(torch.isfinite(loss))
    assert marks > Bf                                          # recordings ended and slots moved on during the run


OPTIONS = {
    "tal_focal_giou": dict(assigner="tal", cls_loss="focal", box_loss="giou"),
    "iou_ciou": dict(box_loss="ciou", box_loss_weight=2.0),
    "lif_gradient": {},
    "learnable_tau": {},
    "activity": {},
}


@pytest.mark.parametrize("name", list(OPTIONS))
def test_the_options_of_the_step_keep_working_on_a_carried_state(S, clip, name):
    """Assigners, the selectable loss, ``set_lif_gradient``, learnable time constants and ``activity.record`` on a chained
    step: finite loss and gradients, and a loss that the carried state moved away from the stateless one."""
    from snn_for_object_detection_amd import activity
    HF = S.functional
    model = clip.model(S, **OPTIONS[name])
    if name == "lif_gradient":
        assert HF.set_lif_gradient(model, surrogate="triangle", detach_reset=True) > 0
    if name == "learnable_tau":
        assert HF.set_lif_time_constants(model, learn_tau="channel") > 0
    lab1, lab2 = clip.lab1.cuda(), clip.lab2.cuda()
    model.training_step((clip.w1, lab1, clip.ones)).backward()
    model.zero_grad()
    if name == "activity":
        with activity.record(model) as rec:
            loss = model.training_step((clip.w2, lab2, clip.zeros))
        assert rec.report()
    else:
        loss = model.training_step((clip.w2, lab2, clip.zeros))
    loss.backward()
    HF.wgrad_stream_sync()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert bool(torch.isfinite(loss)) and grads and all(bool(torch.isfinite(g).all()) for g in grads)
    if name == "learnable_tau":
        taus = [p.grad for n, p in model.named_parameters() if n.endswith(("w_mem", "w_syn"))]
        assert taus and all(g is not None and bool(g.any()) for g in taus)
    stateless = model.training_step((clip.w2, lab2, clip.ones)).detach()
    assert not torch.equal(stateless, loss.detach())
