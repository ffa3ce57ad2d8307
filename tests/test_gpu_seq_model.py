"""``SODa(label_steps=K)``: the training / validation step on six-column labels ``(ts, class, x1, y1, x2, y2)`` against
the CPU oracle run frame by frame with the restatement of tests/seq_targets_ref.py applied to every labelled frame.

TinyYolo, T = 6, B = 2, 32 x 48, two classes.  Tolerances are those of tests/test_gpu_model.py::_train_step_vs_oracle:
loss within 1e-4 relative, every parameter gradient within 1e-3 (L2, relative), BatchNorm running statistics within 1e-5.
"""
import pytest
import torch
from torch.nn import functional as F

from tests import seq_targets_ref as SR
from tests.util import make_pair, rel_err, synthetic_events, synthetic_labels

pytestmark = pytest.mark.gpu

T, B, H, W = 6, 2, 32, 48


@pytest.fixture(scope="module")
def S(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import snn_for_object_detection_amd as pkg
    return pkg


def _labels6(ts_plan, seed=1):
    """``ts_plan[b]``: the timestep of each row of sample ``b``, None for a padding row."""
    n = len(ts_plan[0])
    boxes = synthetic_labels(B, n_boxes=n, seed=seed)
    out = torch.full((B, n, 6), -1.0)
    for b, plan in enumerate(ts_plan):
        for j, ts in enumerate(plan):
            if ts is not None:
                out[b, j, 0] = float(ts)
                out[b, j, 1:] = boxes[b, j]
    return out


# sample 0 has rows on the steps 2 and 5, sample 1 rows on step 5 only and one padding row
TWO_STEPS = [[2, 5, 5], [5, 5, None]]


def _oracle_loss(oracle, X, labels6, K, t0):
    """The oracle frame by frame over the cut sequence, every step's predictions kept; the restatement chooses the slots
    and assigns the anchors, and the loss formula runs in torch autograd over the rows of the valid slots."""
    X = X[t0:]
    state, cls, box = None, [], []
    for frame in X:
        (anchors, c, b), state = oracle._forward_impl(frame, state)
        cls.append(c)
        box.append(b)
    steps = SR.select_steps_ref(labels6, X.shape[0], K, t0)
    roi = SR.roi_steps_ref(anchors.detach(), labels6, steps, t0, oracle.iou_threshold)
    slots = [(k, b) for k in range(K) for b in range(labels6.shape[0]) if steps[k, b] >= 0]
    if not slots:
        return None, steps
    c_sel = torch.stack([cls[int(steps[k, b])][b] for k, b in slots])            # [V, A, C + 1]
    b_sel = torch.stack([box[int(steps[k, b])][b] for k, b in slots])
    off, mask, lab = (torch.stack([t[k, b] for k, b in slots]) for t in (roi.offsets, roi.masks, roi.classes))
    ce = F.cross_entropy(c_sel.reshape(-1, c_sel.shape[-1]), lab.reshape(-1), reduction="none")
    pos = lab.reshape(-1) > 0
    r = oracle.loss_ratio
    loss = ce[pos].mean() * r + ce[~pos].mean() * (1 - r) + (b_sel * mask - off * mask).abs().mean()
    # ... which is the restatement's closed form on the same predictions
    logits = torch.zeros(K, labels6.shape[0], *c_sel.shape[1:])
    boxes = torch.zeros(K, labels6.shape[0], *b_sel.shape[1:])
    for v, (k, b) in enumerate(slots):
        logits[k, b], boxes[k, b] = c_sel[v].detach(), b_sel[v].detach()
    closed = SR.loss_steps_ref(logits, boxes, roi.offsets, roi.masks, roi.classes, steps, r)
    assert closed.V == len(slots) and abs(float(loss.detach()) - closed.loss) <= 1e-5 * abs(closed.loss)
    return loss, steps


def _compare_grads(product, ref_grads):
    worst = 0.0
    for name, p in product.named_parameters():
        if not p.requires_grad:
            continue
        g_ref = ref_grads[name]
        assert p.grad is not None and g_ref is not None, name
        if g_ref.norm() > 1e-8:
            worst = max(worst, rel_err(p.grad, g_ref))
    assert worst < 1e-3, worst


def _train_step_vs_oracle(S, labels6, K, time_window=0, draw_seed=None, expect_steps=None, model_cls=None):
    product, oracle = make_pair(model_cls or S.TinyYolo, num_classes=2, time_window=time_window, label_steps=K)
    X = synthetic_events(T, B, H, W, p=0.08)
    product.train()
    oracle.train()
    t0 = 0
    if draw_seed is not None:
        torch.manual_seed(draw_seed)
        t0 = int(oracle._rand_start_time())
    loss_ref, steps = _oracle_loss(oracle, X, labels6, K, t0)
    if expect_steps is not None:
        assert steps.tolist() == expect_steps
    loss_ref.backward()
    if draw_seed is not None:
        torch.manual_seed(draw_seed)
    loss = product.training_step((X.cuda(), labels6.cuda()))
    loss.backward()
    print(f"t0 {t0} loss {loss.item()!r} oracle {loss_ref.item()!r}")
    assert abs(loss.item() - loss_ref.item()) <= 1e-4 * abs(loss_ref.item())
    _compare_grads(product, {n: p.grad for n, p in oracle.named_parameters()})
    bn_p, bn_r = product.base_net.net.net[0][1], oracle.base_net.net.net[0][1]
    assert rel_err(bn_p.running_mean, bn_r.running_mean) < 1e-5
    assert rel_err(bn_p.running_var, bn_r.running_var) < 1e-5
    assert int(bn_p.num_batches_tracked) == T - t0
    return t0


def test_train_step_on_every_labelled_frame_matches_the_oracle(S):
    _train_step_vs_oracle(S, _labels6(TWO_STEPS), 2, expect_steps=[[2, 5], [5, -1]])


def test_train_step_with_a_random_prefix_shifts_labels_and_frames_alike(S):
    """``time_window=3``: the seeded draw drops two frames, so the rows of the steps 2 and 5 supervise the steps 0 and 3 of
    the four frames that are left."""
    t0 = _train_step_vs_oracle(S, _labels6(TWO_STEPS), 2, time_window=3, draw_seed=0, expect_steps=[[0, 3], [3, -1]])
    assert t0 == 2


def _net_with_batchnorm_in_the_box_net(L):
    """A small non-spiking detector whose box prediction net holds a BatchNorm: it must see every timestep (running
    statistics), so the labelled frames are gathered BEHIND the prediction nets, not in front of them."""
    class Net(L.SODa):
        def backbone_cfgs(self):
            return [L.Conv(8, 3, 2), L.Norm(), L.ReLU(), L.Conv(16, 3, 2), L.Norm(), L.ReLU()]

        def neck_cfgs(self):
            return [L.Conv(16, 3, 2), L.Norm(), L.Tanh(), L.Return()]

        def head_cfgs(self, box_out, cls_out):
            return [[L.Conv(kernel_size=1), L.Norm(), L.Tanh()],
                    [L.Conv(12, 1), L.Norm(), L.Tanh(), L.Conv(box_out, 1)], [L.Conv(cls_out, 1)]]
    return Net


def test_prediction_nets_that_need_every_step_are_gathered_behind(S):
    from snn_for_object_detection_amd import generator as G
    Net = _net_with_batchnorm_in_the_box_net(S)
    probe = Net(num_classes=2, time_window=0, label_steps=2)
    assert any(G._has_state(m) for m in probe.head_net.model_0.box_net.modules())       # the branch under test is taken
    _train_step_vs_oracle(S, _labels6(TWO_STEPS), 2, expect_steps=[[2, 5], [5, -1]], model_cls=Net)
    # the BatchNorm inside the box net took one update per timestep of the sequence, not one per labelled frame
    product, _ = make_pair(Net, num_classes=2, time_window=0, label_steps=2)
    product.train()
    product.training_step((synthetic_events(T, B, H, W, p=0.08).cuda(), _labels6(TWO_STEPS).cuda()))
    bns = [m for m in product.head_net.model_0.box_net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 1 and int(bns[0].num_batches_tracked) == T


def test_bf16_storage_reads_the_labelled_frames_out_in_fp32(S):
    """bf16-storage mode: the head read-out of every step is converted to fp32 before the gather, the prediction nets and
    the loss run in fp32.  Held to the mode's own tolerance against the fp32 oracle (6 % of the loss,
    tests/test_gpu_bf16_storage.py::test_bf16_storage_training_step_tolerance_and_dtypes), for the labelled-frames step
    against the oracle and for one slot on the last step against the single-label step in the same mode."""
    HF = S.functional
    product, oracle = make_pair(S.TinyYolo, num_classes=2, time_window=0, label_steps=2)
    X, labels6 = synthetic_events(T, B, H, W, p=0.08), _labels6(TWO_STEPS)
    product.train()
    oracle.train()
    loss_ref, _ = _oracle_loss(oracle, X, labels6, 2, 0)
    seen = []
    hook = product.head_net.model_0.box_net.register_forward_hook(lambda m, i, o: seen.append((i[0].dtype, i[0].shape[0])))
    HF.set_activation_storage("bf16")
    try:
        loss = product.training_step((X.cuda(), labels6.cuda()))
        loss.backward()
        last6 = _labels6([[T - 1] * 3, [T - 1, T - 1, None]])
        torch.manual_seed(2)
        single = S.TinyYolo(num_classes=2, time_window=0).cuda().train()
        torch.manual_seed(2)
        multi = S.TinyYolo(num_classes=2, time_window=0, label_steps=1).cuda().train()
        loss_1 = single.training_step((X.cuda(), last6[:, :, 1:].contiguous().cuda()))
        loss_m = multi.training_step((X.cuda(), last6.cuda()))
    finally:
        HF.set_activation_storage("fp32")
        hook.remove()
    assert seen == [(torch.float32, 2)]                 # the box net saw the K = 2 gathered frames per sample, in fp32
    print(f"bf16 storage: loss {loss.item()!r} oracle {loss_ref.item()!r}; one slot {loss_m.item()!r} single-label "
          f"{loss_1.item()!r}")
    assert loss.dtype == torch.float32 and bool(torch.isfinite(loss))
    assert abs(loss.item() - loss_ref.item()) <= 0.06 * abs(loss_ref.item())
    for p in product.parameters():
        assert p.grad is None or (p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()))
    assert product.base_net.net.net[0][0].weight.grad is not None
    assert abs(loss_m.item() - loss_1.item()) <= 0.06 * abs(loss_1.item())


def test_one_slot_on_the_last_step_is_the_single_label_step(S):
    """All rows on step T - 1 and ``label_steps=1`` against today's ``training_step`` on the five-column labels: the two
    paths differ only in the head scans writing every step."""
    labels6 = _labels6([[T - 1] * 3, [T - 1, T - 1, None]])
    X = synthetic_events(T, B, H, W, p=0.08).cuda()
    torch.manual_seed(2)
    single = S.TinyYolo(num_classes=2, time_window=0).cuda().train()
    torch.manual_seed(2)
    multi = S.TinyYolo(num_classes=2, time_window=0, label_steps=1).cuda().train()
    loss_ref = single.training_step((X, labels6[:, :, 1:].contiguous().cuda()))
    loss_ref.backward()
    loss = multi.training_step((X, labels6.cuda()))
    loss.backward()
    print(f"loss {loss.item()!r} single-label {loss_ref.item()!r}")
    assert abs(loss.item() - loss_ref.item()) <= 1e-4 * abs(loss_ref.item())
    _compare_grads(multi, {n: p.grad for n, p in single.named_parameters()})


def test_a_batch_without_labels_trains_on_a_zero_gradient(S):
    """All padding (``MTPropheseeDataset.parse_data`` yields such windows): loss 0.0, finite all-zero gradients, and a
    ``FlatTrainer`` step that is NOT skipped as non-finite - the parameters move by what Adamax does with the weight
    decay alone (fp64 ``torch.optim.Adamax`` on a zero gradient; bound of tests/test_gpu_trainer.py for that
    comparison)."""
    from snn_for_object_detection_amd.trainer import FlatTrainer
    lr, wd = 2e-3, 1e-2
    torch.manual_seed(2)
    model = S.TinyYolo(num_classes=2, time_window=0, label_steps=2).cuda().train()
    tr = FlatTrainer(model, lr=lr, skip_nonfinite=True, weight_decay=wd)
    p0 = torch.nn.Parameter(tr.flat_param[: tr.numel].detach().double().cpu())
    opt = torch.optim.Adamax([p0], lr=lr, weight_decay=wd)
    before = tr.flat_param[: tr.numel].clone()
    tr.zero_grad()
    loss = model.training_step((synthetic_events(T, B, H, W, p=0.08).cuda(), torch.full((B, 3, 6), -1.0).cuda()))
    loss.backward()
    tr.synchronize()
    assert float(loss.detach()) == 0.0
    for p, slot in zip(tr.params, tr.slots):       # every parameter received a gradient: in its slot of the flat buffer
        assert slot.written or p.grad is not None  # or, for an operator without slot support, through autograd
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()) and not p.grad.any()
    g = tr.flat_grad[: tr.numel]
    assert bool(torch.isfinite(g).all()) and not g.any()
    p0.grad = torch.zeros_like(p0)
    opt.step()
    tr.step()
    assert tr.skipped_steps == 0
    assert float(tr.last_grad_norm) == 0.0
    after = tr.flat_param[: tr.numel]
    assert not torch.equal(after, before)                                   # the weight decay moved them
    assert rel_err(after, p0) < 1e-5


def test_validation_feeds_map_with_exactly_the_valid_slots(S):
    """``validation_step`` on six-column labels logs ``val_loss`` and updates the mAP state with one image per valid slot:
    the records equal those of ``predict_sequence``'s padded detections of the same frames with the label rows of the
    frame's own timestep; an empty slot leaves no detection and no ground truth behind."""
    from snn_for_object_detection_amd.metrics import MeanAveragePrecision
    K = 2
    labels6 = _labels6(TWO_STEPS)
    X = synthetic_events(T, B, H, W, p=0.1, seed=3).cuda()
    torch.manual_seed(2)
    model = S.TinyYolo(num_classes=2, time_window=0, label_steps=K).cuda().train()
    with torch.no_grad():
        model(X)                                            # warm the running statistics
    model.eval()
    loss = model.validation_step((X, labels6.cuda()))
    assert "val_loss" in model.logged and float(model.logged["val_loss"]) == float(loss.detach()) and bool(torch.isfinite(loss))
    steps = SR.select_steps_ref(labels6, T, K)
    assert steps.tolist() == [[2, 5], [5, -1]]
    dets_seq, _ = model.predict_sequence(X)
    slots = [(k, b) for k in range(K) for b in range(B) if steps[k, b] >= 0]
    dets = torch.stack([dets_seq[int(steps[k, b]), b] for k, b in slots])
    rows = torch.full((len(slots), labels6.shape[1], 5), -1.0)
    for v, (k, b) in enumerate(slots):
        for j, r in enumerate(labels6[b]):
            if SR.row_step(r, 0, T) == int(steps[k, b]):
                rows[v, j] = r[1:]
    assert int((rows[:, :, 0] >= 0).sum()) == 5
    hand = MeanAveragePrecision(2)
    hand.update_padded(dets, rows.cuda())
    got = model.map_metric
    assert len(got._scores) == 1 and len(hand._scores) == 1
    valid = (steps >= 0).reshape(-1)
    sc, mk = got._scores[0].cpu(), got._masks[0].cpu()
    assert sc.shape[0] == K * B
    assert torch.equal(sc[valid], hand._scores[0].cpu()) and torch.equal(mk[valid], hand._masks[0].cpu())
    assert bool(torch.isinf(sc[~valid]).all()) and bool((sc[~valid] < 0).all()) and not mk[~valid].any()
    assert torch.equal(got._npig.cpu(), hand._npig.cpu()) and int(got._npig.sum()) == 5
    a, b = got.compute(), hand.compute()
    for key in ("map", "map_50", "mar_1", "mar_10", "mar_100"):
        assert torch.equal(torch.as_tensor(a[key]).cpu(), torch.as_tensor(b[key]).cpu()), key
