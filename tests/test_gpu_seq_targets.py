"""The kernels behind training on every labelled timestep (csrc/targets.hip: snn_label_steps, snn_gather_steps_fwd / _bwd,
snn_roi_assign_steps; csrc/det_loss.hip: snn_det_loss_steps_fwd / _bwd) against the CPU restatement of tests/seq_targets_ref.py.

Every entry point is called through the C ABI on buffers pre-filled with NaN (0x7F bytes for integer buffers) with a
guard region behind them, and through the Python wrappers (``functional.select_label_steps`` / ``gather_steps`` /
``detection_loss_steps``, ``RoI.steps``), which must return the same bits.  Selection, gather and the integer side of the
assignment are exact; the offsets' logarithm columns and the loss are held to the bounds ``check_roi`` / ``check_loss``
of tests/test_gpu_targets_fp64.py derive."""
import pytest
import torch

from tests import seq_targets_ref as SR
from tests import targets_ref as TR
from tests.test_gpu_targets_fp64 import Guarded, check_loss, check_roi, run_roi_abi

pytestmark = pytest.mark.gpu

PAD = [-1.0] * 6


@pytest.fixture(scope="module")
def hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from snn_for_object_detection_amd import _hip
    return _hip


def _st():
    return torch.cuda.current_stream().cuda_stream


def _i32(steps):
    return steps.to(torch.int32).cuda().contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ====================================================================================================== selection
def _row(ts, cls=0.0):
    return [float(ts), cls, 0.25, 0.25, 0.5, 0.5]


# sample 0: duplicate rows on step 1 (which t0 = 2 cuts away), step 4, and ts = 9 >= T on both cuts
# sample 1: four distinct steps, more than any K here; sample 2: padding rows only
SELECT_LABELS = torch.tensor([[_row(1), _row(1, 1.0), _row(4), _row(9), PAD],
                              [_row(0), _row(2), _row(3), _row(5), _row(3, 1.0)],
                              [PAD, PAD, PAD, PAD, PAD]])


@pytest.mark.parametrize("t0", [0, 2])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_label_steps_equal_the_restatement(hip, K, t0):
    from snn_for_object_detection_amd import functional as HF
    B, N, T = 3, 5, 6
    ref = SR.select_steps_ref(SELECT_LABELS, T, K, t0)
    if K == 3:
        assert ref.tolist() == ([[1, 2, -1], [4, 3, -1], [-1, 5, -1]] if t0 == 0 else [[2, 0, -1], [-1, 1, -1], [-1, 3, -1]])
    lab = SELECT_LABELS.cuda().contiguous()
    out = Guarded(K * B * 4, torch.uint8)
    hip.call("snn_label_steps", lab.data_ptr(), B, N, T, K, t0, out.ptr, _st())
    torch.cuda.synchronize()
    assert out.guard_intact()
    assert torch.equal(out.out(K * B * 4).view(torch.int32).reshape(K, B), ref)
    steps = HF.select_label_steps(lab, T, K, t0)
    assert steps.dtype == torch.int32 and steps.shape == (K, B) and torch.equal(steps.cpu(), ref)


# ====================================================================================================== gather
def _gather_ref(src, steps):
    """``src[T, B, M, C]``, ``steps[K, B]`` -> ``[K, B, M, C]``."""
    K, B = steps.shape
    out = torch.zeros(K, B, *src.shape[2:])
    for k in range(K):
        for b in range(B):
            if steps[k, b] >= 0:
                out[k, b] = src[steps[k, b], b]
    return out


def _scatter_ref(g, steps, T):
    """``g[K, B, M, C]`` -> ``[T, B, M, C]``: two addends at most per element, so the fp32 sum is exact."""
    K, B = steps.shape
    out = torch.zeros(T, B, *g.shape[2:])
    for k in range(K):
        for b in range(B):
            if steps[k, b] >= 0:
                out[steps[k, b], b] += g[k, b]
    return out


GATHER_CASES = [
    # id, T, B, M, C, ld, channel offset inside the ld-wide buffer, steps[K][B]
    ("C4_vector", 4, 2, 6, 4, 4, 0, [[0, 3], [2, -1]]),
    ("C6_scalar", 4, 2, 6, 6, 6, 0, [[1, -1], [3, 0]]),
    ("C4_in_8_vector", 4, 2, 6, 4, 8, 4, [[0, 3], [2, -1]]),
    ("C4_in_8_unaligned_scalar", 4, 2, 6, 4, 8, 2, [[0, 3], [2, -1]]),
    ("T1", 1, 2, 6, 4, 4, 0, [[0, -1]]),
    ("duplicate_step", 4, 2, 6, 4, 4, 0, [[1, 0], [1, 2]]),
    ("all_empty", 4, 2, 6, 4, 4, 0, [[-1, -1]]),
]


@pytest.mark.parametrize("cs", GATHER_CASES, ids=[c[0] for c in GATHER_CASES])
def test_gather_steps_copies_exactly_both_ways(hip, cs):
    from snn_for_object_detection_amd import functional as HF
    _, T, B, M, C, ld, off, steps = cs
    steps = torch.tensor(steps, dtype=torch.int32)
    K = steps.shape[0]
    g = torch.Generator().manual_seed(T * 100 + C + ld)
    src, grad = torch.randn(T, B, M, C, generator=g), torch.randn(K, B, M, C, generator=g)
    fwd_ref, bwd_ref = _gather_ref(src, steps), _scatter_ref(grad, steps, T)
    if cs[0] == "duplicate_step":
        assert torch.equal(bwd_ref[1, 0], grad[0, 0] + grad[1, 0])
    d_steps = _i32(steps)

    def wide(t):       # the tensor as the channels off .. off + C of a buffer ld channels wide; the others hold NaN
        buf = torch.full((*t.shape[:-1], ld), float("nan"))
        buf[..., off:off + C] = t
        return buf.cuda()

    # ---- forward through the ABI: ld-wide source, ld-wide guarded destination
    d_src = wide(src)
    dst = Guarded(K * B * M * ld, torch.float32)
    hip.call("snn_gather_steps_fwd", d_src.data_ptr() + 4 * off, ld, d_steps.data_ptr(), dst.ptr + 4 * off, ld, T, B, K, M,
             C, _st())
    torch.cuda.synchronize()
    assert dst.guard_intact()
    got = dst.out(K, B, M, ld)
    assert torch.equal(_bits(got[..., off:off + C]), _bits(fwd_ref))
    rest = torch.cat([got[..., :off], got[..., off + C:]], dim=-1)
    assert bool(torch.isnan(rest).all())                       # channels outside the slice are not written
    # ---- backward through the ABI: every frame of the slice is written, zeros where no slot selected it
    d_grad = wide(grad)
    gsrc = Guarded(T * B * M * ld, torch.float32)
    hip.call("snn_gather_steps_bwd", d_grad.data_ptr() + 4 * off, ld, d_steps.data_ptr(), gsrc.ptr + 4 * off, ld, T, B, K,
             M, C, _st())
    torch.cuda.synchronize()
    assert gsrc.guard_intact()
    got = gsrc.out(T, B, M, ld)
    assert torch.equal(got[..., off:off + C], bwd_ref)
    assert bool(((got[..., off:off + C] == 0) == (bwd_ref == 0)).all())
    rest = torch.cat([got[..., :off], got[..., off + C:]], dim=-1)
    assert bool(torch.isnan(rest).all())
    # ---- the autograd Function on the aliased channels-last view the executor produces
    H, W = 2, M // 2
    base = torch.zeros(T, B, H, W, ld, device="cuda")
    base[..., off:off + C] = src.cuda().reshape(T, B, H, W, C)
    base.requires_grad_()
    Y = base[..., off:off + C].permute(0, 1, 4, 2, 3)
    assert HF.cl_stride(Y) == ld or T * B * H * W == 1
    out = HF.gather_steps(Y, d_steps)
    assert out.shape == (K, B, C, H, W)
    assert torch.equal(out.detach().permute(0, 1, 3, 4, 2).reshape(K, B, M, C).cpu(), fwd_ref)
    out.backward(grad.cuda().reshape(K, B, H, W, C).permute(0, 1, 4, 2, 3))
    gb = base.grad.cpu().reshape(T, B, M, ld)
    assert torch.equal(gb[..., off:off + C], bwd_ref)
    assert not gb[..., :off].any() and not gb[..., off + C:].any()


# ====================================================================================================== assignment
THR = 0.5
# (id, t0, T of the cut sequence, timestep of every real row per sample; the remaining rows of the N = 5 are padding)
ROI_PLANS = [
    # one valid and one empty slot per sample.  Sample 0: four rows on step 2 and one the prefix cuts away (it takes no
    # part); sample 1: three rows on step 5 and two padding rows (which claim anchors); sample 2: three rows on step 0,
    # two beyond the sequence
    ("one_empty_slot_each", 1, 6, [[3, 3, 0, 3, 3], [6, 6, 6], [1, 9, 1, 9, 1]]),
    # two valid slots in samples 0 and 1: rows of the other labelled step take no part in either
    ("two_steps", 0, 6, [[2, 5, 2, 5], [0, 3, 3, 3, 0], [4, 4]]),
]
_ROI = {}


def _roi_case(name):
    """The case's inputs and its restatement, computed once and shared by the assignment and the loss tests."""
    if name not in _ROI:
        _, t0, T, plan = next(p for p in ROI_PLANS if p[0] == name)
        anchors = SR.grid_anchors(4, 4, 9)
        labels6 = SR.labels6_from(anchors, plan, 5)
        steps = SR.select_steps_ref(labels6, T, 2, t0)
        _ROI[name] = (anchors, labels6, steps, t0, SR.roi_steps_ref(anchors, labels6, steps, t0, THR))
    return _ROI[name]


def run_roi_steps_abi(hip, anchors, labels6, steps, t0, thr):
    anchors, labels6, d_steps = anchors.cuda().contiguous(), labels6.cuda().contiguous(), _i32(steps)
    B, N, _ = labels6.shape
    K, A = steps.shape[0], anchors.shape[0]
    ws = Guarded(hip.query("snn_roi_steps_workspace_size", K, B, A, N), torch.uint8)
    n = K * B * A
    off, mask, cls = Guarded(n * 4, torch.float32), Guarded(n * 4, torch.float32), Guarded(n, torch.int64)
    hip.call("snn_roi_assign_steps", anchors.data_ptr(), labels6.data_ptr(), d_steps.data_ptr(), K, B, A, N, t0,
             float(thr), ws.ptr, off.ptr, mask.ptr, cls.ptr, _st())
    torch.cuda.synchronize()
    for name, g in (("workspace", ws), ("offset", off), ("mask", mask), ("class", cls)):
        assert g.guard_intact(), f"the guard behind the {name} buffer changed"
    return off.out(K, B, A, 4), mask.out(K, B, A, 4), cls.out(K, B, A)


@pytest.mark.parametrize("name", [p[0] for p in ROI_PLANS])
def test_roi_assign_steps_against_the_restatement(hip, name):
    from snn_for_object_detection_amd.roi import RoI
    anchors, labels6, steps, t0, ref = _roi_case(name)
    assert anchors.shape[0] == 144 and labels6.shape == (3, 5, 6)
    if name == "one_empty_slot_each":
        assert steps.tolist() == [[2, 5, 0], [-1, -1, -1]]
        assert ref.rows[0][0].shape[0] == 4 and ref.rows[0][1].shape[0] == 5 and ref.rows[0][2].shape[0] == 3
        assert int(((ref.classes[0, 1] == 0) & (ref.masks[0, 1, :, 0] == 1)).sum()) == 2    # padding rows claim anchors
    else:
        assert steps.tolist() == [[2, 0, 4], [5, 3, -1]]
    off, mask, cls = run_roi_steps_abi(hip, anchors, labels6, steps, t0, THR)
    check_roi(ref, off, mask, cls, {})
    empty = steps < 0
    assert not off[empty].any() and not mask[empty].any() and not cls[empty].any()
    assert not torch.signbit(off[empty]).any()
    o2, m2, c2 = RoI(THR).steps(anchors.cuda(), labels6.cuda(), _i32(steps), t0)
    assert c2.dtype == torch.int64 and torch.equal(c2.cpu(), cls) and torch.equal(m2.cpu(), mask)
    assert torch.equal(_bits(o2.cpu()), _bits(off))


def test_one_slot_on_one_step_gives_the_bits_of_roi_assign(hip):
    """All real rows on one step, K = 1: the packed rows of a slot are the five-column label tensor, padding rows
    included, and the shared device code must give ``snn_roi_assign``'s result bit for bit."""
    anchors = SR.grid_anchors(4, 4, 9)
    labels6 = SR.labels6_from(anchors, [[4] * 5, [4] * 3, [4] * 5], 5, seed=9)
    steps = SR.select_steps_ref(labels6, 6, 1)
    assert steps.tolist() == [[4, 4, 4]]
    off, mask, cls = run_roi_steps_abi(hip, anchors, labels6, steps, 0, THR)
    o1, m1, c1 = run_roi_abi(hip, anchors, labels6[:, :, 1:].contiguous(), THR)
    assert torch.equal(cls[0], c1) and torch.equal(mask[0], m1) and torch.equal(_bits(off[0]), _bits(o1))
    check_roi(TR.roi_assign_ref(anchors, labels6[:, :, 1:], THR), o1, m1, c1, {})


# ====================================================================================================== loss
class _Out:
    pass


def run_loss_steps_abi(hip, logits, bbox, offset, mask, classes, steps, ratio, g_loss):
    K, B, A, C = logits.shape
    d = [t.cuda().contiguous() for t in (logits, bbox, offset, mask, classes)]
    d_steps = _i32(steps)
    ws = Guarded(hip.query("snn_det_loss_steps_workspace_size", K, B, A), torch.uint8)
    stats, loss = Guarded(6, torch.float64), Guarded(1, torch.float32)
    gl, gb = Guarded(K * B * A * C, torch.float32), Guarded(K * B * A * 4, torch.float32)
    g = torch.tensor([g_loss], dtype=torch.float32, device="cuda")
    ptrs = [t.data_ptr() for t in d] + [d_steps.data_ptr()]
    hip.call("snn_det_loss_steps_fwd", *ptrs, K, B, A, C, float(ratio), ws.ptr, stats.ptr, loss.ptr, _st())
    hip.call("snn_det_loss_steps_bwd", *ptrs, K, B, A, C, float(ratio), stats.ptr, g.data_ptr(), gl.ptr, gb.ptr, _st())
    torch.cuda.synchronize()
    for name, b in (("workspace", ws), ("stats", stats), ("loss", loss), ("g_logits", gl), ("g_bbox", gb)):
        assert b.guard_intact(), f"the guard behind the {name} buffer changed"
    o = _Out()
    o.stats, o.loss, o.g_logits, o.g_bbox = stats.out(6), loss.out(1)[0], gl.out(K, B, A, C), gb.out(K, B, A, 4)
    o.device_inputs, o.d_steps = d, d_steps
    return o


def _predictions(K, B, A, C, offset, mask, seed):
    g = torch.Generator().manual_seed(seed)
    logits, bbox = torch.randn(K, B, A, C, generator=g), torch.randn(K, B, A, 4, generator=g)
    same = (torch.arange(A) % 3 == 0).expand(K, B, A)
    bbox[..., 1] = torch.where(same, offset[..., 1], bbox[..., 1])        # bbox * mask == offset * mask: gradient exactly 0
    return logits, bbox


@pytest.mark.parametrize("g_loss", [1.0, -2.5])
@pytest.mark.parametrize("name", [p[0] for p in ROI_PLANS])
def test_det_loss_steps_against_the_restatement(hip, name, g_loss):
    from snn_for_object_detection_amd import functional as HF
    _, _, steps, _, roi = _roi_case(name)
    K, B, A, C = 2, 3, 144, 3
    ratio = 0.04
    logits, bbox = _predictions(K, B, A, C, roi.offsets, roi.masks, seed=21)
    ref = SR.loss_steps_ref(logits, bbox, roi.offsets, roi.masks, roi.classes, steps, ratio, g_loss)
    assert ref.V == (3 if name == "one_empty_slot_each" else 5)
    o = run_loss_steps_abi(hip, logits, bbox, roi.offsets, roi.masks, roi.classes, steps, ratio, g_loss)
    assert float(o.stats[5]) == ref.V
    # the rows of the valid slots, in slot order, are det_loss_ref's rows: check_loss's bounds hold for them as they are
    sel = ref.valid.reshape(-1)
    inner = _Out()
    inner.stats, inner.loss = o.stats[:5], o.loss
    inner.g_logits = o.g_logits.reshape(K * B, A, C)[sel].reshape(-1, C)
    inner.g_bbox = o.g_bbox.reshape(K * B, A, 4)[sel].reshape(-1, 4)
    fails = []
    check_loss(C, ref.inner, inner, fails, {})
    assert not fails, f"{name} g_loss={g_loss}:\n  " + "\n  ".join(fails)
    # the rows of empty slots: exact zeros
    gl_empty, gb_empty = o.g_logits.reshape(K * B, A, C)[~sel], o.g_bbox.reshape(K * B, A, 4)[~sel]
    assert gl_empty.numel() > 0 and not gl_empty.any() and not gb_empty.any()
    # ---- the same through functional.detection_loss_steps: the same bits
    lg, bb, of, mk, lb = o.device_inputs
    lg, bb = lg.clone().requires_grad_(), bb.clone().requires_grad_()
    loss = HF.detection_loss_steps(lg, bb, of, mk, lb, o.d_steps, ratio)
    (loss * g_loss).backward()
    assert torch.equal(_bits(loss.detach().cpu().reshape(1)), _bits(o.loss.reshape(1)))
    assert torch.equal(lg.grad.cpu(), o.g_logits) and torch.equal(bb.grad.cpu(), o.g_bbox)


def test_det_loss_steps_without_a_valid_slot_is_zero(hip):
    """V = 0 (a batch without labels): loss 0.0 and all-zero finite gradients, whatever the targets hold."""
    from snn_for_object_detection_amd import functional as HF
    K, B, A, C = 2, 3, 144, 3
    steps = torch.full((K, B), -1, dtype=torch.int32)
    z4, zc = torch.zeros(K, B, A, 4), torch.zeros(K, B, A, dtype=torch.long)
    logits, bbox = _predictions(K, B, A, C, z4, z4, seed=22)
    for g_loss in (1.0, -2.5):
        o = run_loss_steps_abi(hip, logits, bbox, z4, z4, zc, steps, 0.04, g_loss)
        assert float(o.loss) == 0.0 and float(o.stats[5]) == 0.0 and not o.stats[:5].any()
        assert not o.g_logits.any() and not o.g_bbox.any()
    lg, bb = logits.cuda().requires_grad_(), bbox.cuda().requires_grad_()
    loss = HF.detection_loss_steps(lg, bb, z4.cuda(), z4.cuda(), zc.cuda(), _i32(steps), 0.04)
    loss.backward()
    assert float(loss.detach()) == 0.0 and not lg.grad.any() and not bb.grad.any()


def test_one_full_slot_is_detection_loss(hip):
    """K = 1 with every slot valid: V = B, so the divisor 4 A V is 4 R and the loss is ``detection_loss``'s - within
    2^-22 relative, the bound check_loss derives for the final combination."""
    from snn_for_object_detection_amd import functional as HF
    anchors = SR.grid_anchors(4, 4, 9)
    labels6 = SR.labels6_from(anchors, [[4] * 5, [4] * 3, [4] * 5], 5, seed=9)
    steps = SR.select_steps_ref(labels6, 6, 1)
    roi = SR.roi_steps_ref(anchors, labels6, steps, 0, THR)
    B, A, C = 3, 144, 3
    logits, bbox = _predictions(1, B, A, C, roi.offsets, roi.masks, seed=23)
    d = [t.cuda() for t in (logits, bbox, roi.offsets, roi.masks, roi.classes)]
    a = HF.detection_loss_steps(*d, _i32(steps), 0.04)
    b = HF.detection_loss(d[0][0], d[1][0], d[2][0], d[3][0], d[4][0], 0.04)
    print(f"steps {float(a)!r} single {float(b)!r}")
    assert abs(float(a) - float(b)) <= 2.0 ** -22 * abs(float(b))


# ====================================================================================================== refusals
def _refuser(hip, name, good):
    def refused(**kw):
        args = list(good)
        for k, v in kw.items():
            args[int(k[1:])] = v
        with pytest.raises(RuntimeError, match=name):
            hip.call(name, *args)
    return refused


def test_seq_entry_points_refuse_bad_arguments(hip):
    """One bad call for each SNN_REQUIRE of the new entry points: nothing is launched, the outputs keep their fill; the
    unchanged good call is accepted afterwards."""
    B, N, T, K, A, C, M = 2, 3, 4, 2, 8, 3, 6
    anchors = TR.grid_boxes(A + 1, torch.Generator().manual_seed(1)).cuda()
    labels6 = torch.tensor([[_row(1), _row(3), PAD], [_row(2), PAD, PAD]]).cuda()
    steps = _i32(SR.select_steps_ref(labels6.cpu(), T, K))
    outs = []

    # ---- snn_label_steps
    s_out = Guarded(K * B * 4, torch.uint8)
    good = [labels6.data_ptr(), B, N, T, K, 0, s_out.ptr, _st()]
    refused = _refuser(hip, "snn_label_steps", good)
    refused(a0=None), refused(a6=None)
    refused(a1=0), refused(a2=0), refused(a3=0), refused(a5=-1)
    refused(a4=0), refused(a4=33, a3=64), refused(a4=T + 1)
    calls = [("snn_label_steps", good)]
    outs.append(s_out)

    # ---- snn_gather_steps_fwd / _bwd
    src = torch.randn(T, B, M, 4, device="cuda")
    dst, gsrc = Guarded(K * B * M * 4, torch.float32), Guarded(T * B * M * 4, torch.float32)
    grad = torch.randn(K, B, M, 4, device="cuda")
    for name, good in (("snn_gather_steps_fwd", [src.data_ptr(), 4, steps.data_ptr(), dst.ptr, 4, T, B, K, M, 4, _st()]),
                       ("snn_gather_steps_bwd", [grad.data_ptr(), 4, steps.data_ptr(), gsrc.ptr, 4, T, B, K, M, 4, _st()])):
        refused = _refuser(hip, name, good)
        refused(a0=None), refused(a2=None), refused(a3=None)
        refused(a5=0), refused(a6=0), refused(a8=0), refused(a9=0)
        refused(a1=3), refused(a4=3)                                   # a pixel stride below the channel count
        refused(a7=0), refused(a7=33, a5=64), refused(a7=T + 1)
        calls.append((name, good))
    outs += [dst, gsrc]

    # ---- snn_roi_assign_steps
    ws = Guarded(hip.query("snn_roi_steps_workspace_size", K, B, A, N) + 16, torch.uint8)
    off, mask = Guarded(K * B * A * 4 + 4, torch.float32), Guarded(K * B * A * 4 + 4, torch.float32)
    cls = Guarded(K * B * A, torch.int64)
    good = [anchors.data_ptr(), labels6.data_ptr(), steps.data_ptr(), K, B, A, N, 0, 0.5, ws.ptr, off.ptr, mask.ptr,
            cls.ptr, _st()]
    refused = _refuser(hip, "snn_roi_assign_steps", good)
    for i in (0, 1, 2, 9, 10, 11, 12):
        refused(**{f"a{i}": None})
    refused(a4=0), refused(a5=0), refused(a6=0), refused(a7=-1)
    refused(a5=1 << 16, a6=1 << 15)                                    # A * N = 2^31
    refused(a5=(1 << 31) - 1, a6=1)
    refused(a3=0), refused(a3=33)
    refused(a0=anchors.data_ptr() + 4), refused(a9=ws.ptr + 4), refused(a10=off.ptr + 4), refused(a11=mask.ptr + 4)
    calls.append(("snn_roi_assign_steps", good))
    outs += [ws, off, mask, cls]

    # ---- snn_det_loss_steps_fwd / _bwd
    R = K * B * A
    g = torch.Generator().manual_seed(2)
    d = [t.cuda() for t in (torch.randn(R, C, generator=g), torch.randn(R, 4, generator=g), torch.randn(R, 4, generator=g),
                            torch.ones(R, 4), torch.randint(0, C, (R,), generator=g))]
    spare = torch.zeros(R * 4 + 4, device="cuda")
    lws = Guarded(hip.query("snn_det_loss_steps_workspace_size", K, B, A), torch.uint8)
    stats, loss = Guarded(6, torch.float64), Guarded(1, torch.float32)
    gl, gb = Guarded(R * C, torch.float32), Guarded(R * 4 + 4, torch.float32)
    one = torch.ones(1, device="cuda")
    ok_stats = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, 2.0], dtype=torch.float64, device="cuda")
    ptrs = [t.data_ptr() for t in d] + [steps.data_ptr()]
    fwd = ptrs + [K, B, A, C, 0.04, lws.ptr, stats.ptr, loss.ptr, _st()]
    bwd = ptrs + [K, B, A, C, 0.04, ok_stats.data_ptr(), one.data_ptr(), gl.ptr, gb.ptr, _st()]
    for name, good, ptr_args in (("snn_det_loss_steps_fwd", fwd, (0, 1, 2, 3, 4, 5, 11, 12, 13)),
                                 ("snn_det_loss_steps_bwd", bwd, (0, 1, 2, 3, 4, 5, 11, 12, 13, 14))):
        refused = _refuser(hip, name, good)
        for i in ptr_args:
            refused(**{f"a{i}": None})
        refused(a7=0), refused(a8=0), refused(a9=1), refused(a9=65)
        refused(a6=0), refused(a6=33)
        for i in (1, 2, 3):
            refused(**{f"a{i}": spare.data_ptr() + 4})
        calls.append((name, good))
    _refuser(hip, "snn_det_loss_steps_bwd", bwd)(a14=gb.ptr + 4)
    outs += [lws, stats, loss, gl, gb]

    torch.cuda.synchronize()
    for o in outs:
        assert o.untouched()
    for name, good in calls:                                           # the same arguments unchanged are accepted
        hip.call(name, *good)
    torch.cuda.synchronize()
    for o in outs:
        assert o.guard_intact()
