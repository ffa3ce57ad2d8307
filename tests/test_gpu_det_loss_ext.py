"""The detection loss kernels (csrc/det_loss.hip) under every selectable objective against the fp64 restatement of
tests/det_loss_ext_ref.py: through the C ABI on the guarded, NaN-filled buffers of tests/test_gpu_targets_fp64.py, through
``functional.detection_loss_ext`` / ``detection_loss_steps_ext`` (the same bits) and through a tiny ``SODa``.

Tolerances.  The kernels compute each row in fp32 and add the rows in fp64.  The yardstick is the SAME formulas evaluated
in fp32 torch on the CPU (``ext_loss_ref(dtype=float32)``, autograd gradients) against the fp64 reference, on this file's
own inputs: it is independent of the code under test.  The kernels get 4x that deviation (their expf / logf / atanf are
not torch's; the fp64 sums can only help).  Deviations as ``det_loss_ext_ref.deviation`` forms them: the loss relative to
the reference loss; a gradient tensor as its largest elementwise error over its largest reference magnitude.  The
constants below are the maxima measured over SMALL_SHAPES + LARGE_SHAPE and the cases listed with them
(RATIO / GAMMA / WEIGHT as below, g_loss = 1; MKL_CBWR=COMPATIBLE as tests/conftest.py sets it);
tests/test_det_loss_ext_host.py re-measures the small shapes against them.  A yardstick of 0 asks for equality: exact
zeros (rows that are no box rows; the size gradients past the clamp; GIoU of a clamped prediction that contains its
target depends on no offset at all).

Measured on one MI355X, largest kernel deviation over its yardstick across all cases: loss 0.78, d loss / d logits 2.2
(focal), d loss / d bbox 2.1 (l1: 4.75e-8, the rounding of weight / (4 A V)) and 1.2 in the IoU modes.
"""
import pytest
import torch

from tests import det_loss_ext_ref as R

RATIO, GAMMA, WEIGHT = 0.04, 2.0, 1.5
SMALL_SHAPES = [(2, 300, 3), (2, 300, 2), (2, 300, 64)]   # (frames, A, K): 600 rows = two full blocks and a ragged third
LARGE_SHAPE = (900, 300, 3)                                # 270 000 rows > 1024 blocks x 256 threads: a second grid pass
MAX_CLASSES = 64

# fp32 CPU vs fp64, largest over shapes and cases: loss per (cls, box) mode
YARD_LOSS = {("ce", "l1"): 1.93e-07, ("ce", "giou"): 2.00e-07, ("ce", "diou"): 2.00e-07, ("ce", "ciou"): 2.00e-07,
             ("focal", "l1"): 1.81e-07, ("focal", "giou"): 1.49e-07, ("focal", "diou"): 1.63e-07,
             ("focal", "ciou"): 1.49e-07}
# ... d loss / d logits per cls mode
YARD_G_LOGITS = {"ce": 1.81e-07, "focal": 2.80e-07}
# ... d loss / d bbox per (case, box mode).  l1: the one rounding of weight / (4 A V)
YARD_G_BBOX = {
    ("random", "l1"): 2.24e-08, ("random", "giou"): 2.18e-06, ("random", "diou"): 2.61e-06, ("random", "ciou"): 2.62e-06,
    ("disjoint", "l1"): 2.24e-08, ("disjoint", "giou"): 1.19e-06, ("disjoint", "diou"): 5.46e-07,
    ("disjoint", "ciou"): 5.16e-07,
    ("pred_contains", "l1"): 2.24e-08, ("pred_contains", "giou"): 2.49e-06, ("pred_contains", "diou"): 2.27e-06,
    ("pred_contains", "ciou"): 2.37e-06,
    ("target_contains", "l1"): 2.24e-08, ("target_contains", "giou"): 2.56e-06, ("target_contains", "diou"): 2.56e-06,
    ("target_contains", "ciou"): 2.54e-06,
    ("clamped", "l1"): 2.24e-08, ("clamped", "giou"): 0.0, ("clamped", "diou"): 7.49e-06, ("clamped", "ciou"): 7.51e-06,
    ("equal", "l1"): 0.0, ("equal", "giou"): 0.0, ("equal", "diou"): 0.0, ("equal", "ciou"): 0.0,
    ("no_pos", "l1"): 2.24e-08, ("no_pos", "giou"): 0.0, ("no_pos", "diou"): 0.0, ("no_pos", "ciou"): 0.0,
}
FACTOR = 4.0     # bound = FACTOR x yardstick: loss <= 8.0e-7, g_logits <= 1.1e-6, g_bbox <= 9.0e-8 (l1) ... 3.0e-5 (clamped)

_INPUTS = {}
_REFS = {}


def inputs(Fr, A, K, case):
    key = (Fr, A, K, case)
    if key not in _INPUTS:
        _INPUTS[key] = R.ext_inputs(Fr, A, K, case, seed=Fr * 1000 + K)
    return _INPUTS[key]


def reference(Fr, A, K, case, cls_mode, box_mode):
    """fp64, computed once per (inputs, mode) and shared."""
    key = (Fr, A, K, case, cls_mode, box_mode)
    if key not in _REFS:
        _REFS[key] = R.ext_loss_ref(*inputs(Fr, A, K, case), RATIO, cls_mode, GAMMA, box_mode, WEIGHT)
    return _REFS[key]


def check_case_reaches_its_edge(inp, case):
    """On the CPU, in fp64: the named case is what its name says on every box row."""
    Fr, A, _ = inp.bbox.shape
    bb, off = inp.bbox.double().reshape(-1, 4), inp.offset.double().reshape(-1, 4)
    rows = ((inp.labels > 0) & (inp.mask == 1).all(dim=-1)).reshape(-1)
    if case == "no_pos":
        assert not bool((inp.labels > 0).any())
        return
    assert int(rows.sum()) > 10 and int(((inp.labels > 0).reshape(-1) & ~rows).sum()) > 0      # positives without a mask too
    assert int(((inp.labels == 0) & (inp.mask == 1).all(dim=-1)).sum()) > 0                    # the padded-label quirk
    anc = inp.anchors.double().repeat(Fr, 1)
    p, g = R.decode(anc, bb)[rows], R.decode(anc, off)[rows]
    inter, union, _, _ = R.iou_terms(p, g)
    if case == "disjoint":
        assert bool((inter == 0).all())
    elif case == "pred_contains":
        assert bool(((p[:, :2] < g[:, :2]) & (p[:, 2:] > g[:, 2:])).all())
    elif case == "target_contains":
        assert bool(((g[:, :2] < p[:, :2]) & (g[:, 2:] > p[:, 2:])).all())
    elif case == "clamped":
        assert bool((bb[rows][:, 2:] / 5 > R.EXP_CLAMP + 0.4).all())
    elif case == "equal":
        assert torch.equal(inp.bbox.reshape(-1, 4)[rows], inp.offset.reshape(-1, 4)[rows])
    else:
        assert bool((inter > 0).any())


# ====================================================================================================== device side
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from snn_for_object_detection_amd import _hip
    return _hip


def _st():
    return torch.cuda.current_stream().cuda_stream


class Out:
    pass


def run_ext_abi(hip, inp, cls_mode, gamma, box_mode, weight, steps=None, ratio=RATIO, g_loss=1.0):
    """snn_det_loss_ext_fwd / _bwd through the C ABI on guarded buffers -> host tensors."""
    from tests.test_gpu_targets_fp64 import Guarded
    Fr, A, K = inp.logits.shape
    rows = Fr * A
    d = [t.cuda().contiguous() for t in inp]
    st = None if steps is None else steps.to(torch.int32).cuda().contiguous()
    ws = Guarded(hip.query("snn_det_loss_ext_workspace_size", rows), torch.uint8)
    stats, loss = Guarded(9, torch.float64), Guarded(1, torch.float32)
    gl, gb = Guarded(rows * K, torch.float32), Guarded(rows * 4, torch.float32)
    g = torch.tensor([g_loss], dtype=torch.float32, device="cuda")
    head = [t.data_ptr() for t in d] + [None if st is None else st.data_ptr(), rows, A, K, float(ratio),
                                        hip.LOSS_CLS_MODES[cls_mode], float(gamma), hip.LOSS_BOX_MODES[box_mode],
                                        float(weight)]
    hip.call("snn_det_loss_ext_fwd", *head, ws.ptr, stats.ptr, loss.ptr, _st())
    hip.call("snn_det_loss_ext_bwd", *head, stats.ptr, g.data_ptr(), gl.ptr, gb.ptr, _st())
    torch.cuda.synchronize()
    for name, b in (("workspace", ws), ("stats", stats), ("loss", loss), ("g_logits", gl), ("g_bbox", gb)):
        assert b.guard_intact(), f"the guard behind the {name} buffer changed"
    o = Out()
    o.stats, o.loss, o.g_logits, o.g_bbox = stats.out(9), loss.out(1)[0], gl.out(Fr, A, K), gb.out(Fr, A, 4)
    o.device_inputs, o.device_steps = d, st
    return o


def check_against(ref, o, case, cls_mode, box_mode, fails, tag):
    dl, dgl, dgb = R.deviation(o.loss, o.g_logits, o.g_bbox, ref, skip_box_rows=case == "equal")
    print(f"{tag}: deviation / yardstick: loss {dl:.3g} / {YARD_LOSS[(cls_mode, box_mode)]:.3g}, g_logits {dgl:.3g} / "
          f"{YARD_G_LOGITS[cls_mode]:.3g}, g_bbox {dgb:.3g} / {YARD_G_BBOX[(case, box_mode)]:.3g}")
    if not dl <= FACTOR * YARD_LOSS[(cls_mode, box_mode)]:
        fails.append(f"{tag}: loss {float(o.loss)!r} vs {ref.loss!r}: {dl:.3g} > 4 x {YARD_LOSS[(cls_mode, box_mode)]:.3g}")
    if not dgl <= FACTOR * YARD_G_LOGITS[cls_mode]:
        fails.append(f"{tag}: g_logits {dgl:.3g} > 4 x {YARD_G_LOGITS[cls_mode]:.3g}")
    if not dgb <= FACTOR * YARD_G_BBOX[(case, box_mode)]:
        fails.append(f"{tag}: g_bbox {dgb:.3g} > 4 x {YARD_G_BBOX[(case, box_mode)]:.3g}")
    if not (bool(torch.isfinite(o.g_logits).all()) and bool(torch.isfinite(o.g_bbox).all()) and bool(torch.isfinite(o.loss))):
        fails.append(f"{tag}: non-finite loss or gradient")
    # the terms: counts exactly, V, and loss = (pos term + neg term) + box term in fp32
    s = o.stats
    terms = s[6:9].float()
    if not torch.equal(((terms[0] + terms[1]) + terms[2]).reshape(1).view(torch.int32), o.loss.reshape(1).view(torch.int32)):
        fails.append(f"{tag}: the three terms of stats do not add up to the loss")
    if float(s[5]) != ref.V:
        fails.append(f"{tag}: V {float(s[5])} != {ref.V}")
    for name, got, want in (("cls", float(terms[0] + terms[1]), ref.cls), ("box", float(terms[2]), ref.box)):
        if not abs(got - want) <= FACTOR * YARD_LOSS[(cls_mode, box_mode)] * abs(ref.loss):
            fails.append(f"{tag}: {name} term {got!r} vs {want!r}")
    if box_mode != "l1":
        if bool(o.g_bbox[~ref.box_rows].any()):
            fails.append(f"{tag}: rows that are no box rows have a box gradient")
        if ref.n_pos == 0 and (float(terms[2]) != 0.0 or bool(o.g_bbox.any())):
            fails.append(f"{tag}: box term without positives")
        if case == "clamped" and bool(o.g_bbox[..., 2:].any()):
            fails.append(f"{tag}: size gradients past the clamp are not exact zeros")
        if case == "disjoint" and box_mode in ("giou", "diou") and not bool((o.g_bbox[ref.box_rows][:, :2] != 0).all()):
            fails.append(f"{tag}: a disjoint box row has no centre gradient")
        if case == "equal" and not float(terms[2]) <= 1e-3:
            fails.append(f"{tag}: box term {float(terms[2])} of equal boxes")


CASE_PARAMS = [(s, c) for s in SMALL_SHAPES for c in R.CASES] + [(LARGE_SHAPE, c) for c in R.CASES[:5]]


@pytest.mark.parametrize("shape,case", CASE_PARAMS, ids=[f"{s[0]}x{s[1]}x{s[2]}-{c}" for s, c in CASE_PARAMS])
def test_ext_loss_against_fp64(hip, shape, case):
    """Every (cls, box) mode on every shape and case: loss, both gradients and the logged terms against fp64; exact zeros
    where the formulas give zeros; a second run returns the same bits; ``functional.detection_loss_ext`` returns the bits
    of the C-ABI call."""
    from snn_for_object_detection_amd import functional as HF
    Fr, A, K = shape
    inp = inputs(Fr, A, K, case)
    if case != "equal":
        assert not bool(R.tied_rows(inp.bbox, inp.offset, inp.mask, inp.labels, inp.anchors).any())
    check_case_reaches_its_edge(inp, case)
    fails = []
    for cls_mode, box_mode in R.MODES:
        ref = reference(Fr, A, K, case, cls_mode, box_mode)
        o = run_ext_abi(hip, inp, cls_mode, GAMMA, box_mode, WEIGHT)
        check_against(ref, o, case, cls_mode, box_mode, fails, f"{cls_mode}-{box_mode}")
        if case == "disjoint" and box_mode != "l1":
            assert float(o.stats[4]) >= float(ref.box_rows.sum())            # IoU 0: every row's 1 - IoU + penalty >= 1
        if (cls_mode, box_mode) in (("focal", "ciou"), ("ce", "giou")):
            again = run_ext_abi(hip, inp, cls_mode, GAMMA, box_mode, WEIGHT)
            for a, b in ((o.loss.reshape(1), again.loss.reshape(1)), (o.g_logits, again.g_logits), (o.g_bbox, again.g_bbox),
                         (o.stats, again.stats)):
                assert torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                                   b.view(torch.int64 if b.dtype == torch.float64 else torch.int32))
            lg, bb, of, mk, lb, an = o.device_inputs
            lg, bb = lg.clone().requires_grad_(), bb.clone().requires_grad_()
            loss, t_cls, t_box = HF.detection_loss_ext(lg, bb, of, mk, lb, an, RATIO, cls_mode, GAMMA, box_mode, WEIGHT,
                                                       return_terms=True)
            loss.backward()
            assert torch.equal(loss.detach().cpu().reshape(1).view(torch.int32), o.loss.reshape(1).view(torch.int32))
            assert torch.equal(lg.grad.cpu(), o.g_logits) and torch.equal(bb.grad.cpu(), o.g_bbox)
            assert float(t_cls + t_box) == float(loss.detach())
    assert not fails, f"{shape} [{case}]:\n  " + "\n  ".join(fails)


@pytest.mark.parametrize("empty", ["one", "all"])
def test_ext_loss_over_slots(hip, empty):
    """The steps flavour at K = 3 slots, B = 2: one empty slot / every slot empty, every mode: the rows of an empty slot
    take no part and get exact zeros in both gradients; V = 0 gives loss 0 and zero gradients."""
    from snn_for_object_detection_amd import functional as HF
    Ks, B, A, K = 3, 2, 300, 3
    inp = inputs(Ks * B, A, K, "random")
    assert not bool(R.tied_rows(inp.bbox, inp.offset, inp.mask, inp.labels, inp.anchors).any())
    steps = torch.tensor([[3, -1], [5, 2], [7, 4]], dtype=torch.int32) if empty == "one" else torch.full((Ks, B), -1, dtype=torch.int32)
    fails = []
    for cls_mode, box_mode in R.MODES:
        ref = R.ext_loss_ref(*inp, RATIO, cls_mode, GAMMA, box_mode, WEIGHT, steps=steps)
        assert ref.V == (5 if empty == "one" else 0)
        o = run_ext_abi(hip, inp, cls_mode, GAMMA, box_mode, WEIGHT, steps=steps)
        check_against(ref, o, "random", cls_mode, box_mode, fails, f"{cls_mode}-{box_mode}")
        dead = (steps.reshape(-1) < 0)
        assert not bool(o.g_logits[dead].any()) and not bool(o.g_bbox[dead].any())
        if empty == "all":
            assert float(o.loss) == 0.0 and not bool(o.stats[6:9].any())
        lg, bb, of, mk, lb, an = o.device_inputs
        shp = lambda t, last: t.view(Ks, B, A, last)
        lg, bb = shp(lg, K).clone().requires_grad_(), shp(bb, 4).clone().requires_grad_()
        loss = HF.detection_loss_steps_ext(lg, bb, shp(of, 4), shp(mk, 4), lb.view(Ks, B, A), an, o.device_steps, RATIO,
                                           cls_mode, GAMMA, box_mode, WEIGHT)
        loss.backward()
        assert torch.equal(loss.detach().cpu().reshape(1).view(torch.int32), o.loss.reshape(1).view(torch.int32))
        assert torch.equal(lg.grad.cpu().view(Ks * B, A, K), o.g_logits) and torch.equal(bb.grad.cpu().view(Ks * B, A, 4), o.g_bbox)
    assert not fails, "\n  ".join(fails)


def _flat(inp, ratio=RATIO, g_loss=1.0):
    """The rows of ``inp`` as ``run_loss_abi`` of tests/test_gpu_targets_fp64.py takes them."""
    K = inp.logits.shape[-1]
    return (inp.logits.reshape(-1, K), inp.bbox.reshape(-1, 4), inp.offset.reshape(-1, 4), inp.mask.reshape(-1, 4),
            inp.labels.reshape(-1), ratio, g_loss)


def _assert_same_sums_and_gradients(o, old, tag):
    """The five totals and both gradients of an ``_ext`` run and of an snn_det_loss_* / snn_det_loss_steps_* run: equal."""
    assert torch.equal(o.stats[:5], old.stats[:5]), f"{tag}: stats {o.stats[:5].tolist()} vs {old.stats[:5].tolist()}"
    assert torch.equal(o.g_logits.reshape(old.g_logits.shape), old.g_logits), f"{tag}: g_logits"
    assert torch.equal(o.g_bbox.reshape(old.g_bbox.shape), old.g_bbox), f"{tag}: g_bbox"


@pytest.mark.parametrize("cls_mode", R.CLS_MODES)
def test_gamma_0_with_l1_is_the_existing_loss(hip, cls_mode):
    """Cross entropy (or focal with ``gamma = 0``), L1, weight 1 against snn_det_loss_fwd / _bwd on the same inputs: the
    same kernels in the same order, so the loss, the five totals and both gradients are equal - on 600 rows (two full
    blocks and a ragged third) and on 270 000 (a second grid pass); the inputs have positives and negatives.  The same for
    snn_det_loss_steps_fwd / _bwd with one empty slot among six."""
    from tests.test_gpu_targets_fp64 import run_loss_abi
    from tests.test_gpu_seq_targets import run_loss_steps_abi
    for Fr, A, K in SMALL_SHAPES + [LARGE_SHAPE]:
        inp = inputs(Fr, A, K, "random")
        assert bool((inp.labels > 0).any()) and bool((inp.labels == 0).any())
        o = run_ext_abi(hip, inp, cls_mode, 0.0, "l1", 1.0)
        old = run_loss_abi(hip, _flat(inp))
        print(f"{Fr}x{A}x{K}: ext {float(o.loss)!r} existing {float(old.loss)!r}")
        assert torch.equal(o.loss, old.loss)
        _assert_same_sums_and_gradients(o, old, f"{Fr}x{A}x{K}")
    Ks, B, A, K = 3, 2, 300, 3
    inp = inputs(Ks * B, A, K, "random")
    steps = torch.tensor([[3, -1], [5, 2], [7, 4]], dtype=torch.int32)
    o = run_ext_abi(hip, inp, cls_mode, 0.0, "l1", 1.0, steps=steps)
    shp = lambda t, *last: t.reshape(Ks, B, A, *last)
    old = run_loss_steps_abi(hip, shp(inp.logits, K), shp(inp.bbox, 4), shp(inp.offset, 4), shp(inp.mask, 4),
                             shp(inp.labels), steps, RATIO, 1.0)
    print(f"steps: ext {float(o.loss)!r} existing {float(old.loss)!r}")
    assert torch.equal(o.loss, old.loss) and float(old.stats[5]) == 5.0 and float(o.stats[5]) == 5.0
    _assert_same_sums_and_gradients(o, old, "steps")


def test_an_empty_class_is_nan_in_the_existing_loss_and_zero_in_ext(hip):
    """The one difference between snn_det_loss_* and snn_det_loss_ext_* at cross entropy, L1, weight 1: without positives
    the former divide 0 by 0 (NaN, as the reference's ``ce[pos].mean()``), the latter by ``max(n_pos, 1)``: the positive
    term is 0 and the loss is (0 + negative term) + box term - the box term itself where ``loss_ratio = 1`` leaves the
    negatives no weight.  The totals and the gradients are equal all the same.  ``detection_loss_steps``: every slot
    empty gives 0 and zero gradients, a valid slot without positives NaN.  (``stats`` is guarded at the 5, 6 and 9
    doubles the three entry families own: ``run_loss_abi``, ``run_loss_steps_abi``, ``run_ext_abi``.)"""
    from snn_for_object_detection_amd import functional as HF
    from tests.test_gpu_targets_fp64 import run_loss_abi
    from tests.test_gpu_seq_targets import run_loss_steps_abi
    Fr, A, K = 2, 300, 3
    inp = inputs(Fr, A, K, "no_pos")
    assert not bool((inp.labels > 0).any())
    for ratio in (RATIO, 1.0):
        old = run_loss_abi(hip, _flat(inp, ratio))
        assert bool(torch.isnan(old.loss))
        o = run_ext_abi(hip, inp, "ce", 0.0, "l1", 1.0, ratio=ratio)
        terms = o.stats[6:9].float()
        assert float(terms[0]) == 0.0 and bool(torch.isfinite(o.loss)) and float(terms[2]) > 0
        assert torch.equal(((terms[0] + terms[1]) + terms[2]).reshape(1), o.loss.reshape(1))
        if ratio == 1.0:
            assert float(terms[1]) == 0.0 and float(o.loss) == float(terms[2])
        else:
            assert float(terms[1]) > 0 and bool(old.g_logits.any())       # (at ratio 1 the negatives' weight is 0)
        _assert_same_sums_and_gradients(o, old, f"ratio {ratio}")
        assert float(o.stats[1]) == 0.0 and bool(torch.isfinite(old.g_logits).all()) and bool(old.g_bbox.any())
    d = [t.cuda() for t in inp[:5]]
    assert bool(torch.isnan(HF.detection_loss(*d, RATIO)))
    assert bool(torch.isfinite(HF.detection_loss_ext(*d, inp.anchors.cuda(), RATIO)))
    # ---- two slots of one sample
    shp = lambda t, *last: t.reshape(Fr, 1, A, *last)
    slots = [shp(inp.logits, K), shp(inp.bbox, 4), shp(inp.offset, 4), shp(inp.mask, 4), shp(inp.labels)]
    for steps, want_nan in (([[-1], [-1]], False), ([[0], [-1]], True)):
        steps = torch.tensor(steps, dtype=torch.int32)
        old = run_loss_steps_abi(hip, *slots, steps, RATIO, 1.0)
        lg, bb = slots[0].cuda().requires_grad_(), slots[1].cuda().requires_grad_()
        loss = HF.detection_loss_steps(lg, bb, *(t.cuda() for t in slots[2:]), steps.cuda(), RATIO)
        loss.backward()
        assert torch.equal(lg.grad.cpu(), old.g_logits) and torch.equal(bb.grad.cpu(), old.g_bbox)
        if want_nan:
            assert bool(torch.isnan(loss)) and bool(torch.isnan(old.loss)) and float(old.stats[5]) == 1.0
            assert not bool(lg.grad[1].any()) and bool(lg.grad[0].any()) and bool(torch.isfinite(lg.grad).all())
        else:
            assert float(loss.detach()) == 0.0 and float(old.loss) == 0.0
            assert not bool(lg.grad.any()) and not bool(bb.grad.any())


def test_ext_loss_refusals(hip):
    """Host-side refusals of both entry points: an error code before any launch, the outputs keep their fill."""
    from tests.test_gpu_targets_fp64 import Guarded
    Fr, A, K = 2, 8, 3
    inp = R.ext_inputs(Fr, A, K, "random", 5)
    R_ = Fr * A
    d = [t.cuda().contiguous() for t in inp]
    spare = torch.zeros(R_ * 4 + 4, device="cuda")
    steps = torch.zeros(Fr, dtype=torch.int32, device="cuda")
    ws = Guarded(hip.query("snn_det_loss_ext_workspace_size", R_), torch.uint8)
    stats, loss = Guarded(9, torch.float64), Guarded(1, torch.float32)
    gl, gb = Guarded(R_ * 65, torch.float32), Guarded(R_ * 4 + 4, torch.float32)
    g = torch.ones(1, device="cuda")
    ok_stats = torch.ones(9, dtype=torch.float64, device="cuda")
    head = [t.data_ptr() for t in d] + [steps.data_ptr(), R_, A, K, 0.04, 1, 2.0, 3, 1.0]
    fwd = head + [ws.ptr, stats.ptr, loss.ptr, _st()]
    bwd = head + [ok_stats.data_ptr(), g.data_ptr(), gl.ptr, gb.ptr, _st()]

    def refused(name, good, **kw):
        args = list(good)
        for k, v in kw.items():
            args[int(k[1:])] = v
        with pytest.raises(RuntimeError, match=name):
            hip.call(name, *args)

    for name, good, ptr_args in (("snn_det_loss_ext_fwd", fwd, (0, 1, 2, 3, 4, 5, 15, 16, 17)),
                                 ("snn_det_loss_ext_bwd", bwd, (0, 1, 2, 3, 4, 5, 15, 16, 17, 18))):
        for i in ptr_args:
            refused(name, good, **{f"a{i}": None})                      # null pointers (steps, a6, may be null)
        refused(name, good, a9=0)                                       # K outside 1 .. kMaxClasses
        refused(name, good, a9=MAX_CLASSES + 1)
        refused(name, good, a7=0)                                       # rows
        refused(name, good, a7=R_ + 1)                                  # ... not a multiple of A
        refused(name, good, a8=0)
        refused(name, good, a11=2)                                      # unknown modes
        refused(name, good, a11=-1)
        refused(name, good, a13=4)
        refused(name, good, a13=-1)
        refused(name, good, a12=-0.5)                                   # gamma < 0
        refused(name, good, a12=float("nan"))
        for i in (1, 2, 3, 5):                                          # float4 arrays: 16-byte alignment
            refused(name, good, **{f"a{i}": spare.data_ptr() + 4})
    refused("snn_det_loss_ext_bwd", bwd, a18=gb.ptr + 4)
    torch.cuda.synchronize()
    assert ws.untouched() and stats.untouched() and loss.untouched() and gl.untouched() and gb.untouched()
    hip.call("snn_det_loss_ext_fwd", *fwd)                              # the same arguments unchanged are accepted
    hip.call("snn_det_loss_ext_bwd", *(head + [stats.ptr, g.data_ptr(), gl.ptr, gb.ptr, _st()]))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss.out(1)).all()) and bool(torch.isfinite(gb.buf[:R_ * 4]).all())


def test_functional_refuses_what_the_kernel_would_misread(hip):
    from snn_for_object_detection_amd import functional as HF
    Fr, A, K = 2, 8, 3
    lg, bb, of, mk, lb, an = (t.cuda() for t in R.ext_inputs(Fr, A, K, "random", 6))
    HF.detection_loss_ext(lg, bb, of, mk, lb, an, RATIO, "focal", 2.0, "ciou")
    for bad in ((lg, bb, of.cpu(), mk, lb, an), (lg, bb, of, mk.double(), lb, an), (lg, bb, of, mk, lb.cpu(), an),
                (lg, bb, of, mk, lb, an.cpu()), (lg, bb, of, mk, lb, an.double()), (lg, bb, of, mk, lb, an[:A - 1]),
                (lg, bb, of, mk[:, :A - 1], lb, an), (lg, bb, of, mk, lb.int(), an)):
        with pytest.raises(RuntimeError):
            HF.detection_loss_ext(*bad, RATIO, "focal", 2.0, "ciou")
    for opts in (("bce", 2.0, "l1", 1.0), ("ce", 2.0, "iou", 1.0), ("focal", -1.0, "l1", 1.0), ("ce", 2.0, "giou", -1.0)):
        with pytest.raises(ValueError):
            HF.detection_loss_ext(lg, bb, of, mk, lb, an, RATIO, *opts)
    steps = torch.zeros(1, Fr, dtype=torch.int32, device="cuda")
    v = lambda t: t.unsqueeze(0)
    HF.detection_loss_steps_ext(v(lg), v(bb), v(of), v(mk), v(lb), an, steps, RATIO, "focal", 2.0, "diou")
    for bad_steps in (steps.cpu(), steps.long(), steps[:, :1], torch.zeros(2, Fr, dtype=torch.int32, device="cuda")):
        with pytest.raises(RuntimeError):
            HF.detection_loss_steps_ext(v(lg), v(bb), v(of), v(mk), v(lb), an, bad_steps, RATIO, "focal", 2.0, "diou")
    torch.cuda.synchronize()


# ====================================================================================================== model level
T, B, H, W = 4, 2, 32, 48


def _tiny_net(L):
    class Net(L.SODa):
        def backbone_cfgs(self):
            return [L.Conv(8, 3, 2), L.Norm(), L.ReLU(), L.Conv(16, 3, 2), L.Norm(), L.ReLU()]

        def neck_cfgs(self):
            return [L.Conv(16, 3, 2), L.Norm(), L.Tanh(), L.Return()]

        def head_cfgs(self, box_out, cls_out):
            return [[L.Conv(kernel_size=1), L.Norm(), L.Tanh()], [L.Conv(box_out, 1)], [L.Conv(cls_out, 1)]]
    return Net


def _spy(monkeypatch, HF, name, calls):
    orig = getattr(HF, name)

    def wrapped(*a, **k):
        calls.append((name, a, k))
        return orig(*a, **k)
    monkeypatch.setattr(HF, name, wrapped)


@pytest.mark.parametrize("label_steps", [None, 2])
def test_training_step_with_a_selected_objective(hip, monkeypatch, label_steps):
    """A tiny generated SODa with ``cls_loss="focal", box_loss="ciou"``: the device loss of ``training_step`` is finite
    and equals the CPU branch's expression (``soda.detection_loss_host``, fp32 torch) on the same predictions and targets
    - one side within 4x, the other within 1x the yardstick of the fp64 value, so within 5x of each other - on the
    one-label and on the ``label_steps=2`` path; ``train_loss_cls + train_loss_box`` is ``train_loss``; gradients reach
    the first layer.  With the defaults the steps call ``detection_loss`` / ``detection_loss_steps`` and log the
    reference's keys only."""
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd import functional as HF
    from snn_for_object_detection_amd import soda
    from tests.util import synthetic_events, synthetic_labels
    calls = []
    for name in ("detection_loss", "detection_loss_steps", "detection_loss_ext", "detection_loss_steps_ext"):
        _spy(monkeypatch, HF, name, calls)
    Net = _tiny_net(S)
    X = synthetic_events(T, B, H, W, p=0.08).cuda()
    labels = synthetic_labels(B, n_boxes=2, seed=1)
    if label_steps:
        six = torch.full((B, 3, 6), -1.0)
        six[:, :2, 1:] = labels
        six[0, 0, 0], six[0, 1, 0], six[1, 0, 0], six[1, 1, 0] = 1.0, 3.0, 3.0, 3.0       # sample 1: one empty slot
        labels = six
    opts = dict(cls_loss="focal", focal_gamma=GAMMA, box_loss="ciou", box_loss_weight=WEIGHT)
    torch.manual_seed(2)
    model = Net(num_classes=2, time_window=0, label_steps=label_steps, **opts).cuda().train()
    loss = model.training_step((X, labels.cuda()))
    loss.backward()
    want = "detection_loss_steps_ext" if label_steps else "detection_loss_ext"
    assert [c[0] for c in calls] == [want]
    a = [t.detach().cpu() if isinstance(t, torch.Tensor) else t for t in calls[0][1]]
    valid = (a[6] >= 0) if label_steps else None
    ratio = a[7] if label_steps else a[6]
    if label_steps:
        assert a[6].tolist() == [[1, 3], [3, -1]]
    assert int((a[4] > 0).sum()) > 0
    t_cls, t_box = soda.detection_loss_host(*a[:6], ratio, valid=valid, **opts)
    cpu = float(t_cls + t_box)
    dev = float(loss.detach())
    print(f"label_steps {label_steps}: device {dev!r} CPU branch {cpu!r}")
    assert bool(torch.isfinite(loss)) and dev > 0
    assert abs(dev - cpu) <= 5 * YARD_LOSS[("focal", "ciou")] * abs(cpu)
    assert set(model.logged) == {"train_loss", "train_loss_cls", "train_loss_box"}
    assert {"train_loss_cls", "train_loss_box"} <= model._sync_logged
    assert model.logged["train_loss_cls"].is_cuda and model.logged["train_loss_box"].is_cuda
    assert float(model.logged["train_loss_cls"] + model.logged["train_loss_box"]) == float(model.logged["train_loss"])
    assert float(model.logged["train_loss_box"]) > 0
    g0 = next(model.base_net.parameters()).grad
    assert g0 is not None and bool(torch.isfinite(g0).all()) and bool(g0.any())
    # ---- the defaults: the reference's objective through the functions it always went through
    del calls[:]
    torch.manual_seed(2)
    plain = Net(num_classes=2, time_window=0, label_steps=label_steps).cuda().train()
    plain.training_step((X, labels.cuda()))
    assert [c[0] for c in calls] == ["detection_loss_steps" if label_steps else "detection_loss"]
    assert set(plain.logged) == {"train_loss"}
