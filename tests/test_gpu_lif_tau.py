"""LIF with per-channel, learnable time constants (``functional.affine_neuron(tau=(w_mem, w_syn))``, snn_lif_tau_*) against
the float64 restatement of tests/lif_tau_ref.py, on every class of the reverse scan, and the layer inside a model.

Every row of tests/lif_tau_cases.py calls ``affine_neuron`` forward and backward with constants drawn in c_mem in [0.1, 0.5]
and 1 + c_syn in [0.5, 0.95], different in every channel, and compares the spikes, the final state, dy, dgamma, dbias, g_v0,
g_i0 and the two new gradients dL/dw_mem, dL/dw_syn with the reference; the scan class is proven through
``lif_tau_bwd_plan``.  tests/test_lif_tau_host.py checks, without a GPU, that these inputs tell a wrong kernel apart.

Bounds.  The quantities the scan has always produced take ``FWD_REL``, ``TOL_STATE`` and the spike rule of
tests/test_gpu_norm_neuron_fp64.py, imported (c_mem >= 0.1 keeps the leak's gain <= 10 of that derivation; the slopes are
those of tests/lif_gradient_cases.py).  dL/dw_mem and dL/dw_syn: ||got - ref||_2 / ||ref||_2 per tensor against float64, at
most 16 x the same quantity of the float32 restatement on the same inputs and forced spikes, computed in the test: the
kernel rebuilds i' from stored potentials with one division by c_mem >= 0.1 (a rounding of vd amplified by up to 10) and
sums in another order with block partials in double; the rest of the factor is headroom for the two together.

Measured on an MI355X (||got - ref|| / ||ref||: kernel, float32 yardstick, their ratio; the bound is a ratio of 16):

    row                        dL/dw_mem: kernel  yardstick  ratio     dL/dw_syn: kernel  yardstick  ratio
    c4_vec4_ordered_state                 7.61e-07  2.58e-06  0.29                 1.04e-07  8.32e-07  0.13
    c3_vec1_layer                         2.79e-06  5.53e-06  0.51                 5.41e-08  2.41e-07  0.23
    c16_nobn_mode0                        4.88e-06  4.90e-06  1.00                 3.98e-07  3.67e-07  1.08
    c24_atomics_addend                    3.13e-06  2.87e-06  1.09                 4.26e-07  2.74e-07  1.55
    c512_gy_atan_detached                 2.59e-06  2.67e-06  0.97                 1.07e-06  1.21e-06  0.89
    c16_wide                              3.02e-06  4.00e-06  0.76                 3.01e-07  4.94e-07  0.61
    c32_spikes_never_stored               4.80e-06  3.65e-06  1.32                 7.38e-07  7.40e-07  1.00
    c16_rpb_gt1                           5.42e-07  6.12e-07  0.89                 3.31e-07  3.17e-07  1.04

(the two LDS-atomics rows, c3 and c24, move in the last digits from run to run.)  No spike decision differs from the reference's on any row.
"""
import pytest
import torch

from tests import lif_tau_cases as TC
from tests import test_gpu_lif_gradient as TG
from tests import test_gpu_norm_neuron_fp64 as F
from tests.lif_gradient_cases import SLOPE
from tests.test_gpu_norm_neuron_fp64 import FWD_REL, TOL_STATE, D  # noqa: F401  (the bounds of this file)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def HF(hip_lib):
    from snn_for_object_detection_amd import functional
    return functional


def params_of(HF, rule):
    return HF.neuron_params(surrogate=rule[0], alpha=SLOPE[rule[0]], detach_reset=rule[1])


# ------------------------------------------------------------------------------------------------------ device run
def run_device(HF, row, inp, slots=None, learn=True):
    """forward + backward of one row on the device -> (DevResult, {"w_mem", "w_syn"} gradients, (c_mem, c_syn), bits).
    ``slots``: a pair of GradSlots the two raw parameters carry (their gradients then arrive there, not through autograd)."""
    from snn_for_object_detection_amd import _hip
    from snn_for_object_detection_amd.layer_gen import HipBatchNorm2d
    cs = row.cs
    with HF.levers(SCAN_FLAGS=_hip.SCAN_WIDE_ADDRESSING if row.variant == "wide" else 0):
        bn = None
        if cs.bn is not None:
            bn = HipBatchNorm2d(cs.C).cuda()
            with torch.no_grad():
                bn.weight.copy_(inp.gamma)
                bn.bias.copy_(inp.bias)
                bn.running_mean.copy_(inp.rm)
                bn.running_var.copy_(inp.rv)
            bn.train(cs.bn == "train")
        w_mem, w_syn = (w.cuda().requires_grad_(learn) for w in TC.raw_parameters(row))
        if slots is not None:
            w_mem._snn_grad_slot, w_syn._snn_grad_slot = slots
        c_mem, c_syn = HF.lif_time_constants(w_mem, w_syn, cs.C)
        y = F._cl(inp.y).requires_grad_()
        wrt = [y] + ([bn.weight, bn.bias] if bn is not None else [])
        state = None
        if cs.state:
            v0, i0 = F._cl(inp.v0).requires_grad_(), F._cl(inp.i0).requires_grad_()
            state = HF.NeuronState(v0, i0)
            wrt += [v0, i0]
        addend = None
        if cs.addend:
            addend = F._cl(inp.addend).requires_grad_()
            wrt.append(addend)
        prm = params_of(HF, row.rule)
        out, st = HF.affine_neuron(y, cs.neuron, state, bn=bn, params=prm, addend=addend, spikes_ok=cs.spikes_ok,
                                   tau=(w_mem, w_syn))
        if cs.spikes_ok:
            thr = getattr(out, "_snn_spike_threshold", None)
            assert thr is not None, "spikes_ok: the layer wrote a spike tensor"
            z = (out.detach() > thr).to(D)
        elif cs.addend:
            z = ((out.detach() - addend.detach()) > 0.5).to(D)
        else:
            z = out.detach().to(D)
            assert bool(((z == 0) | (z == 1)).all())
        n_wrt = len(wrt)
        if learn:
            wrt += [w_mem, w_syn]
        gr = torch.autograd.grad([out, st.v, st.i], wrt, [F._cl(inp.g_out), F._cl(inp.g_vT), F._cl(inp.g_iT)],
                                 allow_unused=True)
        torch.cuda.synchronize()
        names = ["dy"] + (["dgamma", "dbias"] if bn is not None else []) + (["dv0", "di0"] if cs.state else []) + \
                (["daddend"] if cs.addend else [])
        grads = {k: v.detach().to(D) for k, v in zip(names, gr[:n_wrt])}
        tau_grads = {}
        if learn:
            tau_grads = {"w_mem": gr[n_wrt], "w_syn": gr[n_wrt + 1]}
        res = F.DevResult(z, z, st.v.detach().to(D), st.i.detach().to(D),
                          None if bn is None else bn.running_mean.detach().to(D),
                          None if bn is None else bn.running_var.detach().to(D), grads, True)
        bits = {"out": out.detach().clone(), "vT": st.v.detach().clone(), "iT": st.i.detach().clone(),
                "dy": gr[0].detach().clone()}
        return res, tau_grads, (c_mem.cpu(), c_syn.cpu()), bits


def plan_of(HF, row, with_tau=True):
    from snn_for_object_detection_amd import _hip
    cs = row.cs
    flags = _hip.SCAN_WIDE_ADDRESSING if row.variant == "wide" else 0
    return HF.lif_tau_bwd_plan(cs.T, cs.B * cs.H * cs.W, cs.C, cs.C, cs.C, cs.bn is not None, with_tau, flags,
                               params=params_of(HF, row.rule))


# ------------------------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("row", TC.ROWS, ids=[r.cs.id for r in TC.ROWS])
def test_tau_against_fp64(HF, row):
    cs = row.cs
    tp = plan_of(HF, row)
    got = F.plan_classes(tp.scan)
    assert set(row.classes) <= got, (cs.id, tp, got)
    assert tp.ordered == row.ordered and tp.scan.buf == (0 if (row.variant == "wide" or tp.scan.vec == 1) else 1)
    if row.multi_pixel:
        # three pixels per thread with the two sums (four without them), several groups per block, the last one partial
        assert (tp.scan.buf, tp.scan.np) == (1, 3) and tp.scan.rpb > 3 and tp.scan.rpb % 3 != 0 and tp.scan.gx > 1, tp
        assert plan_of(HF, row, with_tau=False).scan.np == 4
    inp = TC.make_inputs(cs)
    res, tau_grads, (c_mem, c_syn), _ = run_device(HF, row, inp)
    want_c = TC.host_constants(row)
    assert torch.allclose(c_mem, want_c[0], rtol=1e-6, atol=0) and torch.allclose(c_syn, want_c[1], rtol=2e-6, atol=0)
    z = res.z.cpu()
    assert 0.02 < float(z.mean()) < 0.9
    ref = TC.run_ref(row, inp, z, c_mem, c_syn)
    fails, rec = [], {"plan": list(tp.scan)}
    TG.check_forward(res, ref.ref, 1.0, fails, rec)
    F.check_grads(cs, res, ref.ref, fails, rec)
    yard = TC.yardstick(row, inp, z, c_mem, c_syn, ref)
    for name, r, y_ in (("w_mem", ref.d_wmem, yard[0]), ("w_syn", ref.d_wsyn, yard[1])):
        g = tau_grads[name]
        assert g is not None and tuple(g.shape) == tuple(r.shape) == ((1,) if row.learn == "layer" else (cs.C,))
        e = TC.rel_err(g, r)
        rec[name] = (e, y_)
        print(f"TAU {cs.id} dL/d{name}: kernel {e:.3g} yardstick {y_:.3g} ratio {e / y_:.3g}")
        if not e <= TC.TAU_FACTOR * y_:
            fails.append(f"dL/d{name}: ||d - r|| / ||r|| = {e:.3g} > 16 x {y_:.3g} (the float32 restatement's)")
    print(f"{cs.id}: {rec}")
    assert not fails, f"{cs.id}:\n  " + "\n  ".join(fails)


def test_ordered_plan_is_reproducible(HF):
    row = TC.ROWS[4]   # 512 channels: three pixel blocks, eight channel blocks, four waves each
    assert plan_of(HF, row).ordered == 1 and plan_of(HF, row).scan.gx > 1
    inp = TC.make_inputs(row.cs)
    _, a, _, bits_a = run_device(HF, row, inp)
    _, b, _, bits_b = run_device(HF, row, inp)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for k in bits_a:
        assert torch.equal(bits_a[k], bits_b[k]), k


def test_gradients_accumulate_into_a_written_slot(HF):
    """Slots that already hold data: the finalize adds (accumulate flag from ``claim()``), autograd receives nothing."""
    row = TC.ROWS[0]
    inp = TC.make_inputs(row.cs)
    _, plain, _, _ = run_device(HF, row, inp)
    held = [torch.linspace(-1.0, 2.0, row.cs.C).cuda(), torch.linspace(3.0, -1.0, row.cs.C).cuda()]
    slots = [HF.GradSlot(h.clone()) for h in held]
    for s in slots:
        s.written = True
    _, got, _, _ = run_device(HF, row, inp, slots=slots)
    assert got["w_mem"] is None and got["w_syn"] is None
    assert torch.equal(slots[0].buf, held[0] + plain["w_mem"]) and torch.equal(slots[1].buf, held[1] + plain["w_syn"])
    fresh = [HF.GradSlot(torch.full((row.cs.C,), float("nan")).cuda()) for _ in range(2)]
    run_device(HF, row, inp, slots=fresh)
    assert fresh[0].written and torch.equal(fresh[0].buf, plain["w_mem"]) and torch.equal(fresh[1].buf, plain["w_syn"])


def test_fixed_per_channel_constants_need_no_sums(HF):
    """Raw parameters that require no gradient: same forward and dy bit for bit, no gradient for them."""
    row = TC.ROWS[0]
    inp = TC.make_inputs(row.cs)
    _, _, _, bits = run_device(HF, row, inp)
    _, tau_grads, _, bits_fixed = run_device(HF, row, inp, learn=False)
    assert tau_grads == {}
    for k in bits:
        assert torch.equal(bits[k], bits_fixed[k]), k


def test_scalar_tau_travels_in_the_struct(HF):
    """LIF(tau_mem=...) without learn_tau runs the kernels that exist today: equal, bit for bit, to per-channel arrays that
    hold the struct's two values in every channel."""
    from snn_for_object_detection_amd import _hip
    row = TC.ROWS[5]
    cs, inp = row.cs, TC.make_inputs(row.cs)
    prm = HF.neuron_params(tau_mem=5e-3, tau_syn=4e-3)      # c_mem = 0.2, c_syn = -0.25

    def run(tau):
        from snn_for_object_detection_amd.layer_gen import HipBatchNorm2d
        bn = HipBatchNorm2d(cs.C).cuda().train()
        with torch.no_grad():
            bn.weight.copy_(inp.gamma)
            bn.bias.copy_(inp.bias)
        y = F._cl(inp.y).requires_grad_()
        out, st = HF.affine_neuron(y, _hip.NEURON_LIF, None, bn=bn, params=prm, tau=tau)
        (dy,) = torch.autograd.grad(out, y, F._cl(inp.g_out))
        torch.cuda.synchronize()
        return out.detach(), st.v.detach(), st.i.detach(), dy

    # (the y-reading scan on both sides: the from-state statistic associates differently)
    with HF.levers(USE_SUMS_FROM_STATE=False):
        a = run(None)
    # raw values whose sigmoid is not exactly the struct's constant would differ: hand the kernel the constants themselves
    saved = HF.lif_time_constants
    HF.lif_time_constants = lambda w_mem, w_syn, C: (torch.full((C,), prm.c_mem).cuda(), torch.full((C,), prm.c_syn).cuda())
    try:
        b = run((torch.zeros(1).cuda(), torch.zeros(1).cuda()))
    finally:
        HF.lif_time_constants = saved
    assert 0.02 < float(a[0].mean()) < 0.9
    for x, y_ in zip(a, b):
        assert torch.equal(x, y_)


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_by_name(HF):
    """Error paths only: each is raised before anything is launched."""
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd import _hip
    w = (torch.zeros(8).cuda().requires_grad_(), torch.zeros(8).cuda().requires_grad_())
    y16 = torch.randn(4, 2, 8, 6, 6, device="cuda").to(torch.bfloat16).requires_grad_()
    with pytest.raises(RuntimeError, match="bf16 storage"):
        HF.affine_neuron(y16, _hip.NEURON_LIF, None, bn=None, tau=w)
    y = torch.randn(4, 2, 8, 6, 6, device="cuda").requires_grad_()
    with pytest.raises(RuntimeError, match="LIF layers"):
        HF.affine_neuron(y, _hip.NEURON_LI, None, bn=None, params=S.LICell().params, tau=w)
    with pytest.raises(RuntimeError, match="checkpointed"):
        HF._tau_refusal(_hip.NEURON_LIF, False, True)
    with pytest.raises(ValueError, match="tau_mem"):
        HF.neuron_params(tau_mem=5e-4)        # dt / tau_mem = 2
    with pytest.raises(ValueError, match="tau_mem"):
        S.LIF(tau_mem=5e-4, learn_tau="channel")
    # a learnable Norm -> LIF sequence longer than one scan segment: the look-back of the two sums is not built
    bn = S.HipBatchNorm2d(8).cuda().train()
    y_long = torch.randn(HF.SCAN_SEGMENT_T + 1, 1, 8, 5, 6, device="cuda").requires_grad_()
    with pytest.raises(RuntimeError, match="segment"):
        HF.affine_neuron(y_long, _hip.NEURON_LIF, None, bn=bn, tau=w)
    torch.cuda.synchronize()


def test_checkpoint_lever_leaves_the_layer_on_the_plain_scan(HF):
    row = TC.ROWS[0]
    inp = TC.make_inputs(row.cs)
    _, a, _, bits_a = run_device(HF, row, inp)
    with HF.levers(LIF_CHECKPOINT_BYTES=0):
        _, b, _, bits_b = run_device(HF, row, inp)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for k in bits_a:
        assert torch.equal(bits_a[k], bits_b[k]), k


# ------------------------------------------------------------------------------------------------------ model level
def _block(S):
    return S.BlockGen(2, [S.Conv(8, 3), S.Norm(), S.LIF(learn_tau="channel"), S.Conv(8, 3), S.Norm(), S.LIF(tau_mem=2e-2)])


def test_blockgen_trains_its_time_constants(HF):
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd.trainer import FlatTrainer
    torch.manual_seed(3)
    blk = _block(S).cuda().train()
    plain = S.BlockGen(2, [S.Conv(8, 3), S.Norm(), S.LIF(), S.Conv(8, 3), S.Norm(), S.LIF()])
    new = [k for k in blk.state_dict() if k not in plain.state_dict()]
    assert len(new) == 2 and sorted(k.rsplit(".", 1)[1] for k in new) == ["w_mem", "w_syn"]
    assert set(plain.state_dict()) < set(blk.state_dict())
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.fill_(4.0)     # (unit gain leaves four steps too short to reach the threshold)
    cells = [m for m in blk.modules() if isinstance(m, S.LIFCell)]
    assert cells[0].tau is not None and cells[1].tau is None and cells[1].params.c_mem == pytest.approx(0.05)
    tr = FlatTrainer(blk, lr=1e-2)
    taus = [cells[0].w_mem, cells[0].w_syn]
    before = [p.detach().clone() for p in taus]
    X = F._cl((torch.rand(4, 2, 2, 12, 16) < 0.4).float())
    out, _ = blk(X)
    assert 0.02 < float(out.detach().mean()) < 0.98
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(1))
    out.backward(F._cl(g))
    torch.cuda.synchronize()
    for p in taus:
        slot = p._snn_grad_slot
        assert p.grad is None and slot.written
        assert bool(torch.isfinite(slot.buf).all()) and float(slot.buf.abs().sum()) > 0
    tr.step()
    torch.cuda.synchronize()
    for p, b in zip(taus, before):
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), b)
    # the state round-trips
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    other = _block(S).cuda()
    other.load_state_dict(sd)
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_tiny_yolo_with_learnable_time_constants(HF):
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd.trainer import FlatTrainer
    from tests.util import synthetic_events, synthetic_labels
    torch.manual_seed(11)
    keys = set(S.TinyYolo(num_classes=2, time_window=0).state_dict())
    model = S.TinyYolo(num_classes=2, time_window=0)
    n0 = len(list(model.parameters()))
    n = S.set_lif_time_constants(model, learn_tau="channel")
    assert n == sum(isinstance(m, S.LIFCell) for m in model.modules()) > 0
    assert len(list(model.parameters())) == n0 + 2 * n
    assert keys < set(model.state_dict())
    model = model.to("cuda:0").train()
    tr = FlatTrainer(model, lr=1e-3)
    X, labels = synthetic_events(3, 1, 64, 64, p=0.08), synthetic_labels(1)
    loss = model.training_step((X.to("cuda:0"), labels.to("cuda:0")))
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss.detach()))
    cells = [m for m in model.modules() if isinstance(m, S.LIFCell)]
    for c in cells:
        for p in (c.w_mem, c.w_syn):
            assert p.is_cuda and p.grad is None and p._snn_grad_slot.written
            assert bool(torch.isfinite(p._snn_grad_slot.buf).all())
    assert any(float(c.w_mem._snn_grad_slot.buf.abs().sum()) > 0 for c in cells)
    tr.step()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
