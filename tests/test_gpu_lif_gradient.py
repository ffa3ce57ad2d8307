"""The selectable LIF backward rule (surrogate x reset rule, ``snn_neuron_params.surrogate`` / ``.reset_detached``) against
the float64 restatement of tests/lif_gradient_ref.py, on every class of the reverse scan.

Every row of ROWS calls ``functional.affine_neuron`` forward and backward with a non-default rule, as
tests/test_gpu_norm_neuron_fp64.py does with the default one, and compares dy, dgamma, dbias, g_v0, g_i0 with the
reference.  The shapes are the smallest rows of that file's CASES that reach each scan class; the class is proven through
``affine_neuron_bwd_plan`` asked with the row's own (non-default) parameters.

Bounds: that file's, imported - ``TOL_STATE`` for the gradients with its norm-wise grouping, ``FWD_REL`` for the forward
values, spikes exact except within 1e-5 of the threshold and at most 1e-4 of the decisions.  ``TOL_STATE`` is derived there
from max |s'/s| <= 2 alpha = 200 of SuperSpike at alpha = 100; the slopes used here keep max |ds/du| <= 200 for every
surrogate (s <= 1): triangle |s'| = alpha = 100, atan max |s'| = 0.65 alpha = 65, sigmoid max |s'| = 0.77 alpha = 154
at alpha = 200, super 2 alpha = 200.

tests/test_lif_gradient_host.py checks, without a GPU, that on these very inputs the rules differ from one another by at
least 10x the bound - a kernel that ignored the rule could not pass.
"""
import copy

import pytest
import torch

from tests import lif_gradient_ref as L
from tests import test_gpu_norm_neuron_fp64 as F
from tests.lif_gradient_cases import ROWS, SLOPE, make_inputs, run_ref
from tests.test_gpu_norm_neuron_fp64 import FWD_REL, TOL_STATE, D  # noqa: F401  (the bounds of this file)

pytestmark = pytest.mark.gpu

PARAMS = [pytest.param(row, rule, v_th, id=f"{row.cs.id}-{rule[0]}{'-detached' if rule[1] else ''}")
          for row in ROWS for rule in row.rules for v_th in row.v_ths]


def params_of(HF, rule, v_th=1.0):
    return HF.neuron_params(surrogate=rule[0], alpha=SLOPE[rule[0]], detach_reset=rule[1], v_th=v_th)


@pytest.fixture(scope="module")
def HF(hip_lib):
    from snn_for_object_detection_amd import functional
    return functional


# ------------------------------------------------------------------------------------------------------ device run
def saved_potentials(out, y, cs):
    """The pre-reset potentials the forward saved for its backward: the one saved tensor laid out [T, B, H, W, C] that is
    not y's own memory (found by layout, not by its place in the list; run_device also checks that it gives the spikes)."""
    want = (cs.T, cs.B, cs.H, cs.W, cs.C)
    found = [t for t in out.grad_fn.saved_tensors
             if t is not None and tuple(t.shape) == want and t.dtype == torch.float32 and t.data_ptr() != y.data_ptr()]
    assert len(found) == 1, [None if t is None else tuple(t.shape) for t in out.grad_fn.saved_tensors]
    return found[0]


def run_device(HF, cs, inp, prm, variant="default", ckpt_bytes=None):
    """F.run_device for the rows of this file, with the layer's own parameters; also returns the saved potentials."""
    from snn_for_object_detection_amd import _hip
    from snn_for_object_detection_amd.layer_gen import HipBatchNorm2d
    with HF.levers(USE_SUMS_FROM_STATE=variant != "no_yfree", LIF_CHECKPOINT_BYTES=ckpt_bytes,
                   SCAN_FLAGS=_hip.SCAN_WIDE_ADDRESSING if variant == "wide" else 0):
        bn = None
        if cs.bn is not None:
            bn = HipBatchNorm2d(cs.C).cuda()
            with torch.no_grad():
                bn.weight.copy_(inp.gamma)
                bn.bias.copy_(inp.bias)
                bn.running_mean.copy_(inp.rm)
                bn.running_var.copy_(inp.rv)
            bn.train(cs.bn == "train")
        y = F._cl(inp.y).requires_grad_()
        wrt = [y] + ([bn.weight, bn.bias] if bn is not None else [])
        state = None
        if cs.state:
            v0, i0 = F._cl(inp.v0).requires_grad_(), F._cl(inp.i0).requires_grad_()
            state = HF.NeuronState(v0, i0)
            wrt += [v0, i0]
        out, st = HF.affine_neuron(y, cs.neuron, state, bn=bn, params=prm, last_only=cs.last_only, spikes_ok=cs.spikes_ok)
        vdec = saved_potentials(out, y, cs).detach().clone()
        if cs.spikes_ok:
            thr = getattr(out, "_snn_spike_threshold", None)
            assert thr is not None, "spikes_ok: the layer wrote a spike tensor"
            assert thr == pytest.approx(prm.v_th), "the consumer would threshold at another layer's v_th"
            raw = out.detach().clone()
            z = (raw > thr).to(D)
        else:
            raw = out.detach().clone()
            z = raw.to(D)
            assert bool(((z == 0) | (z == 1)).all())
        z_saved = (vdec > prm.v_th).permute(0, 1, 4, 2, 3).to(D)   # what was fetched IS the pre-reset potential
        assert torch.equal(z_saved[-1] if cs.last_only else z_saved, z), "the saved potentials do not give the spikes"
        outs, gouts = [out, st.v, st.i], [F._cl(inp.g_out), F._cl(inp.g_vT), F._cl(inp.g_iT)]
        gr = torch.autograd.grad(outs, wrt, gouts, allow_unused=True)
        names = ["dy"] + (["dgamma", "dbias"] if bn is not None else []) + (["dv0", "di0"] if cs.state else [])
        torch.cuda.synchronize()
        raw_grads = {k: v.detach().clone() for k, v in zip(names, gr)}
        res = F.DevResult(z, z, st.v.detach().to(D), st.i.detach().to(D),
                          None if bn is None else bn.running_mean.detach().to(D),
                          None if bn is None else bn.running_var.detach().to(D),
                          {k: v.to(D) for k, v in raw_grads.items()}, True)
        bits = {"out": raw, "vT": st.v.detach().clone(), "iT": st.i.detach().clone(), "vdec": vdec}
        return res, bits, raw_grads


# ------------------------------------------------------------------------------------------------------ checks
def check_forward(dev_res, ref, v_th, fails, rec):
    """F.check_forward for LIF, at the layer's own threshold."""
    z, vd = dev_res.z, ref.vdec.to(dev_res.z.device)
    if z.dim() == 4:   # last step only
        vd = vd[-1]
    mism = z != (vd > v_th).to(D)
    near = (vd - v_th).abs() <= 1e-5
    rec["spike_flips"] = int(mism.sum())
    if bool((mism & ~near).any()):
        fails.append(f"spikes: {int((mism & ~near).sum())} decisions differ away from the threshold")
    if mism.float().mean().item() > 1e-4:
        fails.append(f"spikes: {mism.float().mean().item():.3g} of the decisions flipped")
    F._elementwise("vT", dev_res.vT, ref.vT.to(z.device), None, fails, rec)
    F._elementwise("iT", dev_res.iT, ref.iT.to(z.device), None, fails, rec)
    if ref.rm is not None:
        F._elementwise("running_mean", dev_res.rm, ref.rm.to(z.device), None, fails, rec)
        F._elementwise("running_var", dev_res.rv, ref.rv.to(z.device), None, fails, rec)


def plan_of(HF, cs, prm, variant):
    from snn_for_object_detection_amd import _hip
    with_sums = cs.bn is not None
    segmented = with_sums and HF.SCAN_SEGMENT_T and cs.T > HF.SCAN_SEGMENT_T
    T = HF.SCAN_SEGMENT_T if segmented else cs.T
    flags = (_hip.SCAN_WIDE_ADDRESSING if variant == "wide" else 0) | (_hip.SCAN_LAST_STEP_ONLY if cs.last_only else 0)
    return HF.affine_neuron_bwd_plan(cs.neuron, T, cs.B * cs.H * cs.W, cs.C, cs.C, cs.C, with_sums, flags, params=prm), T, flags


@pytest.mark.parametrize("row, rule, v_th", PARAMS)
def test_rule_against_fp64(HF, row, rule, v_th):
    from snn_for_object_detection_amd import _hip
    cs = row.cs
    prm = params_of(HF, rule, v_th)
    inp = make_inputs(cs)
    ref = None
    for variant in row.variants:
        pl, T_seg, flags = plan_of(HF, cs, prm, variant)
        got = F.plan_classes(pl)
        assert set(row.classes) <= got, (cs.id, pl, got)
        if variant == "wide":
            assert pl.buf == 0
        M = cs.B * cs.H * cs.W
        covered = _hip.query("snn_affine_neuron_bwd_sums_from_state", cs.neuron, T_seg, M, cs.C, cs.C, prm, flags)
        if row.lookback:   # the segments behind the first one carry SNN_SCAN_STATE_LOOKBACK
            assert covered == 1 and cs.T > HF.SCAN_SEGMENT_T and HF.USE_SUMS_FROM_STATE
            assert _hip.query("snn_affine_neuron_bwd_sums_from_state", cs.neuron, T_seg, M, cs.C, cs.C, prm,
                              flags | _hip.SCAN_STATE_LOOKBACK) == 1
        res, bits, _ = run_device(HF, cs, inp, prm, variant)
        if ref is None:
            z = res.z.cpu()
            if cs.last_only:
                # the kernel returns the last step's spikes only: the steps before are in its saved potentials [T,B,H,W,C]
                z_all = (bits["vdec"] > prm.v_th).permute(0, 1, 4, 2, 3).to(D).cpu()
                assert torch.equal(z_all[-1], z)
                z = z_all
            ref = run_ref(cs, inp, z, rule, v_th)
        fails, rec = [], {"plan": list(pl)}
        check_forward(res, ref, v_th, fails, rec)
        F.check_grads(cs, res, ref, fails, rec)
        print(f"{cs.id} {rule} v_th={v_th} [{variant}]: {rec}")
        assert not fails, f"{cs.id} {rule} [{variant}]:\n  " + "\n  ".join(fails)


def test_forward_is_the_same_for_every_rule(HF):
    """Outputs, final state and saved potentials of every non-default rule are the default rule's, bit for bit - and a
    non-default rule with LIF_CHECKPOINT_BYTES set takes the plain scan (the checkpointed pair would refuse it)."""
    cs = ROWS[0].cs
    inp = make_inputs(cs)
    _, bits0, grads0 = run_device(HF, cs, inp, HF.neuron_params())
    for rule in L.RULES[1:]:
        prm = params_of(HF, rule)
        _, bits, grads = run_device(HF, cs, inp, prm)
        for k in bits0:
            assert torch.equal(bits[k], bits0[k]), (rule, k)
        assert not torch.equal(grads["dy"], grads0["dy"]), rule
        _, bits_c, grads_c = run_device(HF, cs, inp, prm, ckpt_bytes=0)
        for k in ("out", "vT", "iT"):
            assert torch.equal(bits_c[k], bits0[k]), (rule, k, "LIF_CHECKPOINT_BYTES")
        assert bits_c["vdec"].shape == bits0["vdec"].shape   # per-step potentials, not checkpoints
        for k in grads:
            assert torch.equal(grads_c[k], grads[k]), (rule, k, "LIF_CHECKPOINT_BYTES")


def test_rule_is_fixed_at_the_forward(HF):
    """The backward runs the rule the forward was called with, whatever happens to the struct in between."""
    cs = ROWS[0].cs
    inp = make_inputs(cs)
    prm = params_of(HF, ("atan", True))
    y = F._cl(inp.y).requires_grad_()
    out, _ = HF.affine_neuron(y, cs.neuron, None, bn=None, params=prm)
    prm.surrogate, prm.reset_detached = 0, 0
    (dy,) = torch.autograd.grad(out, y, F._cl(inp.g_out))
    prm = params_of(HF, ("atan", True))
    y2 = F._cl(inp.y).requires_grad_()
    out2, _ = HF.affine_neuron(y2, cs.neuron, None, bn=None, params=prm)
    (dy2,) = torch.autograd.grad(out2, y2, F._cl(inp.g_out))
    assert torch.equal(dy, dy2)


def test_explicit_defaults_change_nothing(HF):
    cs = ROWS[0].cs
    inp = make_inputs(cs)
    _, bits0, grads0 = run_device(HF, cs, inp, HF.neuron_params())
    explicit = HF.neuron_params(surrogate="super", alpha=100.0, detach_reset=False, v_th=1.0, v_reset=0.0, v_leak=0.0)
    assert bytes(explicit) == bytes(HF.neuron_params())
    _, bits, grads = run_device(HF, cs, inp, explicit)
    for k in bits0:
        assert torch.equal(bits[k], bits0[k]), k
    for k in grads0:
        assert torch.equal(grads[k], grads0[k]), k


def test_unknown_rule_and_other_neurons_are_refused(HF):
    from snn_for_object_detection_amd import _hip
    lib = _hip.load()
    bad = HF.neuron_params()
    bad.surrogate = 7
    with pytest.raises(RuntimeError, match="surrogate"):
        HF.affine_neuron_bwd_plan(_hip.NEURON_LIF, 8, 98, 4, 4, 4, True, 0, params=bad)
    prm = params_of(HF, ("triangle", True))
    with pytest.raises(RuntimeError, match="LIF"):
        HF.affine_neuron_bwd_plan(_hip.NEURON_LI, 8, 98, 4, 4, 4, True, 0, params=prm)
    with pytest.raises(RuntimeError, match="bf16"):
        HF.affine_neuron_bwd_plan(_hip.NEURON_LIF, 8, 98, 4, 4, 4, True, _hip.SCAN_BF16_STORAGE, params=prm)
    assert lib.snn_affine_neuron_bwd_sums_from_state(_hip.NEURON_LIF, 8, 98, 4, 4, bad, 0) == 0
    y = torch.randn(4, 2, 8, 6, 6, device="cuda").to(torch.bfloat16).requires_grad_()
    with pytest.raises(RuntimeError, match="triangle"):   # bf16 storage: refused in Python, before any launch
        HF.affine_neuron(y, _hip.NEURON_LIF, None, bn=None, params=prm)


def test_checkpointed_pair_refuses_a_non_default_rule(HF):
    """Host-side refusal of snn_lif_bwd_ckpt: return code and message, nothing launched."""
    from snn_for_object_detection_amd import _hip
    lib = _hip.load()
    T, M, C = 4, 8, 4
    t = [torch.zeros(T * M * C, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    for prm in (params_of(HF, ("atan", False)), params_of(HF, ("super", True))):
        rc = lib.snn_lif_bwd_ckpt(t[0].data_ptr(), C, t[1].data_ptr(), t[2].data_ptr(), C, None, None, None, None, 0,
                                  t[3].data_ptr(), None, None, None, T, M, C, prm, None)
        assert rc != 0
        msg = lib.snn_last_error()
        assert msg and b"snn_lif_bwd_ckpt" in msg and b"gradient rule" in msg
    torch.cuda.synchronize()
    assert float(t[3].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------------ model plumbing
def _grads_of(params):
    return [None if p.grad is None else p.grad.detach().clone() for p in params]


def test_blockgen_carries_the_layer_params(HF):
    """Conv -> Norm -> LIF(rule, v_th) twice as a BlockGen against the same operators chained by hand: bit-identical, and
    not what the default LIF gives."""
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd import _hip
    kw = dict(surrogate="triangle", detach_reset=True, v_th=0.8)
    torch.manual_seed(5)
    blk = S.BlockGen(2, [S.Conv(8, 1), S.Norm(), S.LIF(**kw), S.Conv(8, 1), S.Norm(), S.LIF(**kw)]).cuda().train()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                # BatchNorm's unit gain leaves four steps too short to reach the threshold (0.02 % of the last layer's
                # decisions are spikes); with gain 4 the float64 reference spikes at 13 % / 10 % in the two layers
                m.weight.fill_(4.0)
    hand = copy.deepcopy(blk)
    plain = S.BlockGen(2, [S.Conv(8, 1), S.Norm(), S.LIF(), S.Conv(8, 1), S.Norm(), S.LIF()]).cuda().train()
    plain.load_state_dict(blk.state_dict())
    assert list(plain.state_dict()) == list(blk.state_dict())
    X = (torch.rand(4, 2, 2, 8, 8) < 0.4).float()
    g = torch.randn(4, 2, 8, 8, 8)

    def run(fn, module):
        x = F._cl(X).requires_grad_()
        out = fn(x)
        out.backward(F._cl(g))
        torch.cuda.synchronize()
        return out.detach().clone(), x.grad.detach().clone(), _grads_of(module.parameters())

    def by_hand(x):
        conv1, bn1, lif1, conv2, bn2, lif2 = hand.net[0]
        assert lif1.params.v_th == pytest.approx(0.8) and lif1.params.surrogate == _hip.SURR_TRIANGLE
        prm = HF.neuron_params(**kw)
        assert bytes(prm) == bytes(lif1.params) == bytes(lif2.params)
        y = HF.conv2d(x, conv1.weight, 1, 0, bn_stats=True)
        a, _ = HF.affine_neuron(y, _hip.NEURON_LIF, None, bn=bn1, params=prm)
        y = HF.conv2d(a, conv2.weight, 1, 0, bn_stats=True)
        out, _ = HF.affine_neuron(y, _hip.NEURON_LIF, None, bn=bn2, params=prm)
        return out

    out_b, dx_b, gr_b = run(lambda x: blk(x)[0], blk)
    out_h, dx_h, gr_h = run(by_hand, hand)
    assert 0.02 < float(out_b.mean()) < 0.98, "the block's last layer does not spike: the comparison shows nothing"
    assert torch.equal(out_b, out_h) and torch.equal(dx_b, dx_h)
    for a, b in zip(gr_b, gr_h):
        assert torch.equal(a, b)
    out_p, dx_p, _ = run(lambda x: plain(x)[0], plain)
    assert not torch.equal(out_p, out_b)      # v_th = 0.8 reached the forward scan
    assert not torch.equal(dx_p, dx_b)


def test_tiny_yolo_switches_rule(HF):
    import snn_for_object_detection_amd as S
    from tests.util import synthetic_events, synthetic_labels
    X, labels = synthetic_events(3, 1, 64, 64, p=0.08), synthetic_labels(1)
    grads, losses = [], []
    for switch in (False, True):
        torch.manual_seed(11)
        model = S.TinyYolo(num_classes=2, time_window=0)
        keys = list(model.state_dict())
        if switch:
            n = S.set_lif_gradient(model, surrogate="atan", detach_reset=True)
            assert n == sum(isinstance(m, S.LIFCell) for m in model.modules()) > 0
            assert list(model.state_dict()) == keys
        model = model.to("cuda:0").train()
        loss = model.training_step((X.to("cuda:0"), labels.to("cuda:0")))
        loss.backward()
        torch.cuda.synchronize()
        gr = [p.grad.detach().clone() for p in model.parameters() if p.grad is not None]
        assert gr and all(bool(torch.isfinite(g).all()) for g in gr)
        grads.append(gr)
        losses.append(float(loss.detach()))
    assert losses[0] == pytest.approx(losses[1], rel=1e-5)     # the forward pass is the same
    assert len(grads[0]) == len(grads[1])
    assert any(not torch.equal(a, b) for a, b in zip(*grads))
