"""Host-side checks of the selectable LIF backward rule: the reference's surrogates against closed forms, that the inputs
of tests/test_gpu_lif_gradient.py (tests/lif_gradient_cases.py) tell the rules apart, argument validation, ``set_lif_gradient`` and the struct layout."""
import ctypes
import math

import pytest
import torch

from tests import lif_gradient_ref as L
from tests import lif_gradient_cases as G

D = torch.float64


# ------------------------------------------------------------------------------------------------------ surrogates
@pytest.mark.parametrize("a", [100.0, 200.0, 7.5])
def test_surrogates_against_closed_forms(a):
    """s(u) at u = k / a, k in {0, +-1/2, +-1, +-3}: every value below is the table of include/snn_hip.h worked by hand."""
    ks = [0.0, 0.5, -0.5, 1.0, -1.0, 3.0, -3.0]
    u = torch.tensor([k / a for k in ks], dtype=D)
    sig = lambda x: 1.0 / (1.0 + math.exp(-x))   # noqa: E731
    want = {
        "super": [1.0, 4.0 / 9.0, 4.0 / 9.0, 0.25, 0.25, 1.0 / 16.0, 1.0 / 16.0],
        "triangle": [1.0, 0.5, 0.5, 0.0, 0.0, 0.0, 0.0],
        "sigmoid": [4.0 * sig(k) * (1.0 - sig(k)) for k in ks],
        "atan": [1.0, 0.8, 0.8, 0.5, 0.5, 0.1, 0.1],
    }
    assert want["sigmoid"][0] == 1.0 and want["sigmoid"][3] == pytest.approx(0.7864477329659274, rel=1e-15)
    assert want["sigmoid"] == pytest.approx([1.0 / math.cosh(k / 2.0) ** 2 for k in ks], rel=1e-14)   # = sech^2(x / 2)
    for name, fn in L.SURROGATES.items():
        got = fn(u, a)
        assert torch.allclose(got, torch.tensor(want[name], dtype=D), rtol=1e-13, atol=1e-15), (name, got)
        # ... and it is what the forced spike of that name hands back
        uu = u.clone().requires_grad_()
        z = L.FORCED_SPIKE[name].apply(uu, (uu > 0).to(D), a)
        (g,) = torch.autograd.grad(z, uu, torch.full_like(uu, 3.0))
        assert torch.allclose(g, 3.0 * got, rtol=1e-15, atol=0.0), name


def test_detached_reset_drops_the_reset_term():
    """One step by hand: g_vd = g_v (1 - z) + (g_out + g_v (v_reset - v_dec)) s, detached: g_v (1 - z) + g_out s."""
    x = torch.tensor([[[[[12.0, 3.0]]]]], dtype=D).requires_grad_()   # v_dec = 0.1 x: one neuron above, one below v_th
    z = torch.tensor([[[[[1.0, 0.0]]]]], dtype=D)
    g_out, g_v = 0.7, -1.3
    for name, fn in L.SURROGATES.items():
        for detached in (False, True):
            r = L.lif_scan(x, z, surrogate=name, alpha=G.SLOPE[name], detach_reset=detached)
            (gx,) = torch.autograd.grad([r.out, r.vT], [x], [torch.full_like(r.out, g_out), torch.full_like(r.vT, g_v)])
            v_dec = 0.1 * x.detach().flatten()
            s = fn(v_dec - 1.0, G.SLOPE[name])
            gz = g_out + (0.0 if detached else 1.0) * g_v * (0.0 - v_dec)
            want = 0.1 * (g_v * (1.0 - z.flatten()) + gz * s)      # dv_dec/dx = c_mem (g_iT = 0)
            assert torch.allclose(gx.flatten(), want, rtol=1e-6), (name, detached)   # (c_mem is the fp32 0.1)


# ------------------------------------------------------------------------------------------------------ inputs
_ROWS = [pytest.param(row, v_th, id=row.cs.id) for row in G.ROWS for v_th in row.v_ths]


@pytest.mark.parametrize("row, v_th", _ROWS)
def test_inputs_tell_the_rules_apart(row, v_th):
    """On the inputs of the GPU test, the reference's dy under two different rules differs by >= 10x the bound the GPU test
    holds the kernel to (same norm, same grouping, same scale): every non-default rule against the default one, and
    every detached rule against its non-detached twin."""
    cs = row.cs
    inp = G.make_inputs(cs)
    z = G.reference_spikes(cs, inp, v_th)
    assert 0.02 < float(z.mean()) < 0.9, "the layer hardly spikes (or always does)"
    refs = {}

    def ref(rule):
        if rule not in refs:
            refs[rule] = G.run_ref(cs, inp, z, rule, v_th)
        return refs[rule]

    for rule in row.rules:
        if rule != L.DEFAULT_RULE:
            d = G.dy_distance(cs, ref(rule), ref(L.DEFAULT_RULE))
            print(cs.id, rule, "against the default rule:", d)
            assert d >= 10.0, (cs.id, rule, "against the default rule", d)
        if rule[1]:
            d = G.dy_distance(cs, ref(rule), ref((rule[0], False)))
            print(cs.id, rule, "against its non-detached twin:", d)
            assert d >= 10.0, (cs.id, rule, "against its non-detached twin", d)


# ------------------------------------------------------------------------------------------------------ Python interface
def test_neuron_params_validation():
    from snn_for_object_detection_amd import _hip
    from snn_for_object_detection_amd import functional as HF
    with pytest.raises(ValueError, match="surrogate"):
        HF.neuron_params(surrogate="gauss")
    for alpha in (0.0, -1.0):
        with pytest.raises(ValueError, match="alpha"):
            HF.neuron_params(alpha=alpha)
    for v_reset in (1.0, 1.5):
        with pytest.raises(ValueError, match="v_reset"):
            HF.neuron_params(v_reset=v_reset)
    with pytest.raises(ValueError, match="v_reset"):
        HF.neuron_params(v_th=-0.1)
    p = HF.neuron_params(surrogate="atan", alpha=50.0, detach_reset=True, v_th=0.8, v_reset=-0.1, v_leak=0.05)
    assert (p.surrogate, p.reset_detached) == (_hip.SURR_ATAN, 1)
    assert (p.alpha, p.v_th, p.v_reset, p.v_leak) == tuple(
        torch.tensor([50.0, 0.8, -0.1, 0.05], dtype=torch.float32).tolist())
    d = HF.neuron_params()
    assert (d.surrogate, d.reset_detached, d.alpha, d.v_th, d.v_reset, d.v_leak) == (0, 0, 100.0, 1.0, 0.0, 0.0)
    assert [HF.SURROGATES[n] for n in L.SURROGATE_NAMES] == [0, 1, 2, 3]


def test_layer_generators_take_the_keywords():
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd import functional as HF
    assert bytes(S.LIFCell().params) == bytes(HF.neuron_params()) == bytes(S.LIF().get(4)[0].params)
    kw = dict(surrogate="triangle", detach_reset=True, v_th=0.8)
    cell, ch = S.LIF(**kw).get(4)
    assert ch == 4 and isinstance(cell, S.LIFCell) and bytes(cell.params) == bytes(HF.neuron_params(**kw))
    stored, _ = S.LIF(state_storage=True, alpha=25.0).get(4)
    assert isinstance(stored, S.StateStorage) and stored.module.params.alpha == 25.0
    assert bytes(S.LIFCell(dt=0.002, **kw).params) == bytes(HF.neuron_params(0.002, **kw))
    with pytest.raises(ValueError, match="surrogate"):
        S.LIF(surrogate="gauss")
    with pytest.raises(TypeError):
        S.LIF(slope=3.0)
    assert list(S.LIFCell(**kw).state_dict()) == [] and list(S.LIFCell(**kw).buffers()) == []


def test_set_lif_gradient_on_tiny_yolo():
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd import _hip
    m = S.TinyYolo(num_classes=2, time_window=0)
    keys = list(m.state_dict())
    tree = [type(x).__name__ for x in m.modules()]
    cells = [x for x in m.modules() if isinstance(x, S.LIFCell)]
    wrapped = [x for x in m.modules() if isinstance(x, S.StateStorage) and isinstance(x.module, S.LIFCell)]
    before = [bytes(c.params) for c in cells]
    assert S.set_lif_gradient(m) == len(cells) == 19
    assert [bytes(c.params) for c in cells] == before       # None leaves every field as it is
    assert S.set_lif_gradient(m, surrogate="atan", detach_reset=True) == len(cells)
    assert all((c.params.surrogate, c.params.reset_detached, c.params.alpha) == (_hip.SURR_ATAN, 1, 100.0) for c in cells)
    assert all(w.module.params.surrogate == _hip.SURR_ATAN for w in wrapped)
    assert S.set_lif_gradient(m, alpha=40.0) == len(cells)
    assert all((c.params.surrogate, c.params.reset_detached, c.params.alpha) == (_hip.SURR_ATAN, 1, 40.0) for c in cells)
    assert S.set_lif_gradient(m, detach_reset=False) == len(cells) and all(c.params.reset_detached == 0 for c in cells)
    li = [x for x in m.modules() if isinstance(x, S.LICell)]
    assert li and all(c.params.surrogate == 0 and c.params.alpha == 100.0 for c in li)   # LIF cells only
    assert list(m.state_dict()) == keys and [type(x).__name__ for x in m.modules()] == tree
    with pytest.raises(ValueError, match="surrogate"):
        S.set_lif_gradient(m, surrogate="gauss")
    with pytest.raises(ValueError, match="alpha"):
        S.set_lif_gradient(m, alpha=0.0)


def test_ctypes_layout():
    from snn_for_object_detection_amd import _hip
    assert ctypes.sizeof(_hip.NeuronParams) == 13 * 4
    assert [n for n, _ in _hip.NeuronParams._fields_][-2:] == ["surrogate", "reset_detached"]
    assert _hip.NeuronParams.surrogate.offset == 44 and _hip.NeuronParams.reset_detached.offset == 48
    old = _hip.NeuronParams(0.1, -0.2, 0.0, 1.0, 0.0, 100.0, 1.0, 1000.0, 200.0, 0.001, 0.0)   # the 11 values of ABI 19
    assert (old.surrogate, old.reset_detached) == (0, 0)
    assert _hip.ABI_VERSION == 20


def test_planner_accepts_and_refuses_rules(hip_lib):
    """Host-only plan queries: the general rule takes the default rule's plan; what is not covered is refused by name."""
    from snn_for_object_detection_amd import _hip
    from snn_for_object_detection_amd import functional as HF
    d = HF.neuron_params()
    g = HF.neuron_params(surrogate="sigmoid", alpha=200.0, detach_reset=True)
    for T, M, C, sums, flags in [(8, 98, 4, True, 0), (6, 180, 3, True, 0), (8, 84, 16, False, 0),
                                 (32, 42, 512, True, 0), (6, 84, 16, True, _hip.SCAN_WIDE_ADDRESSING),
                                 (6, 84, 16, True, _hip.SCAN_LAST_STEP_ONLY)]:
        assert (HF.affine_neuron_bwd_plan(_hip.NEURON_LIF, T, M, C, C, C, sums, flags, params=g)
                == HF.affine_neuron_bwd_plan(_hip.NEURON_LIF, T, M, C, C, C, sums, flags, params=d))
    q = hip_lib.snn_affine_neuron_bwd_sums_from_state
    assert q(_hip.NEURON_LIF, 32, 5 * 120 * 152, 64, 64, g, 0) == 1
    assert q(_hip.NEURON_LIF, 32, 5 * 120 * 152, 64, 64, g, _hip.SCAN_STATE_LOOKBACK) == 1
    bad = HF.neuron_params()
    bad.surrogate = 4
    assert q(_hip.NEURON_LIF, 32, 5 * 120 * 152, 64, 64, bad, 0) == 0
    for neuron, prm, flags, word in [(_hip.NEURON_LIF, bad, 0, "surrogate"), (_hip.NEURON_LI, g, 0, "LIF"),
                                     (_hip.NEURON_NONE, g, 0, "LIF"), (_hip.NEURON_LIF, g, _hip.SCAN_BF16_STORAGE, "bf16")]:
        with pytest.raises(RuntimeError, match=word):
            HF.affine_neuron_bwd_plan(neuron, 8, 98, 4, 4, 4, True, flags, params=prm)
    bad.surrogate = -1
    with pytest.raises(RuntimeError, match="surrogate"):
        HF.affine_neuron_bwd_plan(_hip.NEURON_LIF, 8, 98, 4, 4, 4, True, 0, params=bad)
