"""Host-side checks of the per-layer / learnable LIF time constants: ``neuron_params`` keywords, the layer generators and
``set_lif_time_constants``, the new C entry points and their refusals, and that the inputs of tests/test_gpu_lif_tau.py
(tests/lif_tau_cases.py) can tell a kernel that ignores the per-channel arrays, or returns zeros, from a right one."""
import re

import pytest
import torch

from tests import lif_gradient_cases as G
from tests import lif_tau_cases as TC
from tests import lif_tau_ref as TR
from tests.test_gpu_norm_neuron_fp64 import TOL_STATE, D  # noqa: F401

NEW_SYMBOLS = ("snn_lif_tau_param", "snn_lif_tau_fwd", "snn_lif_tau_bwd_partial_size", "snn_lif_tau_bwd_plan",
               "snn_lif_tau_bwd", "snn_lif_tau_finalize")


# ------------------------------------------------------------------------------------------------------ neuron_params
def test_defaults_are_the_13_words_of_today():
    from snn_for_object_detection_amd import _hip
    from snn_for_object_detection_amd import functional as HF
    literal = _hip.NeuronParams(0.1, -0.2, 0.0, 1.0, 0.0, 100.0, 1.0, 1000.0, 200.0, 0.001, 0.0)   # test_ctypes_layout's
    assert bytes(HF.neuron_params()) == bytes(literal) and len(bytes(literal)) == 13 * 4
    assert bytes(HF.neuron_params(tau_mem=1e-2, tau_syn=5e-3)) == bytes(literal)
    p = HF.neuron_params(tau_mem=2e-2, tau_syn=4e-3)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).item()   # noqa: E731
    assert p.c_mem == (0.001 * torch.as_tensor(1.0 / 2e-2)).item() == f32(0.05)
    assert p.c_syn == (-0.001 * torch.as_tensor(1.0 / 4e-3)).item() == f32(-0.25)
    other = bytes(p)
    assert other[8:] == bytes(literal)[8:] and other[:8] != bytes(literal)[:8]      # the two constants and nothing else
    assert _hip.ABI_VERSION == 20


def test_keyword_validation():
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd import functional as HF
    for bad in (5e-4, 0.0, -1e-2):                    # dt / tau_mem > 1, and no time constant at all
        with pytest.raises(ValueError, match="tau_mem"):
            HF.neuron_params(tau_mem=bad)
    for bad in (1e-3, 5e-4, 0.0, -5e-3):              # dt / tau_syn = 1 is refused too (the current would vanish in a step)
        with pytest.raises(ValueError, match="tau_syn"):
            HF.neuron_params(tau_syn=bad)
    assert HF.neuron_params(tau_mem=1e-3).c_mem == 1.0
    with pytest.raises(ValueError, match="tau_mem"):
        HF.neuron_params(0.05)                        # the default tau_mem at a coarse dt
    with pytest.raises(ValueError, match="tau_mem"):
        S.LIF(tau_mem=5e-4)
    with pytest.raises(ValueError, match="learn_tau"):
        S.LIF(learn_tau="pixel")
    with pytest.raises(ValueError, match="learn_tau"):
        S.LIFCell(learn_tau="neuron")
    with pytest.raises(ValueError, match="channel"):
        S.LIFCell(learn_tau="channel")                # no channel count
    with pytest.raises(TypeError):
        S.LIF(tau=1e-2)


# ------------------------------------------------------------------------------------------------------ layers
def test_cells_own_their_parameters():
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd import functional as HF
    plain, ch = S.LIF().get(8)
    assert ch == 8 and list(plain.parameters()) == [] and list(plain.buffers()) == [] and list(plain.state_dict()) == []
    assert plain.tau is None and plain.channels == 8 and bytes(plain.params) == bytes(HF.neuron_params())
    fixed, _ = S.LIF(tau_mem=2e-2).get(8)
    assert list(fixed.state_dict()) == [] and fixed.tau is None
    assert bytes(fixed.params) == bytes(HF.neuron_params(tau_mem=2e-2))
    cell, _ = S.LIF(learn_tau="channel", tau_mem=2e-2, v_th=0.8).get(8)
    assert list(cell.state_dict()) == ["w_mem", "w_syn"] and [tuple(p.shape) for p in cell.parameters()] == [(8,), (8,)]
    assert torch.allclose(torch.sigmoid(cell.w_mem), torch.full((8,), 0.05), rtol=1e-6)
    assert torch.allclose(torch.sigmoid(cell.w_syn), torch.full((8,), 0.8), rtol=1e-6)
    assert cell.params.v_th == pytest.approx(0.8)
    layer, _ = S.LIF(learn_tau="layer", state_storage=True).get(8)
    assert isinstance(layer, S.StateStorage) and [tuple(p.shape) for p in layer.parameters()] == [(1,), (1,)]
    assert cell.tau[0] is cell.w_mem and cell.tau[1] is cell.w_syn


def test_set_lif_time_constants_on_tiny_yolo():
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd import functional as HF
    base = S.TinyYolo(num_classes=2, time_window=0)
    keys = list(base.state_dict())
    tree = [type(x).__name__ for x in base.modules()]
    cells = [m for m in base.modules() if isinstance(m, S.LIFCell)]
    assert len(cells) == 19 and all(c.channels for c in cells) and not any(k.endswith(("w_mem", "w_syn")) for k in keys)
    assert all(list(c.parameters()) == [] for c in cells)
    # constants alone: no parameter, no key, the struct changes
    assert S.set_lif_time_constants(base, tau_mem=2e-2) == 19
    assert list(base.state_dict()) == keys and [type(x).__name__ for x in base.modules()] == tree
    assert all(bytes(c.params) == bytes(HF.neuron_params(tau_mem=2e-2)) for c in cells)
    li = [m for m in base.modules() if isinstance(m, S.LICell)]
    assert li and all(bytes(c.params) == bytes(HF.neuron_params()) for c in li)      # LIF cells only
    # learnable: two parameters per cell, StateStorage-wrapped cells included
    model = S.TinyYolo(num_classes=2, time_window=0)
    n0 = len(list(model.parameters()))
    assert S.set_lif_time_constants(model, learn_tau="channel") == 19
    assert len(list(model.parameters())) == n0 + 2 * 19
    new_keys = set(model.state_dict())
    assert set(keys) < new_keys and len(new_keys - set(keys)) == 2 * 19
    assert all(re.search(r"\.(w_mem|w_syn)$", k) for k in new_keys - set(keys))
    wrapped = [m for m in model.modules() if isinstance(m, S.StateStorage) and isinstance(m.module, S.LIFCell)]
    assert all(m.module.w_mem is not None for m in wrapped)
    for c in (m for m in model.modules() if isinstance(m, S.LIFCell)):
        assert tuple(c.w_mem.shape) == (c.channels,) == tuple(c.w_syn.shape)
    assert [type(x).__name__ for x in model.modules()] == tree
    with pytest.raises(ValueError, match="learn_tau"):
        S.set_lif_time_constants(model, learn_tau="pixel")
    with pytest.raises(ValueError, match="tau_syn"):
        S.set_lif_time_constants(model, tau_syn=1e-3)


# ------------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_are_declared_and_bound():
    import os
    from snn_for_object_detection_amd import _hip
    header = open(os.path.join(os.path.dirname(_hip.__file__), "..", "include", "snn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _hip.SIGNATURES, name
        assert re.search(r"\b" + name + r"\(", header), name
    assert "#define SNN_ABI_VERSION 20" in header


def test_plan_query_follows_the_plain_scan_and_refuses(hip_lib):
    from snn_for_object_detection_amd import _hip
    from snn_for_object_detection_amd import functional as HF
    for name in NEW_SYMBOLS:
        assert hasattr(hip_lib, name)
    g = HF.neuron_params(surrogate="atan", detach_reset=True)
    for T, M, C, sums, flags in [(8, 98, 4, True, 0), (6, 180, 3, True, 0), (8, 84, 16, False, 0), (6, 84, 24, True, 0),
                                 (32, 42, 512, True, 0), (6, 84, 16, True, _hip.SCAN_WIDE_ADDRESSING)]:
        for prm in (None, g):
            tp = HF.lif_tau_bwd_plan(T, M, C, C, C, sums, True, flags, params=prm)
            assert tp.scan == HF.affine_neuron_bwd_plan(_hip.NEURON_LIF, T, M, C, C, C, sums, flags)
            assert tp.ordered == (0 if tp.scan.mode == 2 else 1) and tp.lds_bytes >= tp.scan.lds_bytes
            if not sums:
                assert tp.lds_bytes > 0
        assert hip_lib.snn_lif_tau_bwd_partial_size(T, M, C, int(sums)) == tp.scan.gx * C * 2
    for kw, word in [(dict(neuron=_hip.NEURON_LI), "SNN_NEURON_LIF"), (dict(neuron=_hip.NEURON_NONE), "SNN_NEURON_LIF"),
                     (dict(flags=_hip.SCAN_BF16_STORAGE), "BF16_STORAGE"), (dict(flags=_hip.SCAN_LAST_STEP_ONLY), "LAST_STEP_ONLY"),
                     (dict(flags=_hip.SCAN_SUMS_FROM_STATE), "SUMS_FROM_STATE")]:
        with pytest.raises(RuntimeError, match=word):
            HF.lif_tau_bwd_plan(8, 98, 4, 4, 4, True, True, **kw)
    # without the sums of the constants, the last-step-only scan is the plain one's
    HF.lif_tau_bwd_plan(6, 84, 16, 16, 16, True, False, _hip.SCAN_LAST_STEP_ONLY)
    # the entry points refuse the same by name, before any launch (null pointers: nothing could be launched)
    prm = HF.neuron_params()
    rc = hip_lib.snn_lif_tau_fwd(_hip.NEURON_LI, None, 4, None, None, None, None, None, 4, None, 0, None, None, None, 8, 98, 4,
                                 prm, None, None, 0, None)
    assert rc != 0 and b"SNN_NEURON_LIF" in hip_lib.snn_last_error()
    rc = hip_lib.snn_lif_tau_fwd(_hip.NEURON_LIF, None, 4, None, None, None, None, None, 4, None, 0, None, None, None, 8, 98,
                                 4, prm, None, None, _hip.SCAN_BF16_STORAGE, None)
    assert rc != 0 and b"BF16_STORAGE" in hip_lib.snn_last_error()


def test_python_refusals_by_name():
    from snn_for_object_detection_amd import _hip
    from snn_for_object_detection_amd import functional as HF
    with pytest.raises(RuntimeError, match="LIF layers"):
        HF._tau_refusal(_hip.NEURON_LI, False, False)
    with pytest.raises(RuntimeError, match="bf16 storage"):
        HF._tau_refusal(_hip.NEURON_LIF, True, False)
    with pytest.raises(RuntimeError, match="checkpointed"):
        HF._tau_refusal(_hip.NEURON_LIF, False, True)
    HF._tau_refusal(_hip.NEURON_LIF, False, False)


# ------------------------------------------------------------------------------------------------------ inputs
@pytest.mark.parametrize("row", TC.ROWS, ids=[r.cs.id for r in TC.ROWS])
def test_inputs_can_tell_a_wrong_kernel(row):
    """On the inputs of the GPU rows, with the restatement's own spikes: the float32 restatement alone keeps its spike
    decisions inside the 1e-4 share; the two new gradients are at least 10x their bound away from zero; and per-channel
    constants move dy by at least 10x TOL_STATE (in check_grads' own measure) away from the scalar defaults'."""
    cs = row.cs
    inp = TC.make_inputs(cs)
    c_mem, c_syn = TC.host_constants(row)
    assert 0.0999 < float(c_mem.min()) and float(c_mem.max()) < 0.5001
    assert 0.4999 < float(1.0 + c_syn.min()) and float(1.0 + c_syn.max()) < 0.9501
    if row.learn == "channel":
        assert len(set(c_mem.tolist())) == cs.C == len(set(c_syn.tolist()))
    v0, i0 = TC.state_of(cs, inp)
    z, vd = TR.spikes_of(TC.neuron_input(cs, inp), c_mem.to(D), c_syn.to(D), v0, i0)
    assert 0.02 < float(z.mean()) < 0.9, "the layer hardly spikes (or always does)"
    v0f, i0f = TC.state_of(cs, inp, torch.float32)
    z32, _ = TR.spikes_of(TC.neuron_input(cs, inp, torch.float32), c_mem, c_syn, v0f, i0f)
    flips = z32.to(D) != z
    print(cs.id, "float32 restatement: spike flips", int(flips.sum()), "of", flips.numel())
    assert float(flips.double().mean()) <= 1e-4
    assert bool(((vd - 1.0).abs()[flips] <= 1e-5).all())
    ref = TC.run_ref(row, inp, z, c_mem, c_syn)
    y_mem, y_syn = TC.yardstick(row, inp, z, c_mem, c_syn, ref)
    print(cs.id, "yardstick (float32 restatement against float64): w_mem", y_mem, "w_syn", y_syn)
    for name, yard, g in (("w_mem", y_mem, ref.d_wmem), ("w_syn", y_syn, ref.d_wsyn)):
        assert float(g.norm()) > 0 and bool(torch.isfinite(g).all())
        assert 10.0 * TC.TAU_FACTOR * yard <= 1.0, (name, yard)      # ||dL/dw|| >= 10 x (16 x yardstick x ||dL/dw||)
    defaults = (torch.full((cs.C,), 0.1, dtype=torch.float32), torch.full((cs.C,), -0.2, dtype=torch.float32))
    ref_d = TC.run_ref(row, inp, z, *defaults)
    d = G.dy_distance(cs, ref.ref, ref_d.ref)
    print(cs.id, "dy against the scalar defaults:", d)
    assert d >= 10.0
