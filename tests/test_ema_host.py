"""Host side of the weight average (EMA) and the learning-rate schedule: what needs no GPU - the two new C-ABI symbols and
their refusals (they return before any launch), the decay ramp, ``warmup_cosine``, ``FlatTrainer``'s argument checks, the
in-place exchange of ``averaged_weights()`` on a CPU trainer, and the checkpoint formats (tests/test_gpu_ema.py has the
kernels and the training runs)."""
import ctypes
import math
import os
import re

import pytest
import torch

NEW_SYMBOLS = {"snn_adamax_step_ema": 17, "snn_ema_update": 6}


def _block(seed=1):
    import snn_for_object_detection_amd as S
    torch.manual_seed(seed)
    return S.BlockGen(2, [S.Conv(8, 3, 2), S.Norm(), S.LIF(), S.Conv(4, 1)])


def _trainer(model, **kw):
    from snn_for_object_detection_amd.trainer import FlatTrainer
    return FlatTrainer(model, lr=1e-3, **kw)


def _perturb_average(tr, seed=3):
    """Make the average differ from the live state everywhere (on the CPU nothing else would)."""
    g = torch.Generator().manual_seed(seed)
    tr.flat_ema.add_(torch.randn(tr.flat_ema.shape, generator=g))
    tr.ema_buffers.add_(torch.rand(tr.ema_buffers.shape, generator=g) + 0.5)


# ------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_are_declared_exported_and_bound(hip_lib):
    from snn_for_object_detection_amd import _hip
    header = open(os.path.join(os.path.dirname(_hip._HERE), "include", "snn_hip.h")).read()
    assert "#define SNN_ABI_VERSION 20" in header and _hip.ABI_VERSION == 20 and hip_lib.snn_abi_version() == 20
    declared = set(re.findall(r"\b(snn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name, n_args in NEW_SYMBOLS.items():
        assert name in declared, name
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name][1]) == n_args, name
        assert hasattr(raw, name), name
        fn = getattr(hip_lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _hip.SIGNATURES[name][1]
    # snn_adamax_step_ema is snn_adamax_step_ctl with the average behind the moments and its weight in front of ctl
    ctl_args, ema_args = _hip.SIGNATURES["snn_adamax_step_ctl"][1], _hip.SIGNATURES["snn_adamax_step_ema"][1]
    assert ema_args == ctl_args[:4] + [ctypes.c_void_p] + ctl_args[4:13] + [ctypes.c_float] + ctl_args[13:]


def test_profiler_labels_and_traffic():
    from snn_for_object_detection_amd.profiler import work_of
    label, _, byts = work_of("snn_adamax_step_ema", (1, 2, 3, 4, 5, 1000, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 0.0, 0.0, 0.5,
                                                     None, 0))
    assert (label, byts) == ("k_adamax_ema", 36.0 * 1000)
    label, _, byts = work_of("snn_ema_update", (1, 2, 1000, 0.5, None, 0))
    assert (label, byts) == ("k_ema_update", 12.0 * 1000)


def test_refusals_return_before_any_launch(hip_lib):
    """A null pointer, n <= 0 and an ema_weight outside (0, 1] are refused on the host: no device is needed, and the
    message names the argument."""
    host = (ctypes.c_float * 8)()
    a = ctypes.addressof(host)      # never dereferenced: every call below is refused first
    hyper = (1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 0.0, 0.0)

    def step(param=a, grad=a, exp_avg=a, exp_inf=a, ema=a, n=8, w=0.5):
        rc = hip_lib.snn_adamax_step_ema(param, grad, exp_avg, exp_inf, ema, n, *hyper, w, None, None)
        return rc, hip_lib.snn_last_error().decode()

    def update(ema=a, src=a, n=8, w=0.5):
        rc = hip_lib.snn_ema_update(ema, src, n, w, None, None)
        return rc, hip_lib.snn_last_error().decode()

    for name in ("param", "grad", "exp_avg", "exp_inf", "ema"):
        rc, msg = step(**{name: None})
        assert rc != 0 and msg.startswith("snn_adamax_step_ema") and re.search(rf"\b{name}\b", msg), (name, msg)
    for name in ("ema", "src"):
        rc, msg = update(**{name: None})
        assert rc != 0 and msg.startswith("snn_ema_update") and re.search(rf"\b{name}\b", msg), (name, msg)
    for call, prefix in ((step, "snn_adamax_step_ema"), (update, "snn_ema_update")):
        for n in (0, -4):
            rc, msg = call(n=n)
            assert rc != 0 and msg.startswith(prefix) and re.search(r"\bn\b", msg), (n, msg)
        for w in (0.0, -0.25, 1.0 + 2.0 ** -20, 2.0, float("nan"), float("inf")):
            rc, msg = call(w=w)
            assert rc != 0 and msg.startswith(prefix) and "ema_weight" in msg, (w, msg)


# ------------------------------------------------------------------------------------------ schedules
def test_decay_ramp():
    tr = _trainer(_block(), ema_decay=0.9999, ema_warmup=2000)
    assert tr.ema_decay_at(2000) == 0.9999 * (1.0 - math.exp(-1.0))
    values = [tr.ema_decay_at(k) for k in range(1, 40001, 37)]
    assert all(0 < a < b for a, b in zip(values, values[1:])) and values[-1] < 0.9999
    assert tr.ema_decay_at(10 ** 9) == 0.9999
    flat = _trainer(_block(), ema_decay=0.5, ema_warmup=0)
    assert [flat.ema_decay_at(k) for k in (1, 2, 1000)] == [0.5, 0.5, 0.5]
    assert _trainer(_block(), ema_decay=0.0).ema_decay_at(5) == 0.0
    with pytest.raises(RuntimeError, match="ema_decay"):
        _trainer(_block()).ema_decay_at(1)


def test_warmup_cosine_at_its_corners():
    from snn_for_object_detection_amd.trainer import warmup_cosine
    sched = warmup_cosine(2e-3, warmup_steps=10, total_steps=110, final_ratio=0.01)
    assert sched(0) == 2e-3 / 10                       # linear from base_lr / warmup_steps ...
    assert sched(4) == 2e-3 * 5 / 10
    assert sched(9) == 2e-3                            # ... up to base_lr
    assert sched(10) == 2e-3                           # the cosine starts there
    assert abs(sched(60) - 2e-3 * (0.01 + 0.99 * 0.5)) < 1e-18   # half way: the mean of both ends
    assert abs(sched(110) - 2e-5) < 1e-18 and sched(500) == sched(110)
    values = [sched(k) for k in range(10, 111)]
    assert all(a >= b for a, b in zip(values, values[1:]))
    assert warmup_cosine(1e-3, 0, 10)(0) == 1e-3       # no warmup: the cosine from step 0
    for bad in ((1e-3, 10, 10), (1e-3, -1, 10), (0.0, 1, 10), (1e-3, 1, 10, 1.5)):
        with pytest.raises(ValueError):
            warmup_cosine(*bad)


def test_lr_schedule_is_written_as_a_number_and_survives_a_load():
    from snn_for_object_detection_amd.trainer import warmup_cosine
    sched = warmup_cosine(1e-3, 4, 20)
    tr = _trainer(_block())
    assert tr.state_dict()["param_groups"][0]["lr"] == 1e-3      # a float: as before
    tr.lr = sched
    sd = tr.state_dict()
    assert sd["param_groups"][0]["lr"] == sched(0)
    torch.optim.Adamax(_block().parameters()).load_state_dict(sd)   # torch's format: a number
    tr.load_state_dict(sd)
    assert tr.lr is sched
    other = _trainer(_block())
    other.load_state_dict(sd)
    assert other.lr == sched(0)


# ------------------------------------------------------------------------------------------ the trainer
def test_constructor_checks_and_defaults():
    for kw in ({"ema_decay": 1.0}, {"ema_decay": -0.1}, {"ema_decay": float("nan")}, {"ema_decay": 1.5},
               {"ema_decay": 0.9, "ema_warmup": -1}, {"ema_decay": 0.9, "ema_warmup": 1.5}):
        with pytest.raises(ValueError):
            _trainer(_block(), **kw)
    tr = _trainer(_block())
    assert tr.ema_decay is None and tr.flat_ema is None and tr.ema_buffers is None and tr.ema_updates == 0
    for call in (tr.reset_ema, lambda: tr.averaged_weights().__enter__(), lambda: tr.ema_state_dict(_block())):
        with pytest.raises(RuntimeError, match="ema_decay"):
            call()
    model = _block()
    tr = _trainer(model, ema_decay=0.999, ema_warmup=10)
    assert (tr.ema_decay, tr.ema_warmup, tr.ema_updates) == (0.999, 10, 0)
    assert tr.flat_ema.shape == tr.flat_param.shape and torch.equal(tr.flat_ema, tr.flat_param)
    assert tr.flat_ema.data_ptr() != tr.flat_param.data_ptr()
    live = torch.cat([b.reshape(-1).float() for b in model.buffers() if b.is_floating_point()])
    assert live.numel() == 16 and tr.ema_buffers.dtype == torch.float32 and torch.equal(tr.ema_buffers, live)


def test_averaged_weights_exchanges_in_place_and_restores_every_bit():
    model = _block()
    tr = _trainer(model, ema_decay=0.99)
    _perturb_average(tr)
    float_buffers = [b for b in model.buffers() if b.is_floating_point()]
    int_buffers = [b for b in model.buffers() if not b.is_floating_point()]
    assert float_buffers and int_buffers
    live_p, live_b = [p.data.clone() for p in tr.params], [b.clone() for b in float_buffers]
    live_i = [b.clone() for b in int_buffers]
    flat = (tr.flat_param.clone(), tr.flat_ema.clone(), tr.ema_buffers.clone())
    avg = tr.ema_state_dict(model)["model"]
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    buffer_names = [n for n, b in model.named_buffers() if b.is_floating_point()]
    ptrs = [p.data_ptr() for p in tr.params]
    with tr.averaged_weights() as inside:
        assert inside is tr
        assert [p.data_ptr() for p in tr.params] == ptrs              # the views stay bound
        tr._check_bindings()
        for n, p, was in zip(names, tr.params, live_p):
            assert torch.equal(p.data, avg[n]) and not torch.equal(p.data, was), n
        for n, b, was in zip(buffer_names, float_buffers, live_b):
            assert torch.equal(b, avg[n]) and not torch.equal(b, was), n
        assert all(torch.equal(b, was) for b, was in zip(int_buffers, live_i))
        assert torch.equal(tr.flat_ema, flat[0]) and torch.equal(tr.flat_param, flat[1])
        for name, call in (("step", tr.step), ("zero_grad", tr.zero_grad), ("checkpoint", lambda: tr.checkpoint(model)),
                           ("averaged_weights", lambda: tr.averaged_weights().__enter__())):
            with pytest.raises(RuntimeError, match=rf"FlatTrainer\.{name}: not inside averaged_weights"):
                call()
    assert [p.data_ptr() for p in tr.params] == ptrs
    for got, want in zip((tr.flat_param, tr.flat_ema, tr.ema_buffers), flat):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    for got, want in zip([p.data for p in tr.params] + float_buffers, live_p + live_b):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # an exception inside the block restores too
    with pytest.raises(KeyError):
        with tr.averaged_weights():
            raise KeyError("x")
    assert torch.equal(tr.flat_param, flat[0]) and torch.equal(tr.flat_ema, flat[1])
    tr.zero_grad()      # ... and the trainer works again


def test_ema_state_dict_round_trip_and_deployment():
    model = _block()
    tr = _trainer(model, ema_decay=0.99, ema_warmup=7)
    _perturb_average(tr)
    tr.ema_updates = 5
    model.get_buffer([n for n, b in model.named_buffers() if not b.is_floating_point()][0]).fill_(9)
    sd = tr.ema_state_dict(model)
    assert set(sd) == {"decay", "warmup", "updates", "model"}
    assert (sd["decay"], sd["warmup"], sd["updates"]) == (0.99, 7, 5)
    assert list(sd["model"]) == list(model.state_dict())
    for name, v in model.state_dict().items():
        assert sd["model"][name].shape == v.shape and sd["model"][name].dtype == v.dtype, name
        if not v.is_floating_point():
            assert torch.equal(sd["model"][name], v) and int(v) == 9       # live integer buffers
        else:
            assert not torch.equal(sd["model"][name], v), name            # averaged, and a copy
    fresh = _block(seed=5)
    fresh.load_state_dict(sd["model"], strict=True)                       # the deployment path
    for name, v in fresh.state_dict().items():
        assert torch.equal(v, sd["model"][name]), name
    other_model = _block(seed=6)
    other = _trainer(other_model, ema_decay=0.5, ema_warmup=0)
    other.load_ema_state_dict(sd, other_model)
    assert (other.ema_decay, other.ema_warmup, other.ema_updates) == (0.99, 7, 5)
    assert torch.equal(other.flat_ema.view(torch.int32), tr.flat_ema.view(torch.int32))
    assert torch.equal(other.ema_buffers.view(torch.int32), tr.ema_buffers.view(torch.int32))
    assert not torch.equal(other.flat_param, tr.flat_param)               # the live weights are not the average's business
    bad = dict(sd, model={k: v for k, v in sd["model"].items() if k != list(sd["model"])[0]})
    with pytest.raises(RuntimeError, match="no entry"):
        other.load_ema_state_dict(bad, other_model)


def test_a_frozen_parameter_travels_live():
    model = _block()
    frozen = [p for p in model.parameters()][-1]
    frozen.requires_grad_(False)
    tr = _trainer(model, ema_decay=0.9)
    _perturb_average(tr)
    sd = tr.ema_state_dict(model)["model"]
    name = [n for n, p in model.named_parameters() if p is frozen][0]
    assert torch.equal(sd[name], frozen.data)
    _block(seed=4).load_state_dict(sd, strict=True)


def test_checkpoint_keys_reset_and_broadcast():
    from snn_for_object_detection_amd.trainer import broadcast_parameters
    model = _block()
    ckpt = _trainer(model).checkpoint(model)
    assert set(ckpt) == {"model", "optimizer"}                            # a default trainer: the keys it always had
    assert set(ckpt["optimizer"]) == {"state", "param_groups"}
    tr = _trainer(model, ema_decay=0.99)
    ckpt = tr.checkpoint(model)
    assert set(ckpt) == {"model", "optimizer", "ema"} and set(ckpt["optimizer"]) == {"state", "param_groups"}
    assert list(ckpt["ema"]["model"]) == list(ckpt["model"])
    for bring_back in (tr.reset_ema, lambda: broadcast_parameters(tr)):    # (one rank: nothing to broadcast, the reset stays)
        _perturb_average(tr)
        tr.ema_updates = 3
        assert not torch.equal(tr.flat_ema, tr.flat_param)
        bring_back()
        assert torch.equal(tr.flat_ema, tr.flat_param) and tr.ema_updates == 0
        live = torch.cat([b.reshape(-1).float() for b in model.buffers() if b.is_floating_point()])
        assert torch.equal(tr.ema_buffers, live)
    broadcast_parameters(_trainer(_block()))                              # without an average: as before
