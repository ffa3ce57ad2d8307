"""Host side of gradient clipping / the non-finite step skip / weight decay: what needs no GPU - the workspace helper of
``snn_grad_norm``, ``FlatTrainer``'s argument checks and the optimiser state dict (tests/test_gpu_grad_clip.py has the rest)."""
import pytest
import torch


def _model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))


def test_grad_norm_workspace_size_needs_no_gpu(hip_lib):
    size = hip_lib.snn_grad_norm_workspace_size
    assert size(0) == 0 and size(-5) == 0
    assert size(1) == 8                                   # one fp64 partial per 8192-element run
    assert size(8192 - 3) == 8 and size(8192 - 2) == 16   # a base 12 bytes past a 16-byte boundary shifts the runs by 3
    assert size(4_228_544) == 8 * 517                     # TinyYolo's flat gradient
    assert size(2 ** 40) == 8 * (2 ** 27 + 1)


def test_trainer_argument_checks():
    from snn_for_object_detection_amd.trainer import FlatTrainer
    for kw in ({"gradient_clip_val": 0}, {"gradient_clip_val": -0.5}, {"gradient_clip_val": float("nan")},
               {"gradient_clip_algorithm": "inf"}, {"weight_decay": -1e-4}):
        with pytest.raises(ValueError):
            FlatTrainer(_model(), **kw)
    tr = FlatTrainer(_model(), gradient_clip_val=0.5, gradient_clip_algorithm="value", skip_nonfinite=True, weight_decay=0.01)
    assert (tr.gradient_clip_val, tr.gradient_clip_algorithm, tr.skip_nonfinite, tr.weight_decay) == (0.5, "value", True, 0.01)
    assert tr.skipped_steps == 0
    with pytest.raises(RuntimeError, match="last_grad_norm"):   # the record lives in device memory
        tr.last_grad_norm


def test_state_dict_carries_weight_decay_and_still_refuses_maximize():
    from snn_for_object_detection_amd.trainer import FlatTrainer
    tr = FlatTrainer(_model(), weight_decay=1e-2)
    sd = tr.state_dict()
    assert sd["param_groups"][0]["weight_decay"] == 1e-2
    opt = torch.optim.Adamax(_model().parameters(), lr=1e-3)
    opt.load_state_dict(sd)                                # torch takes the group as it is
    assert opt.param_groups[0]["weight_decay"] == 1e-2
    other = FlatTrainer(_model())
    assert other.state_dict()["param_groups"][0]["weight_decay"] == 0
    other.load_state_dict(opt.state_dict())
    assert other.weight_decay == 1e-2
    sd["param_groups"][0]["maximize"] = True
    with pytest.raises(RuntimeError, match="maximize"):
        other.load_state_dict(sd)
    sd["param_groups"][0].update(maximize=False, weight_decay=-1.0)
    with pytest.raises(ValueError):
        other.load_state_dict(sd)
