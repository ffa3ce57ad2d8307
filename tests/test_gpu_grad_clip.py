"""The optimiser tail of ``FlatTrainer.step()``: the ordered fp64 gradient norm and its control record
(``snn_grad_norm``), the control-word Adamax (``snn_adamax_step_ctl``: clip factor, value clamp, weight decay, nothing
stored for a non-finite gradient), and what the trainer builds from them - Lightning's ``gradient_clip_val`` /
``gradient_clip_algorithm``, ``skip_nonfinite`` and ``weight_decay`` - against ``torch.nn.utils.clip_grad_*`` followed by
``torch.optim.Adamax`` on fp64 CPU copies fed the trainer's own gradients."""
import numpy as np
import pytest
import torch

from tests.util import synthetic_events, synthetic_labels

pytestmark = pytest.mark.gpu

RUN = 8192             # elements one block of the norm kernel owns (include/snn_hip.h)
N_BIG = 2 ** 20 + 3    # 129 blocks, ragged last group
T, B, H, W = 3, 2, 32, 48
LR = 1e-3


@pytest.fixture(scope="module")
def S(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import snn_for_object_detection_amd as pkg
    return pkg


# ------------------------------------------------------------------------------------------ the kernels, through the C ABI
def _gradient_like(n, seed):
    """Signed values whose magnitudes span 1e-9 .. 1e-1 (the gradient range of DESIGN section 3), log-uniform."""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-9.0, -1.0, n)).astype(np.float32)


def _grad_norm(lib, grad, n, grad_scale, max_norm, ctl, ws):
    rc = lib.snn_grad_norm(grad.data_ptr() if isinstance(grad, torch.Tensor) else grad, n, grad_scale, max_norm,
                           ws.data_ptr(), ctl.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.snn_last_error()
    rec = ctl.cpu().numpy()
    return rec[:2].view(np.float32)[0], rec[:2].view(np.float32)[1], int(rec[2]), int(rec[3]), rec.tobytes()


def _workspace(lib, n):
    size = lib.snn_grad_norm_workspace_size(n)
    assert size >= 8 and size % 8 == 0
    return torch.empty(size // 8, dtype=torch.float64, device="cuda")


def _check_record(lib, g_host, grad_dev, n, grad_scale, ws):
    ref = np.float32(np.float64(np.float32(grad_scale)) * np.sqrt(np.sum(g_host.astype(np.float64) ** 2)))
    ctl = torch.zeros(4, dtype=torch.int32, device="cuda")
    for max_norm in (0.0, float(ref) / 2, 1e30):
        norm, scale, finite, skipped, raw = _grad_norm(lib, grad_dev, n, grad_scale, max_norm, ctl, ws)
        print(f"n={n} grad_scale={grad_scale} max_norm={max_norm:.4g}: norm {norm!r} ref {ref!r} "
              f"ulps {abs(float(norm) - float(ref)) / float(np.spacing(ref)):.2f} scale {scale!r}")
        assert abs(np.float64(norm) - np.float64(ref)) <= np.float64(np.spacing(ref)), (n, norm, ref)   # 1 fp32 ulp
        if max_norm > 0:    # clip_grad_norm_'s coefficient in fp32, from the kernel's own norm: bit for bit
            want = np.minimum(np.float32(1), np.float32(max_norm) / (norm + np.float32(1e-6)))
        else:
            want = np.float32(1)
        assert scale.tobytes() == np.float32(want).tobytes(), (n, max_norm, scale, want)
        if max_norm == 1e30:
            assert scale == np.float32(1)
        elif max_norm > 0 and ref > 1e-5:
            assert scale < 1    # half the norm: the clip is active
        assert finite == 1 and skipped == 0
        assert _grad_norm(lib, grad_dev, n, grad_scale, max_norm, ctl, ws)[4] == raw   # reproducible bit for bit


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1023, N_BIG])
def test_grad_norm_against_fp64(S, hip_lib, n):
    g_host = _gradient_like(n, seed=n)
    g = torch.from_numpy(g_host).cuda()
    ws = _workspace(hip_lib, n)
    _check_record(hip_lib, g_host, g, n, 0.5 if n % 2 else 1.0, ws)
    if n == N_BIG:
        _check_record(hip_lib, g_host, g, n, 1.0 / 3.0, ws)


@pytest.mark.parametrize("n", [5, 1023, N_BIG])
def test_grad_norm_on_a_pointer_that_is_only_4_byte_aligned(S, hip_lib, n):
    """include/snn_hip.h: `grad` needs 4-byte alignment only - the call works one float into an allocation."""
    g_host = _gradient_like(n + 1, seed=7 + n)
    g = torch.from_numpy(g_host).cuda()
    assert g.data_ptr() % 16 == 0
    _check_record(hip_lib, g_host[1:], g.data_ptr() + 4, n, 0.5, _workspace(hip_lib, n))


def test_grad_norm_refuses_what_it_cannot_address(S, hip_lib):
    g = torch.ones(16, device="cuda")
    ctl = torch.zeros(4, dtype=torch.int32, device="cuda")
    ws = _workspace(hip_lib, 16)
    st = torch.cuda.current_stream().cuda_stream
    assert hip_lib.snn_grad_norm(g.data_ptr() + 2, 8, 1.0, 0.0, ws.data_ptr(), ctl.data_ptr(), st) != 0
    assert b"aligned" in hip_lib.snn_last_error()
    assert hip_lib.snn_grad_norm(g.data_ptr(), 0, 1.0, 0.0, ws.data_ptr(), ctl.data_ptr(), st) != 0
    assert hip_lib.snn_grad_norm(g.data_ptr(), 16, 1.0, 0.0, None, ctl.data_ptr(), st) != 0
    assert hip_lib.snn_grad_norm_workspace_size(0) == 0


def test_grad_norm_finds_one_non_finite_element_anywhere(S, hip_lib):
    g_host = _gradient_like(N_BIG, seed=3)
    g = torch.from_numpy(g_host).cuda()
    assert g.data_ptr() % 16 == 0      # so the first block's run is elements [0, RUN)
    ws = _workspace(hip_lib, N_BIG)
    ctl = torch.zeros(4, dtype=torch.int32, device="cuda")
    calls = 0
    for pos in (0, N_BIG - 1, RUN - 1):
        for bad in (float("inf"), float("-inf"), float("nan")):
            keep = float(g[pos])
            g[pos] = bad
            norm, scale, finite, skipped, _ = _grad_norm(hip_lib, g, N_BIG, 1.0, 1.0, ctl, ws)
            calls += 1
            assert finite == 0 and skipped == calls, (pos, bad, finite, skipped)
            assert not np.isfinite(norm)
            g[pos] = keep
            assert _grad_norm(hip_lib, g, N_BIG, 1.0, 1.0, ctl, ws)[2:4] == (1, calls)   # finite again: no count


def test_adamax_ctl_without_anything_to_add_is_the_plain_step_and_a_non_finite_record_stores_nothing(S, hip_lib):
    n = 4099
    gen = torch.Generator().manual_seed(5)
    p0, g, m0 = (torch.randn(n, generator=gen).cuda() for _ in range(3))
    u0 = torch.rand(n, generator=gen).cuda()
    st = torch.cuda.current_stream().cuda_stream
    hyper = (n, 2e-3, 0.9, 0.999, 1e-8, 3, 0.5)

    def run(fn, *tail):
        p, m, u = p0.clone(), m0.clone(), u0.clone()
        rc = fn(p.data_ptr(), g.data_ptr(), m.data_ptr(), u.data_ptr(), *hyper, *tail, st)
        assert rc == 0, hip_lib.snn_last_error()
        return p, m, u

    plain = run(hip_lib.snn_adamax_step)
    for tail in ((0.0, 0.0, None), (0.0, -1.0, None)):
        assert all(torch.equal(a, b) for a, b in zip(plain, run(hip_lib.snn_adamax_step_ctl, *tail)))
    # a record with scale 1 and finite 1 changes no bit either; with finite 0 the launch stores nothing
    def record(norm, scale, finite):
        rec = torch.tensor([0, 0, finite, 0], dtype=torch.int32)
        rec[:2].view(torch.float32).copy_(torch.tensor([norm, scale]))
        return rec.cuda()

    ctl = record(3.0, 1.0, 1)
    assert all(torch.equal(a, b) for a, b in zip(plain, run(hip_lib.snn_adamax_step_ctl, 0.0, 0.0, ctl.data_ptr())))
    ctl = record(3.0, 0.5, 0)
    skipped = run(hip_lib.snn_adamax_step_ctl, 1e-2, 0.1, ctl.data_ptr())
    assert all(torch.equal(a, b) for a, b in zip((p0, m0, u0), skipped))
    # order of operations: scale by the record, clamp, then add the decay
    ctl = record(3.0, 0.25, 1)
    p, m, u = run(hip_lib.snn_adamax_step_ctl, 1e-2, 0.05, ctl.data_ptr())
    ge = (g.double() * 0.5 * 0.25).clamp(-0.05, 0.05) + 1e-2 * p0.double()
    m_ref = m0.double() + 0.1 * (ge - m0.double())
    u_ref = torch.maximum(u0.double() * 0.999, ge.abs() + 1e-8)
    p_ref = p0.double() - 2e-3 / (1 - 0.9 ** 3) * m_ref / u_ref
    for got, want in ((m, m_ref), (u, u_ref), (p, p_ref)):
        assert float((got.double() - want).norm() / want.norm()) < 1e-6
    assert hip_lib.snn_adamax_step_ctl(p.data_ptr(), g.data_ptr(), m.data_ptr(), u.data_ptr(), *hyper, -1e-2, 0.0, None,
                                       st) != 0


# ------------------------------------------------------------------------------------------ the trainer
def _batch():
    return synthetic_events(T, B, H, W, p=0.1).cuda(), synthetic_labels(B).cuda()


def _fresh(S, seed=2):
    torch.manual_seed(seed)
    return S.TinyYolo(num_classes=2, time_window=0).cuda().train()


def _backward(model, tr, batch):
    tr.zero_grad()
    model.training_step(batch).backward()
    tr.synchronize()


class _TorchTail:
    """clip_grad_* then torch.optim.Adamax on ONE fp64 CPU tensor holding every parameter in the trainer's flat order
    (Adamax is elementwise and every parameter of these runs takes every step, so one tensor with one ``step`` is the
    per-parameter optimiser; the 2-norm over one tensor is clip_grad_norm_'s norm over all of them)."""

    def __init__(self, tr, weight_decay=0.0):
        self.p = torch.nn.Parameter(tr.flat_param[: tr.numel].detach().double().cpu())
        self.opt = torch.optim.Adamax([self.p], lr=LR, weight_decay=weight_decay)

    def step(self, tr, clip=None, algorithm="norm"):
        self.p.grad = tr.flat_grad[: tr.numel].detach().double().cpu()
        total = None
        if clip is not None and algorithm == "norm":
            total = float(torch.nn.utils.clip_grad_norm_([self.p], clip))
        elif clip is not None:
            torch.nn.utils.clip_grad_value_([self.p], clip)
        self.opt.step()
        return total

    def deviation(self, tr):
        """Largest relative deviation ||p - ref|| / ||ref|| over the trainer's parameters."""
        got, ref = tr.flat_param.detach().double().cpu(), self.p.detach()
        return max(float((got[lo:hi] - ref[lo:hi]).norm() / ref[lo:hi].norm().clamp_min(1e-30))
                   for lo, hi in zip(tr._offsets[:-1], tr._offsets[1:]))


@pytest.fixture(scope="module")
def unclipped(S):
    """This file's reference against the DEFAULT trainer, three steps: the largest relative parameter deviation is the
    yardstick of the clipped runs (they may show twice that: the only new rounding is one fp32 multiply by ``scale``).
    Measured on an MI355X: 5.2e-8, so 1.04e-7 allowed; the clipped runs showed
    5.0e-8 (norm), 8.7e-8 (value), 5.0e-8 (weight decay), 4.6e-8 (the step after a skipped one).  Also the first step's gradient norm and median |g|, from which the
    clipped runs take values that make the clip active."""
    from snn_for_object_detection_amd.trainer import FlatTrainer
    model, batch = _fresh(S), _batch()
    tr = FlatTrainer(model, lr=LR)
    ref = _TorchTail(tr)
    worst, first = 0.0, None
    for it in range(3):
        _backward(model, tr, batch)
        if it == 0:
            g = tr.flat_grad[: tr.numel].detach().double().cpu()
            first = {"norm": float(g.norm()), "median": float(g[g != 0].abs().median())}
        ref.step(tr)
        tr.step()
        worst = max(worst, ref.deviation(tr))
    print(f"unclipped trainer against fp64 torch.optim.Adamax: largest relative parameter deviation {worst:.3e}; "
          f"first gradient norm {first['norm']:.6e}, median |g| {first['median']:.3e}")
    assert 0 < worst < 1e-5      # (the bound of tests/test_gpu_trainer.py for the same comparison)
    return {"tolerance": 2 * worst, **first}


def test_neutral_clip_is_bit_neutral(S):
    from snn_for_object_detection_amd.trainer import FlatTrainer
    batch, out = _batch(), []
    for kw in ({}, {"gradient_clip_val": 1e30}):
        model = _fresh(S)
        tr = FlatTrainer(model, lr=LR, **kw)
        _backward(model, tr, batch)
        tr.step()
        out.append((tr.flat_param.clone(), tr.exp_avg.clone(), tr.exp_inf.clone()))
    assert float(out[0][2].abs().max()) > 0
    for a, b in zip(*out):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", ["norm", "value", "weight_decay"])
def test_clipped_steps_match_torch(S, unclipped, case):
    from snn_for_object_detection_amd.trainer import FlatTrainer
    clip, algorithm, wd = {"norm": (unclipped["norm"] / 2, "norm", 0.0), "value": (unclipped["median"], "value", 0.0),
                           "weight_decay": (None, "norm", 1e-2)}[case]
    model, batch = _fresh(S), _batch()
    tr = FlatTrainer(model, lr=LR, gradient_clip_val=clip, gradient_clip_algorithm=algorithm, weight_decay=wd)
    ref = _TorchTail(tr, weight_decay=wd)
    for it in range(3):
        _backward(model, tr, batch)
        if case == "value":
            g = tr.flat_grad[: tr.numel]
            clamped, kept = int((g.abs() > clip).sum()), int((g.abs() <= clip).sum())
            assert clamped > 0 and kept > 0, (clamped, kept)
        total = ref.step(tr, clip, algorithm)
        tr.step()
        dev = ref.deviation(tr)
        print(f"{case} step {it}: largest relative parameter deviation {dev:.3e} (allowed {unclipped['tolerance']:.3e})")
        assert dev <= unclipped["tolerance"], (case, it, dev, unclipped["tolerance"])
        if case == "norm":
            assert total > clip                                       # the clip is active
            assert abs(float(tr.last_grad_norm) - total) <= 1e-6 * total, (float(tr.last_grad_norm), total)
    if case != "norm":
        with pytest.raises(RuntimeError, match="last_grad_norm"):
            tr.last_grad_norm
    assert tr.skipped_steps == 0


def test_non_finite_step_is_skipped_and_its_step_count_rolled_back(S, unclipped):
    from snn_for_object_detection_amd.trainer import FlatTrainer
    model, batch = _fresh(S), _batch()
    tr = FlatTrainer(model, lr=LR, skip_nonfinite=True)
    ref = _TorchTail(tr)            # sees steps 1 and 3 only
    _backward(model, tr, batch)
    ref.step(tr)
    tr.step()
    after_1 = (tr.flat_param.clone(), tr.exp_avg.clone(), tr.exp_inf.clone())
    _backward(model, tr, batch)
    tr.flat_grad[5] = float("inf")
    tr.step()
    assert not torch.isfinite(tr.last_grad_norm)
    for a, b in zip(after_1, (tr.flat_param, tr.exp_avg, tr.exp_inf)):
        assert torch.equal(a, b)
    _backward(model, tr, batch)
    ref.step(tr)
    tr.step()                       # bias correction with step = 2: the skipped step's count was given back
    dev = ref.deviation(tr)
    print(f"step after a skipped one: largest relative parameter deviation {dev:.3e} (allowed {unclipped['tolerance']:.3e})")
    assert dev <= unclipped["tolerance"], (dev, unclipped["tolerance"])
    assert tr.skipped_steps == 1 and tr.step_count == 3
    sd = tr.state_dict()
    assert len(sd["state"]) == len(tr.params)
    assert all(float(sd["state"][k]["step"]) == 2 for k in sd["state"])
    assert float(ref.opt.state_dict()["state"][0]["step"]) == 2
    # what this guards against: without it one inf stays in exp_inf for good
    model = _fresh(S)
    tr = FlatTrainer(model, lr=LR)
    _backward(model, tr, batch)
    tr.flat_grad[5] = float("inf")
    tr.step()
    assert not torch.isfinite(tr.exp_inf).all()


def test_skipped_first_step_leaves_no_optimizer_state(S):
    """torch creates a parameter's state at its first step: a skipped first step must leave none."""
    from snn_for_object_detection_amd.trainer import FlatTrainer
    model, batch = _fresh(S), _batch()
    tr = FlatTrainer(model, lr=LR, skip_nonfinite=True, gradient_clip_val=1.0)
    _backward(model, tr, batch)
    tr.flat_grad[tr.numel - 1] = float("nan")
    tr.step()
    assert tr.state_dict()["state"] == {} and tr.skipped_steps == 1 and tr.param_steps == [0] * len(tr.params)
    assert float(tr.exp_inf.abs().max()) == 0.0


def test_weight_decay_checkpoint_round_trip(S):
    from snn_for_object_detection_amd.trainer import FlatTrainer
    batch = _batch()

    def one_step(model, trainer):
        _backward(model, trainer, batch)
        trainer.step()

    a = _fresh(S)
    tr_a = FlatTrainer(a, lr=2e-3, weight_decay=1e-2)
    for _ in range(2):
        one_step(a, tr_a)
    ckpt_model = {k: v.clone() for k, v in a.state_dict().items()}
    sd = tr_a.state_dict()
    assert sd["param_groups"][0]["weight_decay"] == 1e-2
    # through torch.optim.Adamax and back
    c = _fresh(S)
    opt = torch.optim.Adamax([p for p in c.parameters() if p.requires_grad], lr=1e-3)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["weight_decay"] == 1e-2
    b = _fresh(S)
    b.load_state_dict(ckpt_model)
    tr_b = FlatTrainer(b, lr=1e-3)
    tr_b.load_state_dict(opt.state_dict())
    assert tr_b.weight_decay == 1e-2 and tr_b.lr == 2e-3 and tr_b.step_count == 2
    one_step(a, tr_a)
    one_step(b, tr_b)
    for x, y in ((tr_a.flat_param, tr_b.flat_param), (tr_a.exp_avg, tr_b.exp_avg), (tr_a.exp_inf, tr_b.exp_inf)):
        assert torch.equal(x, y)
    # the decay acts: the same step without it ends elsewhere
    d = _fresh(S)
    d.load_state_dict(ckpt_model)
    tr_d = FlatTrainer(d, lr=1e-3)
    tr_d.load_state_dict(sd)
    tr_d.weight_decay = 0.0
    one_step(d, tr_d)
    assert not torch.equal(tr_d.flat_param, tr_b.flat_param)


def test_argument_checks(S):
    from snn_for_object_detection_amd.trainer import FlatTrainer
    model = _fresh(S)
    for kw in ({"gradient_clip_val": 0.0}, {"gradient_clip_val": -1.0}, {"gradient_clip_algorithm": "l1"},
               {"gradient_clip_val": 1.0, "gradient_clip_algorithm": "Norm"}, {"weight_decay": -1e-3}):
        with pytest.raises(ValueError):
            FlatTrainer(model, **kw)
    tr = FlatTrainer(model)
    sd = tr.state_dict()
    sd["param_groups"][0]["maximize"] = True
    with pytest.raises(RuntimeError, match="maximize"):
        tr.load_state_dict(sd)
    sd["param_groups"][0].update(maximize=False, weight_decay=-1.0)
    with pytest.raises(ValueError):
        tr.load_state_dict(sd)
