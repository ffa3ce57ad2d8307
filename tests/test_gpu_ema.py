"""The weight average (EMA) on the device: ``snn_adamax_step_ema`` / ``snn_ema_update`` through the C ABI against an fp64
restatement and bit for bit against ``snn_adamax_step_ctl``, and what ``FlatTrainer(ema_decay=...)`` builds from them - an
average that changes no bit of training, follows an fp64 average, skips with a skipped step, moves a parameter without a
gradient, and that ``averaged_weights()`` really puts in front of the kernels (tests/test_ema_host.py has the host side)."""
import numpy as np
import pytest
import torch

from tests.util import synthetic_events, synthetic_labels

pytestmark = pytest.mark.gpu

T, B, H, W = 3, 2, 32, 48      # the batch of tests/test_gpu_grad_clip.py
# Adamax moves every element that has a gradient by about lr per step; 1e-2 keeps the distance between the average and the
# weights (a few lr) an order of magnitude above the "is not the live weights" threshold also for the BatchNorm scales (= 1)
LR = 1e-2
U = 2.0 ** -23                 # fp32 unit in the last place of 1


@pytest.fixture(scope="module")
def S(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import snn_for_object_detection_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def batch(S):
    return synthetic_events(T, B, H, W, p=0.1).cuda(), synthetic_labels(B).cuda()


class _Calls:
    """``_hip.PROFILER`` that only writes down (name, args) of every C-ABI call."""

    def __init__(self):
        self.calls = []

    def before(self, name, args):
        self.calls.append((name, args))

    def after(self, token):
        pass

    def names(self):
        return [n for n, _ in self.calls]


def _recorded_step(tr):
    from snn_for_object_detection_amd import _hip
    rec = _Calls()
    assert _hip.PROFILER is None
    _hip.PROFILER = rec
    try:
        tr.step()
    finally:
        _hip.PROFILER = None
    return rec


# ------------------------------------------------------------------------------------------ the kernels, through the C ABI
def _record(scale, finite):
    rec = torch.tensor([0, 0, finite, 0], dtype=torch.int32)
    rec[:2].view(torch.float32).copy_(torch.tensor([3.0, scale]))
    return rec.cuda()


def _ema_bound(ref, w, src, ema0):
    """One fp32 ulp of the reference plus 2^-23 w |src - ema0| per element: the rounding of the difference, of the product
    and of the sum, fused or not."""
    return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + U * float(w) * np.abs(src - ema0)


def _check_average(got, ema0, src, w, what):
    """``got`` (fp32, from the kernel) against ``ema0 + w (src - ema0)`` in fp64 from the fp32 ``src`` and the fp32 ``w``."""
    ema0, src = ema0.double().cpu().numpy(), src.double().cpu().numpy()
    w = np.float64(np.float32(w))
    ref = ema0 + w * (src - ema0)
    err, bound = np.abs(got.double().cpu().numpy() - ref), _ema_bound(ref, w, src, ema0)
    worst = float(np.max(err / bound))
    print(f"{what}: largest error / bound {worst:.3f}")
    assert np.all(err <= bound), (what, worst)


def _offset(t, off):
    """``t`` copied into a fresh allocation ``off`` floats in: -> (keep-alive tensor, view, pointer)."""
    whole = torch.zeros(t.numel() + off, device="cuda")
    whole[off:].copy_(t)
    assert whole.data_ptr() % 16 == 0
    return whole, whole[off:], whole.data_ptr() + 4 * off


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 4099])
def test_kernels_against_fp64_and_bit_for_bit_against_the_ctl_step(S, hip_lib, n):
    gen = torch.Generator().manual_seed(100 + n)
    p0, g, m0, ema0 = (torch.randn(n, generator=gen) for _ in range(4))    # the average is drawn independently of p
    u0 = torch.rand(n, generator=gen) + 1e-3
    src0 = torch.randn(n, generator=gen)
    st = torch.cuda.current_stream().cuda_stream
    hyper = (n, 2e-3, 0.9, 0.999, 1e-8, 3, 0.5)
    wd, clip = 1e-2, 0.05
    live, dead = _record(0.25, 1), _record(0.25, 0)
    for off in (0, 1):                       # aligned, and one float into the allocations
        for d in (0.0, 0.9, 0.9999):
            w = float(np.float32(1.0 - d))
            # (wd, clip, ctl): everything set; nothing set - where snn_adamax_step_ctl launches the plain kernel
            for tail in ((wd, clip, live), (0.0, 0.0, None)):
                ctl = None if tail[2] is None else tail[2].data_ptr()
                a = [_offset(t, off) for t in (p0, g, m0, u0)]
                rc = hip_lib.snn_adamax_step_ctl(*(x[2] for x in a), *hyper, tail[0], tail[1], ctl, st)
                assert rc == 0, hip_lib.snn_last_error()
                b = [_offset(t, off) for t in (p0, g, m0, u0, ema0)]
                rc = hip_lib.snn_adamax_step_ema(*(x[2] for x in b), *hyper, tail[0], tail[1], w, ctl, st)
                assert rc == 0, hip_lib.snn_last_error()
                for k in (0, 2, 3):          # p, m, u: the same bits
                    assert torch.equal(a[k][0].view(torch.int32), b[k][0].view(torch.int32)), (n, off, d, k)
                assert not torch.equal(b[0][1].cpu(), p0) and torch.equal(b[1][1].cpu(), g)
                _check_average(b[4][1], ema0, b[0][1], w, f"step n={n} off={off} d={d} ctl={ctl is not None}")
            # a record that says "not finite": nothing is stored, the average included
            b = [_offset(t, off) for t in (p0, g, m0, u0, ema0)]
            rc = hip_lib.snn_adamax_step_ema(*(x[2] for x in b), *hyper, wd, clip, w, dead.data_ptr(), st)
            assert rc == 0, hip_lib.snn_last_error()
            for x, t in zip(b, (p0, g, m0, u0, ema0)):
                assert torch.equal(x[1].cpu().view(torch.int32), t.view(torch.int32)), (n, off, d)
            # the same update from an arbitrary source
            for ctl in (None, live.data_ptr()):
                e, s = _offset(ema0, off), _offset(src0, off)
                assert hip_lib.snn_ema_update(e[2], s[2], n, w, ctl, st) == 0, hip_lib.snn_last_error()
                _check_average(e[1], ema0, src0, w, f"update n={n} off={off} d={d}")
                assert torch.equal(s[1].cpu(), src0) and float(e[0][:off].abs().sum()) == 0
            e, s = _offset(ema0, off), _offset(src0, off)
            assert hip_lib.snn_ema_update(e[2], s[2], n, w, dead.data_ptr(), st) == 0, hip_lib.snn_last_error()
            assert torch.equal(e[1].cpu().view(torch.int32), ema0.view(torch.int32))


def test_refusals_on_device_pointers(S, hip_lib):
    x = torch.ones(8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    a = x.data_ptr()
    assert hip_lib.snn_ema_update(a, a + 16, 4, 0.0, None, st) != 0 and b"ema_weight" in hip_lib.snn_last_error()
    assert hip_lib.snn_ema_update(a, a + 16, 4, 0.5, a + 2, st) != 0 and b"aligned" in hip_lib.snn_last_error()
    assert hip_lib.snn_adamax_step_ema(a, a, a, a, None, 4, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 0.0, 0.0, 0.5, None, st) != 0
    assert b"ema" in hip_lib.snn_last_error()
    assert torch.equal(x.cpu(), torch.ones(8))


# ------------------------------------------------------------------------------------------ the trainer
def _fresh(S, seed=2):
    torch.manual_seed(seed)
    return S.TinyYolo(num_classes=2, time_window=0).cuda().train()


def _backward(model, tr, batch):
    tr.zero_grad()
    model.training_step(batch).backward()
    tr.synchronize()


def _float_buffers(model):
    return [b for b in model.buffers() if b.is_floating_point()]


def _live_buffers(model):
    return torch.cat([b.detach().reshape(-1).float() for b in _float_buffers(model)])


class _Fp64Average:
    """An fp64 CPU average of the trainer's flat parameters and float buffers, updated from the trainer's own fp32 values
    with the fp32 weight the kernel was given."""

    def __init__(self, tr, model):
        self.p = tr.flat_param.detach().double().cpu()
        self.b = _live_buffers(model).double().cpu()

    def update(self, tr, model, k):
        w = float(np.float32(1.0 - tr.ema_decay_at(k)))
        self.p += w * (tr.flat_param.detach().double().cpu() - self.p)
        self.b += w * (_live_buffers(model).double().cpu() - self.b)

    def deviation(self, tr):
        """Largest ||ema - ref|| / ||ref|| over the trainer's parameters, and the same over the buffer vector."""
        got = tr.flat_ema.detach().double().cpu()
        per_param = max(float((got[lo:hi] - self.p[lo:hi]).norm() / self.p[lo:hi].norm().clamp_min(1e-30))
                        for lo, hi in zip(tr._offsets[:-1], tr._offsets[1:]))
        buffers = float((tr.ema_buffers.detach().double().cpu() - self.b).norm() / self.b.norm())
        return per_param, buffers


def test_averaging_changes_no_bit_of_training_and_a_default_step_no_call(S, batch):
    from snn_for_object_detection_amd.trainer import FlatTrainer
    plain_model, ema_model = _fresh(S), _fresh(S)
    plain = FlatTrainer(plain_model, lr=LR)
    ema = FlatTrainer(ema_model, lr=LR, ema_decay=0.5, ema_warmup=0)
    assert plain.flat_ema is None and plain.ema_buffers is None
    assert torch.equal(plain.flat_param, ema.flat_param)
    for it in range(3):
        _backward(plain_model, plain, batch)
        _backward(ema_model, ema, batch)
        ema.flat_grad.copy_(plain.flat_grad)        # the same gradient: backward non-determinism does not enter
        a, b = _recorded_step(plain).names(), _recorded_step(ema).names()
        assert "snn_adamax_step_ema" not in a and "snn_ema_update" not in a
        assert a.count("snn_adamax_step") == 1 and "snn_adamax_step_ctl" not in a
        assert b.count("snn_adamax_step_ema") == 1 and b.count("snn_ema_update") == 1     # (the buffers)
        assert "snn_adamax_step" not in b and "snn_adamax_step_ctl" not in b
        # apart from the average the two steps are the same sequence of calls
        assert [n for n in b if n != "snn_ema_update"] == ["snn_adamax_step_ema" if n == "snn_adamax_step" else n for n in a]
        for x, y in ((plain.flat_param, ema.flat_param), (plain.exp_avg, ema.exp_avg), (plain.exp_inf, ema.exp_inf)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), it
    assert ema.ema_updates == 3 and plain.ema_updates == 0
    assert not torch.equal(ema.flat_ema, ema.flat_param)


K_STEPS = 4
FP64_BOUND = K_STEPS * 2.0 ** -22
# Adamax moves an element by lr * m / (max |g| + eps) per step: "about lr" only where |g| is well above eps.  On this small
# three-timestep clip the gradients of one backbone residual block are 1e-11 .. 1e-9 (measured), under torch's default
# eps = 1e-8, and those weights then move by lr / 250 per step.  The run below is about the average, not about Adamax's
# floor, so it puts eps under every gradient fp32 can hold here (and 18 decades above the smallest normal number).
EPS_BELOW_EVERY_GRADIENT = 1e-20


@pytest.fixture(scope="module", params=[0, 2], ids=["warmup0", "warmup2"])
def averaged_run(S, batch, request):
    """K = 4 training steps with ``ema_decay=0.5`` next to an fp64 average; shared by the two tests below."""
    from snn_for_object_detection_amd.trainer import FlatTrainer
    warmup = request.param
    model = _fresh(S)
    tr = FlatTrainer(model, lr=LR, eps=EPS_BELOW_EVERY_GRADIENT, ema_decay=0.5, ema_warmup=warmup)
    ref = _Fp64Average(tr, model)
    nonzero = [False] * len(tr.params)
    for k in range(1, K_STEPS + 1):
        _backward(model, tr, batch)
        assert all(slot.written for slot in tr.slots)                # every parameter receives a gradient ...
        for i, (lo, hi) in enumerate(zip(tr._offsets[:-1], tr._offsets[1:])):
            nonzero[i] = nonzero[i] or bool((tr.flat_grad[lo:hi] != 0).any())   # ... but not every gradient is non-zero
        tr.step()
        ref.update(tr, model, k)
        assert tr.ema_updates == k
    return warmup, tr, ref, nonzero


def test_average_against_fp64(averaged_run):
    """Per parameter ||ema - ref|| / ||ref|| <= K 2^-22: each update adds at most 2^-23 (||ema|| + w ||p - ema||), earlier
    errors shrink by d, and ||p - ema|| <= ||ema|| in these runs.  Measured on an MI355X: 4.3e-8 (warmup 0) and 3.3e-8
    (warmup 2) for the parameters, 5.1e-8 and 2.1e-8 for the buffer vector, against 9.5e-7."""
    warmup, tr, ref, _ = averaged_run
    dev, dev_buffers = ref.deviation(tr)
    print(f"warmup {warmup}: largest relative deviation of the average from fp64 after {K_STEPS} steps: parameters "
          f"{dev:.3e}, buffers {dev_buffers:.3e} (allowed {FP64_BOUND:.3e})")
    assert dev <= FP64_BOUND and dev_buffers <= FP64_BOUND


def test_average_is_not_the_live_weights(averaged_run):
    """||ema - p|| / ||p|| > 1000 K 2^-22 = 9.5e-4 for every parameter that received a gradient ("Adamax moves each such
    element by about lr per step").

    "Received a gradient" is read as "a gradient with a non-zero element in one of the K steps": 46 of TinyYolo's 70
    parameters get a gradient that is exactly zero in all four steps of this clip (in three timesteps no spike reaches the
    deeper neck layers or the heads), Adamax cannot move them (m = 0), and for those the test asserts what must hold
    instead - the average equals the parameter bit for bit.
    Measured on an MI355X over the other 24: smallest 2.3e-3 (``ema_warmup=0``) and 1.9e-3 (``ema_warmup=2``), the
    BatchNorm scales that see their first gradient late.  With torch's default eps = 1e-8 instead of
    ``EPS_BELOW_EVERY_GRADIENT`` four parameters of one residual block, whose gradients are under 1e-9, showed 7.5e-5 ..
    5.7e-4: Adamax's floor, not the average."""
    warmup, tr, _, nonzero = averaged_run
    got, live = tr.flat_ema.detach().double().cpu(), tr.flat_param.detach().double().cpu()
    apart = []
    for i, (lo, hi) in enumerate(zip(tr._offsets[:-1], tr._offsets[1:])):
        if nonzero[i]:
            apart.append(float((got[lo:hi] - live[lo:hi]).norm() / live[lo:hi].norm()))
        else:   # Adamax left it where it was (m = 0): the average of a constant is that constant
            assert torch.equal(tr.flat_ema[lo:hi].view(torch.int32), tr.flat_param[lo:hi].view(torch.int32))
    apart.sort()
    print(f"warmup {warmup}: ||ema - p|| / ||p|| over the {len(apart)} parameters with a non-zero gradient: smallest "
          f"{[f'{a:.3e}' for a in apart[:5]]}, largest {apart[-1]:.3e} (each must exceed {1000 * FP64_BOUND:.3e}); "
          f"{len(nonzero) - len(apart)} parameters with an all-zero gradient")
    assert apart and apart[0] > 1000 * FP64_BOUND


def test_parameter_without_a_gradient_still_moves_the_average(S):
    from snn_for_object_detection_amd.trainer import FlatTrainer
    torch.manual_seed(4)
    used = S.BlockGen(2, [S.Conv(8, 3, 2), S.Norm(), S.LIF(), S.Conv(4, 1)])
    unused = S.BlockGen(2, [S.Conv(8, 3)])
    model = torch.nn.ModuleList([used, unused]).cuda()
    tr = FlatTrainer(model, lr=LR, ema_decay=0.9, ema_warmup=0)
    (k,) = [i for i, p in enumerate(tr.params) if any(p is q for q in unused.parameters())]
    lo, hi = tr._offsets[k], tr._offsets[k + 1]
    tr.flat_ema[lo:hi] += 0.1
    ema0, p0 = tr.flat_ema.clone(), tr.flat_param.clone()
    tr.zero_grad()
    for p in used.parameters():
        p.grad = torch.randn_like(p)
    rec = _recorded_step(tr)
    updates = [a for n, a in rec.calls if n == "snn_ema_update"]
    assert len(updates) == 2 and updates[0][2] == hi - lo         # the unwritten range, then the buffers
    assert torch.equal(tr.flat_param[lo:hi], p0[lo:hi])           # Adamax left the parameter alone ...
    _check_average(tr.flat_ema[lo:hi], ema0[lo:hi], p0[lo:hi], np.float32(1.0 - 0.9), "unused convolution")
    assert float((tr.flat_ema[lo:hi] - ema0[lo:hi]).abs().min()) > 0.005     # ... and the average moved towards it
    assert k not in tr.state_dict()["state"] and tr.param_steps[k] == 0      # its Adamax state stays absent
    assert float(tr.exp_avg[lo:hi].abs().max()) == 0 and float(tr.exp_inf[lo:hi].abs().max()) == 0
    assert not torch.equal(tr.flat_param[:lo], p0[:lo]) and len(tr.state_dict()["state"]) == len(tr.params) - 1
    _check_average(tr.flat_ema[:lo], ema0[:lo], tr.flat_param[:lo], np.float32(1.0 - 0.9), "used parameters")


def test_skipped_step_leaves_the_average_alone_and_gives_its_update_back(S, batch):
    from snn_for_object_detection_amd.trainer import FlatTrainer
    model = _fresh(S)
    tr = FlatTrainer(model, lr=LR, ema_decay=0.5, ema_warmup=2, skip_nonfinite=True)
    ref = _Fp64Average(tr, model)
    _backward(model, tr, batch)
    tr.step()
    ref.update(tr, model, 1)
    after_1 = (tr.flat_ema.clone(), tr.ema_buffers.clone(), tr.flat_param.clone())
    live_1 = _live_buffers(model)
    _backward(model, tr, batch)
    tr.flat_grad[5] = float("inf")
    tr.step()
    for was, now in zip(after_1, (tr.flat_ema, tr.ema_buffers, tr.flat_param)):
        assert torch.equal(was.view(torch.int32), now.view(torch.int32))
    assert not torch.equal(_live_buffers(model), live_1)          # the forward pass did move the live statistics
    _backward(model, tr, batch)
    tr.step()
    ref.update(tr, model, 2)                                      # d_2, not d_3: the skipped update was given back
    dev, dev_buffers = ref.deviation(tr)
    print(f"average after [step, skipped step, step] against fp64 with d_1, d_2: parameters {dev:.3e}, buffers "
          f"{dev_buffers:.3e} (allowed {2 * 2.0 ** -22:.3e})")
    assert dev <= 2 * 2.0 ** -22 and dev_buffers <= 2 * 2.0 ** -22
    assert tr.skipped_steps == 1 and tr.ema_updates == 2 and tr.step_count == 3
    assert tr.ema_state_dict(model)["updates"] == 2


def test_averaged_weights_rebuilds_what_the_kernels_read(S, batch):
    from snn_for_object_detection_amd.trainer import FlatTrainer
    model = _fresh(S)
    tr = FlatTrainer(model, lr=LR, ema_decay=0.5, ema_warmup=0)
    for _ in range(3):
        _backward(model, tr, batch)
        tr.step()
    model.eval()
    # a clip the eval-mode network answers: with the running statistics of three steps a spike needs more timesteps and
    # denser events than the training batch has to reach the heads (that batch gives all zeros whatever the weights are)
    clip = synthetic_events(16, B, H, W, p=1.0).cuda()
    assert tr.flat_wt is not None and tr.flat_w16 is not None and tr.flat_wfrag is not None
    images = [tr.flat_param, tr.flat_ema, tr.ema_buffers, tr.flat_wt, tr.flat_w16, tr.flat_wfrag, *_float_buffers(model)]
    before = [t.detach().clone() for t in images]

    def forward(m):
        with torch.no_grad():
            _, cls, bbox = m(clip)
        return torch.cat([cls.reshape(-1), bbox.reshape(-1)]).clone()

    with tr.averaged_weights():
        inside = forward(model)
        assert not torch.equal(tr.flat_wt, before[3]) and not torch.equal(tr.flat_w16.view(torch.int32),
                                                                           before[4].view(torch.int32))
    outside = forward(model)
    for t, was in zip(images, before):
        assert torch.equal(t.view(torch.int32), was.view(torch.int32))
    # model B: a fresh model deployed from the checkpointed average, reading the same kind of weight images
    other = S.TinyYolo(num_classes=2, time_window=0)
    other.load_state_dict(tr.ema_state_dict(model)["model"], strict=True)
    other = other.cuda().eval()
    other_tr = FlatTrainer(other, lr=LR)
    assert torch.equal(other_tr.flat_param, tr.flat_ema)
    first, second = forward(other), forward(other)
    spread = float((first - second).abs().max())
    print(f"eval forward run twice: largest difference {spread:.3e}; inside averaged_weights() against the deployed "
          f"average {float((inside - first).abs().max()):.3e}, against the live weights "
          f"{float((inside - outside).abs().max()):.3e}")
    print(f"non-zero outputs: averaged {int((inside != 0).sum())}, live {int((outside != 0).sum())} of {inside.numel()}")
    assert int((inside != 0).sum()) > 0 and int((outside != 0).sum()) > 0      # the network answers this clip
    assert torch.equal(first, second)         # the eval path is reproducible, so the comparison below is exact
    assert torch.equal(inside, first)
    assert not torch.equal(inside, outside)
    assert float((inside - outside).abs().max()) > 1e-4


def test_lr_schedule_sees_the_count_of_successful_steps(S):
    from snn_for_object_detection_amd.trainer import FlatTrainer, warmup_cosine
    torch.manual_seed(4)
    model = S.BlockGen(2, [S.Conv(8, 3, 2), S.Norm(), S.LIF(), S.Conv(4, 1)]).cuda()
    sched = warmup_cosine(1e-3, warmup_steps=3, total_steps=8)
    tr = FlatTrainer(model, lr=sched, skip_nonfinite=True)
    seen = []
    for it in range(5):
        tr.zero_grad()
        for p in tr.params:
            p.grad = torch.randn_like(p)
        if it == 1:
            tr.params[0].grad[(0,) * tr.params[0].dim()] = float("inf")
        rec = _recorded_step(tr)
        seen += [a[5] for n, a in rec.calls if n == "snn_adamax_step_ctl"]
        assert not any(n in ("snn_adamax_step", "snn_adamax_step_ema") for n in rec.names())
    # attempts 0..4 with attempt 1 skipped: the schedule is read at 0, 1, 1 (again: that step did not count), 2, 3
    assert seen == [sched(k) for k in (0, 1, 1, 2, 3)]
    assert seen[2] == sched(1) != sched(2)
    assert tr.skipped_steps == 1 and tr.step_count == 5
    assert tr.state_dict()["param_groups"][0]["lr"] == sched(4)
