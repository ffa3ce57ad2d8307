"""Autograd operators over the HIP C ABI (``include/snn_hip.h``).

Every operator works on a whole layer-major sequence ``[T, B, C, H, W]`` (logical NCHW per
frame, channels-last memory ``[T][B][H][W][C]``), or on one timestep ``[B, C, H, W]`` which is
the ``T = 1`` case of the same kernels (streaming ``predict``, reference-style time-outer loops).

torch is used for device memory, the autograd tape and the current stream only; all arithmetic
of the hot path happens in ``libsnn_hip.so``.  No CPU / eager fallback exists: tensors that are
not on a HIP device raise.
"""

import collections
import contextlib
import ctypes
import functools
import os
import struct
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch.autograd import Function

from . import _hip
from ._hip import NeuronParams
# The stateless families live in the modules below (each imports only the stdlib, torch, ``_hip`` and ``_layout``); this
# module keeps every lever and all mutable state, and stays the one namespace the package, the tests and the tools use.
from ._layout import (_BF16, _F32, ConcatPromise, Dest, _add_cl, _alias, _cl_view, _Convert, _copy_cl,  # noqa: F401
                      _dims5, _new_cl, _out_tensor, _ptr, _raw_convert, _raw_dense_cl, _raw_to_cl, _raw_to_nchw,
                      _require_device, _stream, _through_fp32, _ToChannelsLast, as_sequence, cl_stride, is_channels_last,
                      to_bfloat16, to_channels_last, to_float32)
from .pointwise import (POOL2D_COVERED, _Act, _Pool, _PoolPad, _SPP, _Upsample, activation, pool2d,  # noqa: F401
                        pool_covers, pool_sets, spp_covers, upsample_nearest)
from .losses import (MAX_LABEL_STEPS, _DetectionLoss, _GatherSteps, _loss_entry, _loss_ext, _require_steps,  # noqa: F401
                     check_loss_options, detection_loss, detection_loss_ext, detection_loss_steps,
                     detection_loss_steps_ext, gather_steps, select_label_steps)
from .event_ops import (AUG_Q16_MAX, AUG_Q16_MIN, AUG_Q16_ONE, _check_batch_vectors, _launch_batch_scatter,  # noqa: F401
                        check_aug_table, events_to_frames, events_to_frames_aug, events_to_frames_packed, labels_augment)

# The assignable levers of this module (each is defined, with its meaning, beside the code that reads it).
LEVERS = ("USE_WGRAD_STREAM", "USE_HEAD_STREAMS", "WGRAD_SIDE_DEPTH", "FUSE_OUTER_ADDEND", "USE_SIBLING_FUSION",
          "USE_SPIKES_FROM_VDEC", "USE_SPIKE_MASK", "SPIKE_MASK_MIN_BYTES", "USE_HALO_CONV", "USE_DEFERRED_BN_APPLY",
          "SCAN_SEGMENT_T", "USE_CONV_BN_STATS", "USE_PRESPLIT_WEIGHTS", "USE_PRESPLIT_DGRAD", "SCAN_FLAGS",
          "USE_SUMS_FROM_STATE", "LIF_CHECKPOINT_BYTES", "USE_LSTM_SCAN", "USE_FUSED_BWD1X1",
          "FUSED_BWD1X1_MIN_BYTES")


@contextlib.contextmanager
def levers(**values):
    """Set levers for the enclosed block and put back what was found, however the block ends.  A name that is not in
    ``LEVERS`` raises ``AttributeError`` before anything is changed (a misspelt lever must not pass as a no-op)."""
    unknown = sorted(set(values) - set(LEVERS))
    if unknown:
        raise AttributeError(f"functional has no lever {', '.join(unknown)} (LEVERS: {', '.join(LEVERS)})")
    found = {name: globals()[name] for name in values}
    globals().update(values)
    try:
        yield
    finally:
        globals().update(found)

# norse defaults as fp32 rounds them (dt*tau_mem_inv, -dt*tau_syn_inv, v_leak, v_th, v_reset, alpha);
# oracle/neurons.py:neuron_constants() evaluates the same torch expressions (tests pin the equality).
DEFAULT_DT = 0.001


# LIF surrogate gradients (SNN_SURR_* of include/snn_hip.h, where they are defined): name -> code
SURROGATES = {"super": _hip.SURR_SUPER, "triangle": _hip.SURR_TRIANGLE, "sigmoid": _hip.SURR_SIGMOID,
              "atan": _hip.SURR_ATAN}


def _surrogate_code(surrogate: str) -> int:
    if surrogate not in SURROGATES:
        raise ValueError(f"unknown surrogate {surrogate!r}: one of {sorted(SURROGATES)}")
    return SURROGATES[surrogate]


def _check_lif_constants(alpha: float, v_th: float, v_reset: float) -> None:
    if not alpha > 0:
        raise ValueError(f"the surrogate slope alpha must be positive, got {alpha}")
    if not v_reset < v_th:
        raise ValueError(f"v_reset ({v_reset}) must lie below v_th ({v_th})")


def _check_time_constants(dt: float, tau_mem: float, tau_syn: float) -> None:
    """c_mem = dt / tau_mem in (0, 1] (the potential does not overshoot its target), -c_syn = dt / tau_syn in (0, 1) (the
    current decays without changing sign, and 1 + c_syn has a logit for the learnable layer)."""
    if not (tau_mem > 0 and 0 < dt / tau_mem <= 1):
        raise ValueError(f"tau_mem ({tau_mem}) must give 0 < dt/tau_mem <= 1 at dt = {dt}")
    if not (tau_syn > 0 and 0 < dt / tau_syn < 1):
        raise ValueError(f"tau_syn ({tau_syn}) must give 0 < dt/tau_syn < 1 at dt = {dt}")


def neuron_params(dt: float = DEFAULT_DT, *, tau_mem: float = 1e-2, tau_syn: float = 5e-3, surrogate: str = "super",
                  alpha: float = 100.0, detach_reset: bool = False, v_th: float = 1.0, v_reset: float = 0.0,
                  v_leak: float = 0.0) -> NeuronParams:
    """The constants of one neuron layer.  The keywords are the LIF layer's own: its membrane and synaptic time constants
    (seconds; the kernels see ``c_mem = dt / tau_mem`` and ``c_syn = -dt / tau_syn``), its threshold / reset / leak
    potentials and its BACKWARD rule - the surrogate ``dz/du`` (``"super"``, ``"triangle"``, ``"sigmoid"``, ``"atan"``, all
    with value 1 at the threshold and slope parameter ``alpha``) and whether the spike inside the reset term is a constant
    of the backward pass (``detach_reset``).  The defaults are the norse defaults the reference runs with."""
    code = _surrogate_code(surrogate)
    _check_lif_constants(alpha, v_th, v_reset)
    _check_time_constants(dt, tau_mem, tau_syn)
    tau_syn_inv = torch.as_tensor(1.0 / tau_syn)
    tau_mem_inv = torch.as_tensor(1.0 / tau_mem)
    # + SLI saturation potential (sli.py:38-39) and the synapse constants (synapse.py:26-36,77)
    return NeuronParams((dt * tau_mem_inv).item(), (-dt * tau_syn_inv).item(), float(v_leak), float(v_th), float(v_reset),
                        float(alpha), 1.0, torch.as_tensor(1.0 / 1e-3).item(), torch.as_tensor(1.0 / 5e-3).item(), dt, 0.0,
                        code, int(bool(detach_reset)))


def default_gradient_rule(params: NeuronParams) -> bool:
    """SuperSpike with the reset differentiated through the spike: the rule every scan kernel has."""
    return params.surrogate == _hip.SURR_SUPER and not params.reset_detached


def set_lif_gradient(model, surrogate: Optional[str] = None, alpha: Optional[float] = None,
                     detach_reset: Optional[bool] = None) -> int:
    """Rewrite the backward rule of every ``LIFCell`` of ``model`` (``StateStorage``-wrapped ones included); ``None``
    leaves a field as it is.  Returns the number of cells changed.  The rule lives in each cell's ``params`` - no
    parameter, buffer or ``state_dict`` key is involved, and the forward pass does not change."""
    from .layer_gen import LIFCell
    code = None if surrogate is None else _surrogate_code(surrogate)
    n = 0
    for m in model.modules():
        if not isinstance(m, LIFCell):
            continue
        p = m.params
        _check_lif_constants(p.alpha if alpha is None else alpha, p.v_th, p.v_reset)
        if code is not None:
            p.surrogate = code
        if alpha is not None:
            p.alpha = float(alpha)
        if detach_reset is not None:
            p.reset_detached = int(bool(detach_reset))
        n += 1
    return n


LEARN_TAU = (None, "layer", "channel")


def set_lif_time_constants(model, tau_mem: Optional[float] = None, tau_syn: Optional[float] = None,
                           learn_tau: Optional[str] = None) -> int:
    """Set the time constants of every ``LIFCell`` of ``model`` (``StateStorage``-wrapped ones included) and, with
    ``learn_tau="layer"`` / ``"channel"``, make them parameters of the cell (``w_mem``, ``w_syn``; see ``LIFCell``); ``None``
    leaves a field as it is.  Returns the number of cells changed.  For a model built from an unchanged description: a cell
    records its channel count when its generator builds it (``LIF.get``), and ``learn_tau="channel"`` on a cell that has none
    raises.  Because it may ADD or REPLACE parameters (new constants re-initialise a learnable cell's raw parameters) it must
    run before the ``FlatTrainer`` (or any optimiser) is built; a cell whose parameters a ``FlatTrainer`` already holds
    raises."""
    from .layer_gen import LIFCell
    if learn_tau not in LEARN_TAU:
        raise ValueError(f"learn_tau must be one of {LEARN_TAU}, not {learn_tau!r}")
    cells = [m for m in model.modules() if isinstance(m, LIFCell)]
    for m in cells:   # every cell is checked before the first one changes
        m.check_time_constants(tau_mem, tau_syn, learn_tau)
    dev = next((q.device for q in model.parameters()), None)
    for m in cells:
        m.set_time_constants(tau_mem, tau_syn, learn_tau, device=dev)
    return len(cells)


def lif_time_constants(w_mem: torch.Tensor, w_syn: torch.Tensor, channels: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(c_mem[C], c_syn[C])`` of a learnable LIF layer from its raw parameters (``[1]`` or ``[C]`` each):
    ``c_mem = sigmoid(w_mem)``, ``1 + c_syn = sigmoid(w_syn)`` (snn_lif_tau_param).  No autograd: the layer's backward
    applies the chain rule itself."""
    w_mem, w_syn = w_mem.detach(), w_syn.detach()
    _require_device(w_mem, "time-constant parameters")
    n = w_mem.numel()
    if n not in (1, channels) or w_syn.numel() != n or w_syn.dtype != _F32 or not w_syn.is_cuda:
        raise RuntimeError(f"time-constant parameters: w_mem and w_syn hold 1 or {channels} fp32 values each on the device, not "
                           f"{n} and {w_syn.numel()}")
    c = torch.empty((2, channels), device=w_mem.device, dtype=_F32)
    _hip.call("snn_lif_tau_param", w_mem.contiguous().data_ptr(), w_syn.contiguous().data_ptr(), n, channels,
              c[0].data_ptr(), c[1].data_ptr(), _stream())
    return c[0], c[1]


def _tau_refusal(neuron: int, bf16_storage: bool, checkpointed: bool = False) -> None:
    """What a layer with per-channel / learnable time constants (``affine_neuron(tau=...)``) cannot be combined with: said by
    name, before any launch.  ``checkpointed`` is there for completeness only: no caller in the package passes True,
    because ``LIF_CHECKPOINT_BYTES`` never selects such a layer (it stays on the plain scan, ``_AffineNeuron.forward``); the
    branch states what a caller that forced the checkpointed pair would be told."""
    if neuron != _hip.NEURON_LIF:
        raise RuntimeError("per-channel / learnable time constants (tau=...) belong to LIF layers: LI, LI+Tanh, SLI and "
                           "Synapse scans save no potential to rebuild the current from")
    if bf16_storage:
        raise RuntimeError("bf16 storage has no scan with per-channel / learnable time constants (tau=...): keep this layer's "
                           "tensors fp32")
    if checkpointed:
        raise RuntimeError("the checkpointed LIF pair (LIF_CHECKPOINT_BYTES) has the struct's scalar time constants only: a "
                           "layer with tau=... takes the plain scan")


# ------------------------------------------------------------------------------------------- precision
# The arithmetic of a convolution is an argument of every C-ABI call (include/snn_hip.h, SNN_PREC_*): the library keeps
# no arithmetic state.  What is kept HERE is the Python-side default that layers without their own setting use:
#   forward : "fp16x3" (default: two fp16 pieces per operand after exact power-of-two pre-scaling, three products;
#             fp32-grade for conv inputs |x| < 4094 and weights |w| < 255 - spikes and normalised activations),
#             "bf16x6" (three bf16 pieces, six products: fp32-grade for any range, half the speed),
#             "fp32"   (exact fp32 MFMA, an fmaf chain);
#   backward: "bf16x3" (default: bf16 hi + lo, hi*hi + hi*lo + lo*hi, relative error ~1e-5 of the exact product),
#             "fp32";
#   both    : "bf16"   - the opt-in THROUGHPUT mode: operands rounded once to bf16, ONE product per multiply-add, fp32
#             accumulation and fp32 tensors.  8 significant bits: not a parity mode and never a default (stated
#             tolerances: tests/test_gpu_bf16_mode.py).
# A layer overrides it with ``HipConv2d.forward_precision / .backward_precision`` (BlockGen sets "bf16x6" on
# convolutions fed by an unbounded activation - ReLU / SiLU / SumPool / ConvLSTM - where the fp16 range contract of
# "fp16x3" is not guaranteed by construction).
FORWARD_MODES = {"fp32": _hip.PREC_FP32, "bf16x6": _hip.PREC_BF16X6, "fp16x3": _hip.PREC_FP16X3,
                 "bf16": _hip.PREC_BF16X1}
BACKWARD_MODES = {"fp32": _hip.PREC_FP32, "bf16x3": _hip.PREC_BF16X3, "bf16": _hip.PREC_BF16X1}
DEFAULT_FORWARD_PRECISION = "fp16x3"
DEFAULT_BACKWARD_PRECISION = "bf16x3"


def _checked(mode: str, table: dict, what: str) -> str:
    if mode not in table:
        raise ValueError(f"{what} precision must be one of {sorted(table)}, got {mode!r}")
    return mode


# session defaults; SNN_FORWARD_PRECISION / SNN_BACKWARD_PRECISION preset them (validated here, not in the library)
_forward_precision = _checked(os.environ.get("SNN_FORWARD_PRECISION") or DEFAULT_FORWARD_PRECISION, FORWARD_MODES,
                              "SNN_FORWARD_PRECISION: forward")
_backward_precision = _checked(os.environ.get("SNN_BACKWARD_PRECISION") or DEFAULT_BACKWARD_PRECISION, BACKWARD_MODES,
                               "SNN_BACKWARD_PRECISION: backward")


def set_forward_precision(mode: str) -> None:
    """Default forward arithmetic of convolutions without their own ``forward_precision``."""
    global _forward_precision
    _forward_precision = _checked(mode, FORWARD_MODES, "forward")


def get_forward_precision() -> str:
    return _forward_precision


def set_backward_precision(mode: str) -> None:
    """Default arithmetic of the backward convolutions (data / weight gradients) without their own setting."""
    global _backward_precision
    _backward_precision = _checked(mode, BACKWARD_MODES, "backward")


def get_backward_precision() -> str:
    return _backward_precision


# ------------------------------------------------------------------------------------------- activation storage
# "fp32" (default, the parity path): every activation tensor is fp32 in HBM.
# "bf16": the opt-in bf16-STORAGE throughput mode (the dtype BASELINE configs[1] names).  The wide tensors of a layer-major
#   step - convolution outputs y, spikes / neuron outputs, saved decayed potentials, gradients gx / dy / dx - are bf16 in
#   HBM (half the bytes of every HBM-bound kernel); neuron state (v, i) stays fp32 in registers across T, BatchNorm
#   statistics / coefficients, weights, weight gradients and the optimiser stay fp32, accumulation is fp32 (spikes are
#   exact in bf16).  Convolutions multiply the stored bf16 activations by bf16-rounded weights: one MFMA product
#   (SNN_PREC_BF16S).  The event frames stay fp32 ({0,1}: two channels), and so does everything behind the head's
#   last-step read-out (a few frames).  Not a parity mode: 8 significant bits per stored value; stated tolerances in
#   tests/test_gpu_bf16_storage.py.  The mode is decided where the event frames enter (the Cin = 2 layer writes bf16) and
#   follows the tensors from there: an operator works in the storage type of its input.
STORAGE_MODES = {"fp32": _F32, "bf16": _BF16}
_activation_storage = _checked(os.environ.get("SNN_ACTIVATION_STORAGE") or "fp32", STORAGE_MODES,
                               "SNN_ACTIVATION_STORAGE: storage")


def set_activation_storage(mode: str) -> None:
    """"fp32" (default) or "bf16" (opt-in throughput mode, see above)."""
    global _activation_storage
    if mode not in STORAGE_MODES:
        raise ValueError(f"activation storage must be one of {sorted(STORAGE_MODES)}, got {mode!r}")
    _activation_storage = mode


def get_activation_storage() -> str:
    return _activation_storage


def _prec_codes(forward: Optional[str], backward: Optional[str]) -> Tuple[int, int]:
    """Per-call ``precision`` arguments: the layer's own modes, else the session defaults."""
    return (FORWARD_MODES[_checked(forward or _forward_precision, FORWARD_MODES, "forward")],
            BACKWARD_MODES[_checked(backward or _backward_precision, BACKWARD_MODES, "backward")])


def _conv_precs(prec: Optional[Tuple[int, int]], bf16_storage: bool) -> Tuple[int, int]:
    """``(forward, backward)`` codes of one convolution call: ``prec`` (else the session defaults), or the one-product
    bf16-storage mode for both when the call reads or writes bf16 activations."""
    fwd_prec, bwd_prec = prec if prec is not None else _prec_codes(None, None)
    if bf16_storage:
        fwd_prec = bwd_prec = _hip.PREC_BF16S
    return fwd_prec, bwd_prec


# ------------------------------------------------------------------------------------------- helpers
# Weight gradients do not feed the rest of the backward pass, so they run on a second HIP stream beside the
# data-gradient chain (fills the CUs that small feature maps leave idle).  ``wgrad_stream_sync()`` joins the
# side stream; trainer.FlatTrainer.step() calls it before the all-reduce / optimiser read the gradients.
_SIDE_STREAMS = {}
USE_WGRAD_STREAM = not os.environ.get("SNN_NO_WGRAD_STREAM")   # tuning aid: everything on one stream


# HIP multiplexes its streams onto a few hardware queues (four by default), in the order the streams are first used.  Two
# streams that land on ONE queue run strictly one after the other: with an RCCL communicator created before the model
# (the normal order under torchrun) the weight-gradient stream shared the main stream's queue and the step lost the whole
# overlap - 25.9 instead of 24.7 ms, measured with a one-rank RCCL group (tools/dist_overhead.py).  So a side stream is
# not taken blindly from torch's pool: candidates are PROBED against the stream they are meant to run beside.
STREAM_PROBE_CANDIDATES = 12
_STREAM_PROBE_LOG = []   # (device, candidates tried, concurrent?) per chosen stream - bench.py reports it


def runs_concurrently(candidate: "torch.cuda.Stream", beside: "torch.cuda.Stream") -> bool:
    """True if work queued on ``candidate`` AFTER a long-running job on ``beside`` finishes before that job does (the two
    do not share a hardware queue).  Synchronises the device; about 2 ms."""
    dev = beside.device
    torch.cuda.synchronize(dev)
    big = torch.empty(64 << 20, dtype=torch.float32, device=dev)      # 256 MiB: eight fills are about a millisecond
    small = torch.empty(64, dtype=torch.float32, device=dev)
    e0, e1, c1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    with torch.cuda.stream(beside):
        big.fill_(0.0)                                                # first-touch cost stays outside the timed part
        e0.record(beside)
        for _ in range(8):
            big.fill_(1.0)
        e1.record(beside)
    with torch.cuda.stream(candidate):
        small.fill_(1.0)
        c1.record(candidate)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(c1) < 0.5 * e0.elapsed_time(e1)


def concurrent_stream(beside: "torch.cuda.Stream", avoid=()) -> "torch.cuda.Stream":
    """A stream of ``beside``'s device that really runs beside it (and is none of ``avoid``): the first probed candidate
    from torch's pool that does; the first candidate if none does (the result is still correct, only serial)."""
    dev = beside.device
    tried = []
    for _ in range(STREAM_PROBE_CANDIDATES):
        cand = torch.cuda.Stream(device=dev)
        if any(cand.cuda_stream == o.cuda_stream for o in tuple(avoid) + tuple(tried) + (beside,)):
            continue
        tried.append(cand)
        if runs_concurrently(cand, beside):
            _STREAM_PROBE_LOG.append((str(dev), len(tried), True))
            return cand
    _STREAM_PROBE_LOG.append((str(dev), len(tried), False))
    return tried[0] if tried else torch.cuda.Stream(device=dev)


def _side_stream(device) -> "torch.cuda.Stream":
    st = _SIDE_STREAMS.get(device)
    if st is None:
        st = _SIDE_STREAMS[device] = concurrent_stream(torch.cuda.current_stream(device))
    return st


USE_HEAD_STREAMS = False   # bench.py saves and restores it around its profiled steps; nothing else reads it


# Operands of a side-stream kernel are kept alive HERE until the main stream has waited for that kernel, instead of
# being handed to ``Tensor.record_stream``: a record_stream'ed block returns to the caching allocator only once the
# GPU has really passed the event, and the host enqueues a whole backward pass ahead of the GPU - so every dy of the
# pass stayed reserved at once (257 GiB reserved for 113 GiB live on the 1280x720 B=4 step, and an allocator that
# frees and re-mallocs its cache each step from B=6 on).  Released this way the blocks are recycled in stream order.
_SIDE_PENDING = collections.deque()   # (event recorded on the side stream, tensors its kernels read)
# weight-gradient launches the side stream may lag behind the main stream before the main stream waits for the oldest
WGRAD_SIDE_DEPTH = int(os.environ.get("SNN_WGRAD_SIDE_DEPTH", "1"))


def _side_retire(main, keep: int) -> None:
    """Main stream waits for all but the ``keep`` most recent side-stream launches and drops their operands."""
    while len(_SIDE_PENDING) > keep:
        ev, _tensors = _SIDE_PENDING.popleft()
        main.wait_event(ev)


def _side_hold(side, *tensors) -> None:
    ev = torch.cuda.Event()
    ev.record(side)
    _SIDE_PENDING.append((ev, tensors))


def wgrad_stream_sync() -> None:
    """Make the current stream wait for every weight-gradient kernel queued on the side stream."""
    _SIDE_PENDING.clear()
    for dev, st in _SIDE_STREAMS.items():
        torch.cuda.current_stream(dev).wait_stream(st)


class _WgradLaunch:
    """``with _WgradLaunch(...) as (stream handle, split-K workspace [splitk, rows*cols], G [rows, cols] or None):`` the
    stream and scratch of one weight-gradient launch, both allocated on that stream.  A gradient that goes straight into
    the flat buffer (``slotted``) feeds nothing downstream in autograd, so it runs on the side stream, concurrently with
    the data-gradient chain: the launch before the previous one is joined first (its operands go), the side stream waits
    for the main stream (gy and every earlier use of the slot are complete), and ``hold`` - the tensors the launched
    kernels read - stays alive until the main stream has waited for them.  (A class, not a generator: it runs for every
    weight gradient of a step, on the host's critical path.)"""

    __slots__ = ("device", "on_side", "shape", "hold", "with_g", "stream", "scope")

    def __init__(self, device, slotted: bool, splitk: int, rows: int, cols: int, hold: Sequence[torch.Tensor] = (),
                 with_g: bool = False):
        self.device, self.on_side, self.shape = device, slotted and USE_WGRAD_STREAM, (splitk, rows, cols)
        self.hold, self.with_g = hold, with_g

    def __enter__(self):
        main = torch.cuda.current_stream()
        self.stream = _side_stream(self.device) if self.on_side else main
        if self.on_side:
            _side_retire(main, WGRAD_SIDE_DEPTH)
            self.stream.wait_stream(main)
        self.scope = torch.cuda.stream(self.stream)
        self.scope.__enter__()
        splitk, rows, cols = self.shape
        ws = torch.empty((splitk, rows * cols), device=self.device, dtype=_F32)
        G = torch.empty((rows, cols), device=self.device, dtype=_F32) if self.with_g else None
        return self.stream.cuda_stream, ws, G

    def __exit__(self, *exc):
        self.scope.__exit__(*exc)
        if self.on_side:
            _side_hold(self.stream, *self.hold)


# ------------------------------------------------------------------------------------------- gradient slots
# ------------------------------------------------------------------------------------------- activity counts
_ACTIVITY = None   # the ``activity.Recorder`` of the enclosing ``activity.record(...)`` block, else None: nothing is counted


def _activity_launch(ptr: int, kind: int, ld: int, threshold: float, T: int, M: int, C: int, per_step: bool,
                     counts: torch.Tensor, accumulate: bool) -> None:
    _hip.call("snn_activity_count", ptr, kind, ld, float(threshold), T, M, C, int(bool(per_step)), counts.data_ptr(),
              int(bool(accumulate)), _stream())


def activity_plan(kind: int, T: int, M: int, C: int, ld: int, aligned: bool) -> Tuple[int, int, int, int]:
    """``(channels per access, pixel rows per block, grid x, grid y)`` of the launch ``snn_activity_count`` takes (host only)."""
    out = (ctypes.c_int64 * 4)()
    _hip.call("snn_activity_count_plan", kind, T, M, C, ld, int(bool(aligned)), out)
    return tuple(int(v) for v in out)


def spike_count(x: Optional[torch.Tensor], threshold: Optional[float] = None, mask: Optional[torch.Tensor] = None,
                per_step: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Exact per-channel element counts of a sequence, int64 ``[C]`` (``per_step``: ``[T,C]``), by one launch of
    ``snn_activity_count``; nothing is synchronised.

    ``x`` is ``[T,B,C,H,W]`` channels-last, or a channel slice of such a tensor (``cl_stride``), fp32 or bf16: counted is
    ``x != 0`` (-0.0 is zero; NaN and denormals are not), or, with ``threshold``, ``x > threshold`` (strict, the scans'
    comparison: ``x`` holds saved potentials).  ``mask`` (int32 ``[T,B,H,W,words]``, the spike bit mask of a stage-entry LIF
    scan, possibly the first ``words`` columns of wider rows) is counted instead of ``x``, which then only tells the channel
    count (``x=None``: ``32 * words``).  ``out``: an int64 tensor of the result's shape that the counts are ADDED to."""
    if mask is not None:
        if not mask.is_cuda:   # (_require_device also checks for a float type)
            raise RuntimeError(f"spike_count mask: tensor is on {mask.device}; the MI355X path has no CPU fallback "
                               "(move the model and its inputs to a HIP device)")
        if mask.dim() != 5 or mask.dtype != torch.int32:
            raise RuntimeError("spike_count: the mask is int32 [T,B,H,W,words]")
        T, B, H, W, words = mask.shape
        C = int(x.shape[-3]) if x is not None else 32 * words
        ld = mask.stride(3)
        want = (B * H * W * ld, H * W * ld, W * ld, ld, 1)
        if C % 32 or C // 32 > words or ld < words or any(n > 1 and s != w for n, s, w in zip(mask.shape, mask.stride(), want)):
            raise RuntimeError("spike_count: the mask rows hold C / 32 words (C a multiple of 32) at one pixel stride")
        src, kind, th = mask, _hip.ACTIVITY_MASK, 0.0
    else:
        _require_device(x, "spike_count input", bf16_ok=True)
        if x.dim() != 5 or cl_stride(x) is None:
            raise RuntimeError("spike_count takes a channels-last sequence [T,B,C,H,W] (functional.to_channels_last) or a "
                               "channel slice of one")
        T, B, C, H, W = _dims5(x)
        ld = cl_stride(x)
        bf = x.dtype == _BF16
        if threshold is None:
            kind, th = (_hip.ACTIVITY_NONZERO_BF16 if bf else _hip.ACTIVITY_NONZERO_F32), 0.0
        else:
            kind, th = (_hip.ACTIVITY_ABOVE_BF16 if bf else _hip.ACTIVITY_ABOVE_F32), float(threshold)
        src = x
    shape = (T, C) if per_step else (C,)
    if out is None:
        counts = torch.empty(shape, device=src.device, dtype=torch.int64)
    else:
        if out.dtype != torch.int64 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != src.device:
            raise RuntimeError(f"spike_count: out must be a contiguous int64 tensor of shape {shape} on {src.device}")
        counts = out
    _activity_launch(src.data_ptr(), kind, ld, th, T, B * H * W, C, per_step, counts, out is not None)
    return counts


class GradSlot:
    """Destination of a parameter's gradient inside a flat gradient buffer (``trainer.FlatTrainer``).

    When a parameter carries ``_snn_grad_slot`` the backward kernels write (first use in a step) or
    accumulate (later uses) its gradient straight into ``buf`` - the buffer the data-parallel all-reduce
    and the fused Adamax step work on - and autograd receives no gradient for it (zero copies).
    ``buf`` is dense in the parameter's STORAGE order (OHWI for conv weights).
    """

    __slots__ = ("buf", "written")

    def __init__(self, buf: torch.Tensor):
        self.buf = buf
        self.written = False

    def claim(self) -> int:
        """-> the ``accumulate`` flag for the kernel and mark the slot as holding data."""
        acc = 1 if self.written else 0
        self.written = True
        return acc


_NBT_BATCH = None  # while a model-level forward runs: deferred ``num_batches_tracked`` increments (see soda.py)


def begin_counter_batch() -> None:
    global _NBT_BATCH
    _NBT_BATCH = []


def flush_counter_batch() -> None:
    """Apply the deferred BatchNorm ``num_batches_tracked`` increments in one multi-tensor launch (22 BatchNorms
    = 22 one-element kernels per step otherwise)."""
    global _NBT_BATCH
    pending, _NBT_BATCH = _NBT_BATCH, None
    if pending:
        by_inc = {}
        for t, inc in pending:
            by_inc.setdefault(inc, []).append(t)
        for inc, tensors in by_inc.items():
            torch._foreach_add_(tensors, inc)


FUSE_OUTER_ADDEND = not os.environ.get("SNN_NO_OUTER_ADDEND")  # bisecting aid
# sibling 1x1 convolutions of one input (the C2f split) as ONE convolution (generator.BlockGen._plan_siblings)
USE_SIBLING_FUSION = not os.environ.get("SNN_NO_SIBLING_FUSION")
# a Norm -> LIF layer whose only consumer is such a convolution writes NO spike tensor: the consumer thresholds the saved
# potentials itself (snn_conv1x1_spikes_*; SNN_NO_SPIKES_FROM_VDEC: tuning / bisecting aid)
USE_SPIKES_FROM_VDEC = not os.environ.get("SNN_NO_SPIKES_FROM_VDEC")
# ... and such a layer also writes its spikes as one bit per neuron, which the consumer reads instead of the 32-bit
# potentials where snn_conv1x1_mask_supported covers the call (SNN_NO_SPIKE_MASK: tuning / bisecting aid - no mask is
# written, the consumer thresholds the potentials)
USE_SPIKE_MASK = not os.environ.get("SNN_NO_SPIKE_MASK")
# The mask pays where the potentials are HBM traffic.  A layer whose saved potentials are smaller than one XCD's L2 (4 MiB)
# is served from cache and its convolutions are bound by launch latency: it keeps the potentials path and allocates nothing.
SPIKE_MASK_MIN_BYTES = 4 << 20


class GradAccumulator:
    """Shared by the aliases a block hands to its branches (``fanout``): lets the FIRST data-gradient
    convolution that runs for the fanned-out tensor add the gradients other branches have already produced
    in its epilogue (``snn_conv2d_dgrad(addend=...)``) instead of a separate add pass afterwards."""

    __slots__ = ("deposits", "result", "fused", "outer", "exclusive", "grad_in_slot")

    def __init__(self):
        self.deposits = {}    # alias index -> gradient produced for that alias by a pass-through consumer
        self.result = None    # dx written by the fusing convolution
        self.fused = {}       # alias index -> deposit that went into ``result``
        self.outer = None     # (accumulator, alias index) of the enclosing fanout when the fanned-out tensor is
        #                       itself an alias (Residual inside Dense: the YOLO bottleneck)
        self.exclusive = set()    # keys whose deposit nobody else reads (a channel slice of a concat gradient handed to
        #                           exactly this consumer): the accumulated gradient may be written over it
        self.grad_in_slot = False  # the fanned-out tensor wants its total gradient left IN such a slice (split_channels)

    def deposit(self, key, g: torch.Tensor, exclusive: bool = False) -> None:
        if self.result is None and g is not None:
            self.deposits[key] = g
            if exclusive:
                self.exclusive.add(key)

    def set_result(self, dx: torch.Tensor) -> None:
        self.result = dx


def _acc_of(x):
    return getattr(x, "_snn_acc", None)


def _same_tensor(a: torch.Tensor, b: torch.Tensor) -> bool:
    return (a.data_ptr() == b.data_ptr() and tuple(a.shape) == tuple(b.shape) and a.stride() == b.stride())


def _slot_of(param) -> Optional[GradSlot]:
    return getattr(param, "_snn_grad_slot", None) if param is not None else None


# ------------------------------------------------------------------------------------------- conv
def _dgrad_accumulate(acc, gy, ldg, wt, x, geom, st, prec, wt_split=None, wt_image=None, fuse=None):
    """Data gradient of a convolution with the gradient accumulation of its input folded into the epilogue
    (up to two addends; see ``GradAccumulator``).  ``wt`` is the transposed weight ``[Cin][KH][KW][Cout]``.
    ``fuse(dx, addend, ld_add, addend2, ld_add2) -> bool``: a launch that writes this ``dx`` together with something else
    (``_FusedBwd1x1``); asked once the addends and ``dx`` are settled, True: it ran, no data-gradient kernel is launched here.
    The bookkeeping around the launch is the same either way."""
    T, B, Cin, H, W, Cout, KH, KW, Ho, Wo, stride, pad = geom
    dx, dx_shape = None, (T, B, Cin, H, W)
    addend, ld_add, addend2, ld_add2 = None, 0, None, 0
    outer_fused = None
    if acc is not None and acc[0].result is None and acc[0].deposits:
        # another branch of the block already produced its gradient for this tensor: add it here
        key, other = next(iter(acc[0].deposits.items()))
        other = _raw_to_cl(other)
        if tuple(other.shape) == dx_shape:
            addend, ld_add = other.data_ptr(), cl_stride(other)
            acc[0].fused[key] = acc[0].deposits.pop(key)
    if (acc is not None and acc[0].result is None and not acc[0].deposits and acc[0].outer is not None
            and FUSE_OUTER_ADDEND):
        # the tensor is itself one alias of an enclosing fanout whose other consumer already deposited
        # its gradient (bottleneck input: conv + residual shortcut + Dense pass-through): second addend
        o_acc, o_key = acc[0].outer
        if o_acc.result is None and len(o_acc.deposits) == 1 and o_key not in o_acc.deposits:
            key2, other2 = next(iter(o_acc.deposits.items()))
            other2 = _raw_to_cl(other2)
            if tuple(other2.shape) == dx_shape:
                addend2, ld_add2 = other2.data_ptr(), cl_stride(other2)
                outer_fused = (o_acc, o_key, key2)
                if (o_acc.grad_in_slot and key2 in o_acc.exclusive and other2.dtype == x.dtype and ld_add2 % 4 == 0
                        and USE_SIBLING_FUSION):
                    # the total is written over the concat-gradient slice it contains (every kernel's epilogue reads an
                    # addend element and stores the sum from the same lane): the gradient of a split_channels part then
                    # lies next to its siblings' and the fused convolution reads them as ONE channel-sliced tensor
                    dx = _alias(other2, other2.storage_offset(), T, B, Cin, H, W, ld_add2)
    chained = False
    if (acc is not None and acc[0].result is not None and addend is None and acc[1] not in acc[0].fused
            and tuple(acc[0].result.shape) == dx_shape):
        # a sibling convolution already produced (its gradient + the fused deposits) for this tensor: add
        # that here and become the accumulated result (two convolutions on one input: the C2f split)
        prev = acc[0].result
        addend, ld_add = prev.data_ptr(), cl_stride(prev)
        chained = True
    if dx is None:
        dx = _new_cl((T, B), Cin, H, W, x)
    if fuse is not None and fuse(dx, addend, ld_add, addend2, ld_add2):
        pass
    elif (prec in _HALO_BWD_PRECS and _halo_operand_ok(gy.data_ptr(), ldg, prec == _hip.PREC_BF16S) and USE_HALO_CONV
            and (KH, KW, stride, pad) == (3, 3, 2, 1)
            and _hip.query("snn_conv3x3_s2_dgrad_supported", T * B, H, W, Cin, Ho, Wo, Cout)):
        # stride 2: all four phase classes of dx from ONE staged pass over dy (k_conv_s2dgrad3)
        if wt_image is None:
            wt_image = _frag_image(wt, Cin, Cout, 1, _hip.PREC_BF16X3)
        _hip.call("snn_conv3x3_s2_dgrad", gy.data_ptr(), ldg, wt_image.data_ptr(), dx.data_ptr(), cl_stride(dx), T * B, H, W, Cin, Ho,
                  Wo, Cout, addend, ld_add, addend2, ld_add2, prec, st)
    elif (prec in _HALO_BWD_PRECS and _halo_operand_ok(gy.data_ptr(), ldg, prec == _hip.PREC_BF16S)
            and _halo_ok(T * B, H, W, Cout, Cin, KH, KW, stride, pad)):
        # dx = conv3x3(dy, mirrored taps of w^T): the halo-resident kernel with the data gradient's weight image
        if wt_image is None:
            wt_image = _frag_image(wt, Cin, Cout, 1, _hip.PREC_BF16X3)
        _hip.call("snn_conv3x3_halo", gy.data_ptr(), ldg, wt_image.data_ptr(), dx.data_ptr(), cl_stride(dx), T * B, H, W, Cout,
                  Cin, addend, ld_add, addend2, ld_add2, None, 0, None, prec, st)
    else:
        _hip.call("snn_conv2d_dgrad", gy.data_ptr(), ldg, wt.data_ptr(), wt_split, dx.data_ptr(), cl_stride(dx), T * B, H, W,
                  Cin, Ho, Wo, Cout, KH, KW, stride, pad, addend, ld_add, addend2, ld_add2, prec, st)
    if acc is not None and (acc[0].result is None or chained):
        if chained and acc[0].outer is not None and acc[0].outer[0].result is acc[0].result:
            acc[0].outer[0].set_result(dx)                 # the enclosing fanout expects what this
            acc[0].outer[0].fused[acc[0].outer[1]] = dx    # fanout will hand back: the new total
        acc[0].set_result(dx)
        acc[0].fused[acc[1]] = dx
    if outer_fused is not None:
        o_acc, o_key, key2 = outer_fused
        o_acc.fused[key2] = o_acc.deposits.pop(key2)
        o_acc.fused[o_key] = dx   # what the inner fanout will hand back for this alias
        o_acc.set_result(dx)
    return dx


# A stride-1 1x1 convolution that owes both gradients runs ONE kernel over dy where snn_conv1x1_bwd_supported covers the
# call: the weight-gradient kernel also writes dx (k_conv_wgrad_pipe DX; SNN_NO_FUSED_BWD1X1: A/B and bisecting aid - the
# two launches, same bits)
USE_FUSED_BWD1X1 = not os.environ.get("SNN_NO_FUSED_BWD1X1")
# The fusion removes one HBM read of dy.  A dy smaller than one XCD's L2 (4 MiB) is read the second time from cache, its
# launches are latency-bound and the fused kernel (fewer resident waves) has nothing to win: such a layer keeps its two
# launches, as a layer below SPIKE_MASK_MIN_BYTES keeps its potentials.
FUSED_BWD1X1_MIN_BYTES = 4 << 20


class _FusedBwd1x1:
    """The ``fuse`` hook of ``_dgrad_accumulate`` for a 1x1 / stride 1 convolution whose weight gradient is wanted too.
    ``xop`` is the weight gradient's x operand - the fp32 activations, or (``is_mask``) the spike bit mask - with its pixel
    stride.  Called, it asks the query with the settled ``dx`` and addends and, on a yes, launches the fused kernel on the
    CURRENT stream (dx is on the critical path) into a split-K workspace allocated there: ``ws`` then holds the slabs and
    the caller reduces them (``snn_conv2d_wgrad_reduce``) on the weight-gradient stream, keeping ``ws`` in that launch's
    ``hold`` so that it is neither freed nor reused before the reduction has run."""

    __slots__ = ("gy", "ldg", "wt", "xop", "ldxop", "is_mask", "geom", "prec", "splitk", "ws")

    def __init__(self, gy, ldg, wt, xop, ldxop, is_mask, geom, prec, splitk):
        self.gy, self.ldg, self.wt, self.xop, self.ldxop, self.is_mask = gy, ldg, wt, xop, ldxop, is_mask
        self.geom, self.prec, self.splitk, self.ws = geom, prec, splitk, None

    @staticmethod
    def eligible(geom, prec, gy, x) -> bool:
        T, B, _, H, W, Cout = geom[:6]
        return (USE_FUSED_BWD1X1 and tuple(geom[6:8]) == (1, 1) and tuple(geom[10:12]) == (1, 0)
                and T * B * H * W * Cout * 4 >= FUSED_BWD1X1_MIN_BYTES and prec == _hip.PREC_BF16X3 and gy.dtype == _F32 and x.dtype == _F32)

    def __call__(self, dx, addend, ld_add, addend2, ld_add2) -> bool:
        T, B, Cin, H, W, Cout = self.geom[:6]
        tail = (self.gy.data_ptr(), self.ldg, self.wt.data_ptr(), dx.data_ptr(), cl_stride(dx), addend, ld_add, addend2, ld_add2)
        if not _hip.query("snn_conv1x1_bwd_supported", T * B, H, W, Cin, Cout, self.xop.data_ptr(), self.ldxop,
                          int(self.is_mask), *tail, None, self.splitk, self.prec):
            return False
        self.ws = torch.empty((self.splitk, Cout * Cin), device=dx.device, dtype=_F32)
        _hip.call("snn_conv1x1_mask_bwd" if self.is_mask else "snn_conv1x1_bwd", self.xop.data_ptr(), self.ldxop, *tail, None,
                  T * B, H, W, Cin, Cout, 0, self.ws.data_ptr(), self.splitk, self.prec, _stream())
        return True


# Halo-resident 3x3 kernel (csrc/conv_halo.hip) for the 64 / 128-channel stride-1 layers, forward and data gradient
# (SNN_NO_HALO_CONV: tuning / bisecting aid - the implicit GEMM everywhere)
USE_HALO_CONV = not os.environ.get("SNN_NO_HALO_CONV")
# backward modes the halo kernels take; both read the bf16 x 3 image of the transposed weights (bf16 storage: hi pieces only)
_HALO_BWD_PRECS = (_hip.PREC_BF16X3, _hip.PREC_BF16S)


def _halo_ok(N: int, H: int, W: int, Cin: int, Cout: int, KH: int, KW: int, stride: int, pad: int) -> bool:
    return (USE_HALO_CONV and KH == 3 and KW == 3 and stride == 1 and pad == 1
            and bool(_hip.query("snn_conv3x3_halo_supported", N, H, W, Cin, Cout)))


def _halo_operand_ok(ptr: int, ld: int, bf16: bool) -> bool:
    """The operand the halo-resident kernels stage (snn_conv3x3_halo x / dy, snn_conv3x3_s2_dgrad dy): pixel stride a
    multiple of 4 and 16-byte aligned (8 for bf16 storage).  A channel slice of a concat buffer or of a concat gradient at
    another offset is not; the implicit GEMM takes it instead."""
    return ld % 4 == 0 and ptr % (8 if bf16 else 16) == 0


def _spikes_fwd_ok(supported: bool, halo: bool, x_ptr: int, w_ptr: int) -> bool:
    """A convolution over saved potentials can run its thresholding forward kernel.  ``supported``: the shape query
    (snn_conv2d_spikes_supported / snn_conv1x1_spikes_supported), which sees shapes and strides only.  The implicit GEMM
    (k_conv_gather XSP) also needs 16-byte aligned potentials and weight - a FlatTrainer parameter may start on any float
    of the flat buffer; the halo-resident kernel reads its own weight image instead (``halo``)."""
    return bool(supported) and x_ptr % 16 == 0 and (halo or w_ptr % 16 == 0)


def _spikes_wgrad_ok(x_ptr: int, ldx: int, gy_ptr: int, ldg: int) -> bool:
    """The thresholding weight gradient (snn_conv2d_spikes_wgrad) covers the pipelined kernel only - the halo-resident one
    drops to it for buffers it cannot address: pixel strides multiples of 4 and 16-byte aligned potentials AND output
    gradient.  A gradient that is a slice of a concat gradient at another channel offset fails that; its convolution
    writes the spikes out for its weight gradient instead."""
    return ldx % 4 == 0 and ldg % 4 == 0 and x_ptr % 16 == 0 and gy_ptr % 16 == 0


def _spikes_dense(x: torch.Tensor, x_th: float) -> torch.Tensor:
    """z = (x > x_th) of saved potentials ``x`` ([T,B,C,H,W] channels-last view) as a dense fp32 spike tensor."""
    return _cl_view((x.permute(0, 1, 3, 4, 2) > x_th).to(_F32).contiguous())


def _spikes_fwd_operand(x: torch.Tensor, x_th: Optional[float], covered) -> Tuple[torch.Tensor, Optional[float]]:
    """Forward operand of a convolution: ``(x, x_th)`` when ``x`` holds no potentials or a thresholding kernel takes the
    call (``covered()``, asked only then: the call's own test on top of ``_spikes_fwd_ok``), else the spikes written out
    after all and no threshold."""
    if x_th is None or covered():
        return x, x_th
    return _spikes_dense(x, x_th), None


def _spikes_wgrad_operand(x: torch.Tensor, ldx: int, x_th: Optional[float], gy: torch.Tensor, ldg: int):
    """Weight-gradient operand -> ``(operand, its pixel stride, threshold)``: the potentials and their threshold where
    ``_spikes_wgrad_ok``, else the spikes written out (same bits: the plain kernel on the stored spikes) and no
    threshold."""
    if x_th is None or _spikes_wgrad_ok(x.data_ptr(), ldx, gy.data_ptr(), ldg):
        return x, ldx, x_th
    z = _spikes_dense(x, x_th)
    return z, cl_stride(z), None


def _frag_image(src: torch.Tensor, O: int, I: int, flip: int, prec: int) -> torch.Tensor:
    """Weight image in MFMA-fragment order of ONE ``[O][3][3][I]`` matrix (snn_weight_frag_image_batched with a
    one-row table): what a layer without a FlatTrainer-kept image builds per call (one small launch)."""
    img = torch.empty((9 * O * I,), device=src.device, dtype=_F32)
    table = torch.tensor([[0, 0, O, I]], dtype=torch.int64, device=src.device)
    _hip.call("snn_weight_frag_image_batched", src.data_ptr(), img.data_ptr(), table.data_ptr(), 1,
              9 * (I // 32) * (O // 32) * 128, flip, prec, _stream())
    return img


def _kept_view(weight, name: str, frag_prec: int = _hip.PREC_FP16X3) -> Optional[torch.Tensor]:
    """A weight view FlatTrainer keeps on the parameter and refreshes once per optimiser step (``_snn_wt``,
    ``_snn_w16``, ``_snn_wt16``, ``_snn_wfrag``, ``_snn_wtfrag``; tensor views, alive as long as the parameter is), or
    None: the parameter does not live in a FlatTrainer, it changed since the last refresh (version counter), or - the
    forward fragment image - the image holds the pieces of another precision than ``frag_prec``."""
    view = getattr(weight, name, None)
    if view is None or weight._snn_wt_version != weight._version:
        return None
    if name == "_snn_wfrag" and getattr(weight, "_snn_wfrag_prec", _hip.PREC_FP16X3) != frag_prec:
        return None
    return view


class PendingBnApply(NamedTuple):
    """Second phase of a train-mode BatchNorm backward that has NOT been run: dy = A[t,c]*gx + B[t,c]*y + C[t,c]
    (snn_bn_bwd_apply).  ``_AffineNeuron.backward`` hands its producer convolution gx together with this record when that
    convolution announced (``y._snn_defer_apply``) that its backward forms dy while reading it (snn_conv2d_wgrad_bn):
    the 12-bytes-per-element apply pass and the dy tensor disappear."""
    gx: torch.Tensor      # dense [T,B,H,W,C]
    y: torch.Tensor       # the convolution output saved for the BatchNorm backward ([T,B,C,H,W], channels-last)
    coef: torch.Tensor    # [3, T, C]
    dims: Tuple[int, int, int, int, int]   # T, B, C, H, W


_PENDING_APPLY = {}   # gx.data_ptr() -> PendingBnApply
USE_DEFERRED_BN_APPLY = not os.environ.get("SNN_NO_DEFERRED_BN_APPLY")   # tuning / bisecting aid


def reset_backward_state() -> None:
    """Drop records of a backward pass that did not finish (an exception between the two nodes)."""
    _PENDING_APPLY.clear()


def _apply_pending(pend: PendingBnApply) -> None:
    """The classic second phase, in place: gx becomes dy."""
    T, B, C, H, W = pend.dims
    _hip.call("snn_bn_bwd_apply_bf16" if pend.gx.dtype == _BF16 else "snn_bn_bwd_apply", pend.gx.data_ptr(), pend.y.data_ptr(), cl_stride(pend.y), pend.coef[0].data_ptr(),
              pend.coef[1].data_ptr(), pend.coef[2].data_ptr(), pend.gx.data_ptr(), C, T, B * H * W, C, 0, _stream())


def _wgrad_bn_ok(x: torch.Tensor, weight: torch.Tensor, stride: int, pad: int) -> bool:
    """The convolution's backward can apply the BatchNorm-backward affine itself: in its weight gradient, when nothing
    else needs dy (the event-frame layer)."""
    if not (USE_DEFERRED_BN_APPLY and weight.requires_grad and x.dim() == 5) or x.requires_grad:
        return False
    T, B, Cin, H, W = x.shape
    Cout, _, KH, KW = weight.shape
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    return bool(_hip.query("snn_conv2d_wgrad_bn_supported", T * B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad))


class _Conv2d(Function):
    """nn.Conv2d(bias=False, padding=int(k/2), stride) over all T*B frames (layer_gen.py:129-136)."""

    @staticmethod
    def forward(ctx, x, weight, stride: int, pad: int, slot=None, dest=None, acc=None, prec=None, bn_out=None, x_th=None):
        # x_th (a float): x holds the saved POTENTIALS of a LIF layer that wrote no spike tensor; the operand is
        # z = (x > x_th), formed by the kernels while they read (snn_conv2d_spikes_* / snn_conv3x3_halo_spikes)
        _require_device(x, "conv2d input", bf16_ok=True)
        _require_device(weight, "conv2d weight")
        T, B, Cin, H, W = _dims5(x)
        Cout, Cin_w, KH, KW = weight.shape
        # bf16 storage: follows the input; enters at the event-frame layer (fp32 {0,1} frames in, bf16 out)
        sb = x.dtype == _BF16 or (_activation_storage == "bf16" and Cin == 2 and (KH, KW) == (3, 3))
        fwd_prec, bwd_prec = _conv_precs(prec, sb)
        if Cin_w != Cin:
            raise RuntimeError(f"conv2d: input has {Cin} channels, weight expects {Cin_w}")
        Ho = (H + 2 * pad - KH) // stride + 1
        Wo = (W + 2 * pad - KW) // stride + 1
        x = _raw_to_cl(x)
        w = weight.detach()
        w_ohwi = w if is_channels_last(w) else _raw_dense_cl(w)
        x, x_th = _spikes_fwd_operand(x, x_th, lambda: not sb and _spikes_fwd_ok(
            _hip.query("snn_conv2d_spikes_supported", T * B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, cl_stride(x),
                       fwd_prec, bwd_prec),
            _halo_ok(T * B, H, W, Cin, Cout, KH, KW, stride, pad), x.data_ptr(), w_ohwi.data_ptr()))
        if _ACTIVITY is not None:
            _ACTIVITY.count_conv((weight,), x, x_th, None, Cout, KH, KW, stride)
        y = _out_tensor(dest, T, B, Cout, Ho, Wo, x, _BF16 if sb else None)
        partial = layout = None
        if bn_out is not None:  # a train-mode BatchNorm follows: its statistics come out of this kernel's epilogue
            n_part = _hip.query("snn_conv2d_fwd_bn_partial_size", T * B, B, Ho, Wo, Cout)
            partial = torch.empty((n_part,), device=x.device, dtype=torch.float64)
            layout = (ctypes.c_int * 2)()
        # FlatTrainer keeps a pre-split image of the weights: ready-made pieces
        w16 = None
        if fwd_prec == _hip.PREC_FP16X3 and USE_PRESPLIT_WEIGHTS and w_ohwi is w:
            w16 = _ptr(_kept_view(weight, "_snn_w16"))
        halo = (_halo_ok(T * B, H, W, Cin, Cout, KH, KW, stride, pad)
                and _halo_operand_ok(x.data_ptr(), cl_stride(x), x.dtype == _BF16))
        if halo and fwd_prec in (_hip.PREC_FP16X3, _hip.PREC_BF16S):
            # the image holds fp16 pieces (fp16 x 3) or bf16 pieces (bf16 storage: the hi pieces are the rounded weights)
            img_prec = _hip.PREC_BF16X3 if sb else _hip.PREC_FP16X3
            img = _kept_view(weight, "_snn_wfrag", img_prec) if w_ohwi is w else None
            if img is None:
                img = _frag_image(w_ohwi, Cout, Cin, 0, img_prec)
            if x_th is not None:
                _hip.call("snn_conv3x3_halo_spikes", x.data_ptr(), cl_stride(x), x_th, img.data_ptr(), y.data_ptr(),
                          cl_stride(y), T * B, H, W, Cin, Cout, _ptr(partial), B, layout, _stream())
            else:
                _hip.call("snn_conv3x3_halo", x.data_ptr(), cl_stride(x), img.data_ptr(), y.data_ptr(), cl_stride(y), T * B,
                          H, W, Cin, Cout, None, 0, None, 0, _ptr(partial), B, layout, fwd_prec, _stream())
        elif x_th is not None:
            _hip.call("snn_conv2d_spikes_fwd", x.data_ptr(), cl_stride(x), x_th, w_ohwi.data_ptr(), y.data_ptr(), cl_stride(y),
                      T * B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, _ptr(partial), B, layout, _stream())
        else:
            _hip.call("snn_conv2d_fwd", x.data_ptr(), cl_stride(x), w_ohwi.data_ptr(), w16, y.data_ptr(), cl_stride(y),
                      T * B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, None, 0, _ptr(partial), B, layout, fwd_prec,
                      _stream())
        if layout is not None and layout[0] > 0:
            bn_out.append(BnPartial(partial, int(layout[0]), int(layout[1]), y.data_ptr(), (T, B * Ho * Wo, Cout)))
        ctx.prec = bwd_prec
        ctx.x_th = x_th
        ctx.save_for_backward(x, w_ohwi)
        ctx.weight = weight   # (FlatTrainer's w^T views, _kept_view)
        ctx.geom = (T, B, Cin, H, W, Cout, KH, KW, Ho, Wo, stride, pad)
        ctx.slot = slot
        ctx.acc = acc
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w_ohwi = ctx.saved_tensors
        T, B, Cin, H, W, Cout, KH, KW, Ho, Wo, stride, pad = ctx.geom
        gy = _raw_to_cl(gy)
        ldg, ldx = cl_stride(gy), cl_stride(x)
        st = _stream()
        dx = dw = None
        pend = _PENDING_APPLY.pop(gy.data_ptr(), None)
        if pend is not None:
            fused = (not ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and ctx.slot is not None
                     and pend.gx.dtype == _F32 and pend.dims == (T, B, Cout, Ho, Wo) and cl_stride(pend.y) % 4 == 0
                     and _hip.query("snn_conv2d_wgrad_bn_supported", T * B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad))
            if fused:
                # dy is formed while the weight-gradient kernel reads gx and y: no apply pass, no dy tensor
                splitk = _hip.query("snn_conv2d_wgrad_splitk", T * B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ctx.prec)
                with _WgradLaunch(x.device, True, splitk, Cout, KH * KW * Cin,
                                   hold=(x, pend.gx, pend.y, pend.coef)) as (stream, ws, _):
                    _hip.call("snn_conv2d_wgrad_bn", x.data_ptr(), ldx, pend.gx.data_ptr(), Cout, pend.y.data_ptr(),
                              cl_stride(pend.y), pend.coef.data_ptr(), T, B, ctx.slot.buf.data_ptr(), T * B, H, W, Cin, Ho,
                              Wo, Cout, KH, KW, stride, pad, ctx.slot.claim(), ws.data_ptr(), splitk, stream)
                return None, None, None, None, None, None, None, None, None, None
            _apply_pending(pend)   # this convolution takes a materialised dy after all
        fuse = None
        if ctx.needs_input_grad[0]:
            wt = _kept_view(ctx.weight, "_snn_wt")   # transposed once per optimiser step for all layers (FlatTrainer)
            wt16 = wt_img = None
            if wt is not None:
                wt_img = _kept_view(ctx.weight, "_snn_wtfrag")   # ... and arranged for the halo-resident data gradient
                if ctx.prec == _hip.PREC_BF16X3 and USE_PRESPLIT_WEIGHTS and USE_PRESPLIT_DGRAD:
                    wt16 = _ptr(_kept_view(ctx.weight, "_snn_wt16"))   # ... and pre-split into its bf16 pieces
            else:
                wt = torch.empty((Cin, KH, KW, Cout), device=x.device, dtype=_F32)
                _hip.call("snn_weight_transpose", w_ohwi.data_ptr(), wt.data_ptr(), Cout, KH, KW, Cin, st)
            if ctx.needs_input_grad[1] and ctx.x_th is None and _FusedBwd1x1.eligible(ctx.geom, ctx.prec, gy, x):
                # plain 1x1: dx and the weight-gradient slabs from one pass over gy (when the query covers the call)
                fuse = _FusedBwd1x1(gy, ldg, wt, x, ldx, False, ctx.geom, ctx.prec, _hip.query(
                    "snn_conv2d_wgrad_splitk", T * B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ctx.prec))
            dx = _dgrad_accumulate(ctx.acc, gy, ldg, wt, x, ctx.geom, st, ctx.prec, wt_split=wt16, wt_image=wt_img, fuse=fuse)
        if ctx.needs_input_grad[1]:
            splitk = _hip.query("snn_conv2d_wgrad_splitk", T * B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ctx.prec)
            xw, ldxw, x_th = _spikes_wgrad_operand(x, ldx, ctx.x_th, gy, ldg)
            slot = ctx.slot
            fws = fuse.ws if fuse is not None else None   # the slabs are there already: only their reduction is left
            with _WgradLaunch(x.device, slot is not None, 0 if fws is not None else splitk, Cout, KH * KW * Cin,
                              hold=(x, xw, gy, fws)) as (stream, ws, _):
                if slot is not None:
                    dst, accumulate = slot.buf, slot.claim()
                else:
                    dst, accumulate = torch.empty((Cout, KH, KW, Cin), device=x.device, dtype=_F32), 0
                if fws is not None:
                    _hip.call("snn_conv2d_wgrad_reduce", fws.data_ptr(), dst.data_ptr(), Cout * Cin, splitk, accumulate, stream)
                elif x_th is not None:   # x holds potentials: thresholded on load
                    _hip.call("snn_conv2d_spikes_wgrad", xw.data_ptr(), ldxw, x_th, gy.data_ptr(), ldg, dst.data_ptr(),
                              T * B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, accumulate, ws.data_ptr(), splitk,
                              stream)
                else:
                    _hip.call("snn_conv2d_wgrad", xw.data_ptr(), ldxw, gy.data_ptr(), ldg, dst.data_ptr(), T * B, H, W,
                              Cin, Ho, Wo, Cout, KH, KW, stride, pad, accumulate, ws.data_ptr(), splitk, ctx.prec,
                              stream)
            if slot is None:
                dw = dst.permute(0, 3, 1, 2)
        return dx, dw, None, None, None, None, None, None, None, None


def _small_gemm(a: torch.Tensor, trans_a: bool, b: torch.Tensor, trans_b: bool, c: torch.Tensor, accumulate: int,
                ct: Optional[torch.Tensor] = None, ct_col: int = 0) -> None:
    """``c (+)= op(a) @ op(b)`` on dense row-major fp32 matrices (``snn_small_gemm``, current stream); ``ct``: the
    transposed result from the same launch - ``[n, m]``, or columns ``ct_col .. ct_col + m`` of a wider ``[n, M]`` matrix."""
    m, n = c.shape
    k = a.shape[0] if trans_a else a.shape[1]
    ct_ptr, ldct = (None, 0) if ct is None else (ct.data_ptr() + 4 * ct_col, ct.shape[1])
    _hip.call("snn_small_gemm", a.data_ptr(), a.shape[1], int(trans_a), b.data_ptr(), b.shape[1], int(trans_b),
              c.data_ptr(), n, m, n, k, int(accumulate), ct_ptr, ldct, _stream())


class _SplitChannels(Function):
    """Channel ranges of one channels-last tensor as separate tensors (aliases, no copy): the branch inputs behind a
    fused sibling convolution.  Backward wants ONE gradient for the whole tensor: the parts ask (``_snn_grad_in_slot``)
    that their accumulated gradients be left in the concat-gradient slices they contain (``_dgrad_accumulate``), which
    for sibling outputs that sit side by side in a Dense merge are side by side too - then the gradients ARE one
    channel-sliced tensor; otherwise they are gathered by the strided copy kernel."""

    @staticmethod
    def forward(ctx, x, widths):
        T, B, C, H, W = _dims5(x)
        if sum(widths) != C:
            raise RuntimeError(f"split_channels: widths {widths} do not add up to {C} channels")
        ctx.widths, ctx.like = tuple(widths), (T, B, H, W)
        ld, outs, off = cl_stride(x), [], 0
        for c in widths:
            t = _alias(x, x.storage_offset() + off, T, B, c, H, W, ld)
            t._snn_grad_in_slot = True
            outs.append(t)
            off += c
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        T, B, H, W = ctx.like
        live = [g for g in gs if g is not None]
        if not live:
            return None, None
        gs = [None if g is None else _raw_to_cl(g) for g in gs]
        first = gs[0]
        joined = first is not None
        if joined:
            ld, base, off = cl_stride(first), first.untyped_storage().data_ptr(), first.storage_offset()
            for g, c in zip(gs, ctx.widths):
                if (g is None or g.untyped_storage().data_ptr() != base or g.storage_offset() != off or cl_stride(g) != ld
                        or g.dtype != first.dtype or tuple(g.shape) != (T, B, c, H, W)):
                    joined = False
                    break
                off += c
        if joined:
            return _alias(first, first.storage_offset(), T, B, sum(ctx.widths), H, W, ld), None
        like = live[0]
        out = _new_cl((T, B), sum(ctx.widths), H, W, like)
        off = 0
        for g, c in zip(gs, ctx.widths):
            dst = out.narrow(2, off, c)
            if g is None:
                dst.zero_()
            else:
                _copy_cl(g, dst)
            off += c
        return out, None


def split_channels(x: torch.Tensor, widths: Sequence[int]) -> List[torch.Tensor]:
    return list(_SplitChannels.apply(x, tuple(int(c) for c in widths)))


# FlatTrainer builds the stacked (composed) weight of every registered group and its transpose once per optimiser step,
# all groups in ONE launch (snn_small_gemm_batched, trainer.FlatTrainer._refresh_composed).  Both the registration and
# the product live on the group's first w2 and are keyed by the WHOLE group (``_group_key``): a group registers itself on
# first use (``w2s[0]._snn_sibling_group[key] = (w1, w2s)``) and the trainer fills ``w2s[0]._snn_sibling_weight[key] =
# (w1, w2s, version counters, [w2_0; w2_1; ...] w1, its transpose)``.  The same w2a opens a two-branch group in a training
# step and a one-branch group (``composed_conv1x1``) in a streaming prediction: two entries side by side.
def _group_key(w1: torch.Tensor, w2s: Sequence[torch.Tensor]) -> Tuple[int, ...]:
    return (id(w1),) + tuple(id(w) for w in w2s)


def _group_versions(w1: torch.Tensor, w2s: Sequence[torch.Tensor]) -> Tuple[int, ...]:
    return tuple(w._version for w in w2s) + (w1._version,)


def _kept_product(w1: torch.Tensor, w2s: Sequence[torch.Tensor], shape: Tuple[int, int]):
    """``(wc, wct)``: FlatTrainer's product of this group while every version counter matches, else None (same fmaf
    chains, same bits as the per-call product)."""
    kept = getattr(w2s[0], "_snn_sibling_weight", None)
    entry = kept.get(_group_key(w1, w2s)) if kept is not None else None
    if entry is None:
        return None
    k1, k2s, versions, wc, wct = entry
    if (k1 is w1 and all(a is b for a, b in zip(k2s, w2s)) and versions == _group_versions(w1, w2s)
            and tuple(wc.shape) == shape):
        return wc, wct
    return None


class _SiblingConv1x1(Function):
    """Several plain 1x1 convolutions of ONE input as one convolution with the row-stacked weight - the two
    ``Conv(c/2, 1)`` that open the branches of a C2f block (``models/tiny_yolo.py:84-85``), whose outputs sit side by side
    in the block's Dense merge - optionally each composed with a shared 1x1 convolution in front (``w1``: the C2f entry
    ``Conv(c, 1)``, ``models/tiny_yolo.py:76-82``, with no Norm / neuron in between).  The input is read once instead of
    once per branch; backward is ONE data gradient (instead of two chained through an addend: one read and one write of
    dx less) and ONE pixel reduction ``G = sum gy x^T`` whose row blocks give the branches' weight gradients.
    Arithmetic per output element is that of the separate convolutions (the same k-ordered products); only ``dw1`` sums its
    branch contributions in another order.

    Composition: both maps are linear, so ``y_b = (w2_b w1) x``.  Forward runs the convolution with the composed weight;
    backward needs neither ``conv(x, w1)`` nor its gradient: ``dw2_b = G_b w1^T``, ``dw1 = sum_b w2_b^T G_b`` and
    ``dx = conv^T(gy, [w2_0; w2_1; ...] w1)``.  The composed weight is rounded once in fp32 (a re-association of the
    reference's two fp32 sums, same error level as any other summation order).  With one ``w2`` this is
    ``composed_conv1x1``."""

    @staticmethod
    def forward(ctx, x, w1, dest, acc, prec, slot1, slots2, x_th, x_mask, *w2s):
        """``x_th`` (not None): ``x`` holds the saved potentials of the LIF layer in front (``affine_neuron(spikes_ok=True)``),
        the operand is ``z = (x > x_th)``; ``x_mask`` (not None): the same spikes as the bit mask that layer's scan wrote
        (``[T,B,H,W,ceil(C/32)]`` int32), read instead of the potentials where ``snn_conv1x1_mask_supported`` says so."""
        _require_device(x, "conv2d input", bf16_ok=True)
        fwd_prec, bwd_prec = _conv_precs(prec, x.dtype == _BF16)
        T, B, Cin, H, W = _dims5(x)
        C1 = w1.shape[0] if w1 is not None else Cin
        widths = [int(w.shape[0]) for w in w2s]
        Ct = sum(widths)
        for w in w2s:
            if w.shape[1] != C1 or tuple(w.shape[2:]) != (1, 1):
                raise RuntimeError("sibling 1x1 convolutions: weight shapes do not match the input")
        if w1 is not None and (w1.shape[1] != Cin or tuple(w1.shape[2:]) != (1, 1)):
            raise RuntimeError("sibling 1x1 convolutions: the composed weight does not chain")
        x = _raw_to_cl(x)
        w1m = None if w1 is None else w1.detach().reshape(C1, Cin).contiguous()
        w2ms = [w.detach().reshape(c, C1).contiguous() for w, c in zip(w2s, widths)]
        need_t = ctx.needs_input_grad[0]
        kept = _kept_product(w1, w2s, (Ct, Cin)) if w1 is not None else None
        if kept is not None:
            wc, wct = kept
        else:
            if w1 is not None and all(getattr(w, "_snn_wt", None) is not None for w in (w1, *w2s)):
                # all live in a FlatTrainer's flat buffer: the group is served from its next refresh on
                if getattr(w2s[0], "_snn_sibling_group", None) is None:
                    w2s[0]._snn_sibling_group = {}
                w2s[0]._snn_sibling_group[_group_key(w1, w2s)] = (w1, tuple(w2s))
            wc = torch.empty((Ct, Cin), device=x.device, dtype=_F32)
            # ... and the transpose, the operand of the data gradient, out of the same launches (same fmaf chains)
            wct = torch.empty((Cin, Ct), device=x.device, dtype=_F32) if need_t else None
            row = 0
            for w2m, c in zip(w2ms, widths):
                if w1m is not None:
                    _small_gemm(w2m, False, w1m, False, wc[row:row + c], 0, ct=wct, ct_col=row)
                else:
                    wc[row:row + c].copy_(w2m)
                row += c
            if w1m is None and need_t:
                wct.copy_(wc.t())
        y = _out_tensor(dest, T, B, Ct, H, W, x)
        x, x_th = _spikes_fwd_operand(x, x_th, lambda: _spikes_fwd_ok(
            _hip.query("snn_conv1x1_spikes_supported", T * B, H, W, Cin, Ct, cl_stride(x), fwd_prec, bwd_prec), False,
            x.data_ptr(), wc.data_ptr()))
        if x_th is None:
            x_mask = None
        reads_mask = x_mask is not None and bool(_hip.query(
            "snn_conv1x1_mask_supported", T * B, H, W, Cin, Ct, x_mask.data_ptr(), x_mask.shape[-1], wc.data_ptr(),
            y.data_ptr(), cl_stride(y), None, 0, None, fwd_prec, bwd_prec))
        if _ACTIVITY is not None:
            _ACTIVITY.count_conv(((w1,) if w1 is not None else ()) + tuple(w2s), x, x_th, x_mask if reads_mask else None,
                                 Ct, 1, 1, 1)
        if reads_mask:
            _hip.call("snn_conv1x1_mask_fwd", x_mask.data_ptr(), x_mask.shape[-1], wc.data_ptr(), y.data_ptr(), cl_stride(y),
                      T * B, H, W, Cin, Ct, _stream())
        elif x_th is not None:
            _hip.call("snn_conv1x1_spikes_fwd", x.data_ptr(), cl_stride(x), x_th, wc.data_ptr(), y.data_ptr(), cl_stride(y),
                      T * B, H, W, Cin, Ct, _stream())
        else:
            _hip.call("snn_conv2d_fwd", x.data_ptr(), cl_stride(x), wc.data_ptr(), None, y.data_ptr(), cl_stride(y), T * B,
                      H, W, Cin, H, W, Ct, 1, 1, 1, 0, None, 0, None, 0, None, fwd_prec, _stream())
        ctx.prec = bwd_prec
        ctx.x_th = x_th
        ctx.x_mask = x_mask
        ctx.fwd_prec = fwd_prec
        ctx.save_for_backward(x, w1m, *w2ms)
        ctx.wct = wct
        ctx.geom = (T, B, Cin, H, W, Ct, 1, 1, H, W, 1, 0)
        ctx.widths, ctx.c1 = widths, C1
        ctx.slot1, ctx.slots2 = slot1, slots2
        ctx.acc = acc
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w1m, *w2ms = ctx.saved_tensors
        T, B, Cin, H, W, Ct = ctx.geom[:6]
        C1, widths = ctx.c1, ctx.widths
        composed = w1m is not None
        gy = _raw_to_cl(gy)
        ldg, ldx = cl_stride(gy), cl_stride(x)
        dx = dw1 = None
        dw2s = [None] * len(widths)
        want_dw = any(ctx.needs_input_grad[9:]) or (composed and ctx.needs_input_grad[1])
        fuse = None
        if ctx.needs_input_grad[0]:
            if want_dw and _FusedBwd1x1.eligible(ctx.geom, ctx.prec, gy, x) and (ctx.x_th is None or ctx.x_mask is not None):
                # dx and the slabs of G from one pass over gy (when the query covers the call); x as the weight gradient
                # below would read it: the spike bit mask of the LIF layer in front, or stored activations
                splitk = _hip.query("snn_conv2d_wgrad_splitk", T * B, H, W, Cin, H, W, Ct, 1, 1, 1, 0, ctx.prec)
                if ctx.x_mask is None:
                    fuse = _FusedBwd1x1(gy, ldg, ctx.wct, x, ldx, False, ctx.geom, ctx.prec, splitk)
                else:
                    fuse = _FusedBwd1x1(gy, ldg, ctx.wct, ctx.x_mask, ctx.x_mask.shape[-1], True, ctx.geom, ctx.prec, splitk)
            dx = _dgrad_accumulate(ctx.acc, gy, ldg, ctx.wct, x, ctx.geom, _stream(), ctx.prec, fuse=fuse)
        if want_dw:
            slot1, slots2 = ctx.slot1, ctx.slots2
            slotted = all(s_ is not None for s_ in slots2) and (slot1 is not None or not composed)
            splitk = _hip.query("snn_conv2d_wgrad_splitk", T * B, H, W, Cin, H, W, Ct, 1, 1, 1, 0, ctx.prec)
            xw, ldxw, x_th = _spikes_wgrad_operand(x, ldx, ctx.x_th, gy, ldg)
            x_mask = ctx.x_mask
            fws = fuse.ws if fuse is not None else None   # the slabs are there already: only their reduction is left
            with _WgradLaunch(x.device, slotted, 0 if fws is not None else splitk, Ct, Cin, hold=(x, xw, gy, x_mask, fws),
                              with_g=True) as (stream, ws, G):
                if fws is not None:
                    _hip.call("snn_conv2d_wgrad_reduce", fws.data_ptr(), G.data_ptr(), Ct * Cin, splitk, 0, stream)
                elif x_mask is not None and _hip.query("snn_conv1x1_mask_supported", T * B, H, W, Cin, Ct, x_mask.data_ptr(),
                                                       x_mask.shape[-1], None, None, 0, gy.data_ptr(), ldg, G.data_ptr(),
                                                       ctx.fwd_prec, ctx.prec):
                    # the spikes of the LIF layer in front as its bit mask; otherwise its potentials, which are always there
                    _hip.call("snn_conv1x1_mask_wgrad", x_mask.data_ptr(), x_mask.shape[-1], gy.data_ptr(), ldg, G.data_ptr(),
                              T * B, H, W, Cin, Ct, 0, ws.data_ptr(), splitk, stream)
                elif x_th is not None:   # x holds the potentials of the LIF layer in front: thresholded on load
                    _hip.call("snn_conv1x1_spikes_wgrad", xw.data_ptr(), ldxw, x_th, gy.data_ptr(), ldg, G.data_ptr(),
                              T * B, H, W, Cin, Ct, 0, ws.data_ptr(), splitk, stream)
                else:
                    _hip.call("snn_conv2d_wgrad", xw.data_ptr(), ldxw, gy.data_ptr(), ldg, G.data_ptr(), T * B, H, W,
                              Cin, H, W, Ct, 1, 1, 1, 0, 0, ws.data_ptr(), splitk, ctx.prec, stream)
                # straight into the flat gradient slots when there are any
                g1 = None
                if composed:
                    g1 = slot1.buf.view(C1, Cin) if slotted else torch.empty((C1, Cin), device=x.device, dtype=_F32)
                    acc1 = slot1.claim() if slotted else 0
                row = 0
                for b, (w2m, c) in enumerate(zip(w2ms, widths)):
                    Gb = G[row:row + c]
                    row += c
                    if slotted:
                        g2, acc2 = slots2[b].buf.view(c, C1), slots2[b].claim()
                    else:
                        g2, acc2 = torch.empty((c, C1), device=x.device, dtype=_F32), 0
                    if composed:
                        _small_gemm(Gb, False, w1m, True, g2, acc2)      # dw2_b = G_b w1^T
                        _small_gemm(w2m, True, Gb, False, g1, acc1)      # dw1 (+)= w2_b^T G_b
                        acc1 = 1
                    elif acc2:
                        g2.add_(Gb)
                    else:
                        g2.copy_(Gb)
                    if not slotted:
                        dw2s[b] = g2.view(c, C1, 1, 1)
                if composed and not slotted:
                    dw1 = g1.view(C1, Cin, 1, 1)
        return (dx, dw1, None, None, None, None, None, None, None, *dw2s)


def sibling_conv1x1(x: torch.Tensor, w1: Optional[torch.Tensor], w2s: Sequence[torch.Tensor], dest: Optional[Dest] = None,
                    forward_precision: Optional[str] = None, backward_precision: Optional[str] = None) -> torch.Tensor:
    """``cat([conv1x1(h, w) for w in w2s], channels)`` with ``h = conv1x1(x, w1)`` (``h = x`` when ``w1`` is None), as one
    convolution; ``x`` is a sequence ``[T,B,C,H,W]``."""
    return _SiblingConv1x1.apply(x, w1, dest, _acc_of(x), _prec_codes(forward_precision, backward_precision),
                                 _slot_of(w1), tuple(_slot_of(w) for w in w2s), getattr(x, "_snn_spike_threshold", None),
                                 getattr(x, "_snn_spike_mask", None), *w2s)


def composed_conv1x1(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, dest: Optional[Dest] = None,
                     forward_precision: Optional[str] = None, backward_precision: Optional[str] = None) -> torch.Tensor:
    """``conv1x1(conv1x1(x, w1), w2)`` without the intermediate tensor: the sibling convolution with one branch (the
    C2f entry in front of ONE branch-opening convolution: a block without sibling fusion, or a single timestep
    ``[B,C,H,W]``).  ``x`` never holds saved potentials here (``generator.BlockGen`` plans none in front)."""
    if x.dtype == _BF16 and (w1.shape[1] % 32 or w2.shape[0] % 32):   # (see conv2d)
        y = to_bfloat16(composed_conv1x1(to_float32(x), w1, w2, None, forward_precision, backward_precision))
        return place(y, dest) if dest is not None else y
    seq, single = as_sequence(x)
    y = _SiblingConv1x1.apply(seq, w1, dest, _acc_of(seq), _prec_codes(forward_precision, backward_precision),
                              _slot_of(w1), (_slot_of(w2),), None, None, w2)
    return y[0] if single else y


class BnPartial(NamedTuple):
    """Statistics partials a forward convolution left for the BatchNorm behind it (``snn_conv2d_fwd`` ``bn_partial``)."""
    partial: torch.Tensor
    chunks: int
    rows_per_chunk: int
    data_ptr: int          # the tensor they describe
    dims: Tuple[int, int, int]   # (T, pixels per timestep, channels)


def conv2d(x: torch.Tensor, weight: torch.Tensor, stride: int = 1, padding: int = 0, dest: Optional[Dest] = None,
           forward_precision: Optional[str] = None, backward_precision: Optional[str] = None,
           bn_stats: bool = False) -> torch.Tensor:
    """``forward_precision`` / ``backward_precision``: this call's arithmetic (None = the session default).

    ``bn_stats``: the result feeds a train-mode BatchNorm - the kernel also emits that layer's statistics partials
    (attached to the result as ``_snn_bn_partial``; ``affine_neuron`` picks them up and skips its own pass over y).
    """
    if x.dtype == _BF16 and (weight.shape[1] % 32 or weight.shape[0] % 32):
        # bf16 storage: the kernels want whole 32-channel k-steps (forward: Cin, data gradient: Cout); other layers - a
        # prediction head applied to every timestep - take the fp32 kernels between two conversions
        y = to_bfloat16(conv2d(to_float32(x), weight, stride, padding, None, forward_precision, backward_precision, False))
        return place(y, dest) if dest is not None else y
    x_th = getattr(x, "_snn_spike_threshold", None)   # x holds a LIF layer's saved potentials (affine_neuron spikes_ok)
    seq, single = as_sequence(x)
    bn_out = [] if bn_stats else None
    y = _Conv2d.apply(seq, weight, int(stride), int(padding), _slot_of(weight), dest, _acc_of(seq),
                      _prec_codes(forward_precision, backward_precision), bn_out, x_th)
    y = y[0] if single else y
    if bn_out:
        y._snn_bn_partial = bn_out[0]
    if bn_stats and not single and _slot_of(weight) is not None and _wgrad_bn_ok(seq, weight, int(stride), int(padding)):
        y._snn_defer_apply = True   # (bn_stats: the BatchNorm behind is y's only consumer)
    return y


# ------------------------------------------------------------------------------------------- depthwise conv
def depthwise_covers(N: int, H: int, W: int, C: int, K: int, stride: int, pad: int) -> bool:
    """What the depthwise kernels run: ``snn_dwconv_supported`` (host only; the library is the one place that says it)."""
    return bool(_hip.query("snn_dwconv_supported", N, H, W, C, K, stride, pad))


@functools.lru_cache(maxsize=None)
def depthwise_sets() -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """``(kernel sizes, strides)`` the depthwise kernels take - ASKED of ``snn_dwconv_supported`` over the candidates a
    description could name, not restated here (what ``layer_gen.Conv.get`` names in its refusals)."""
    sizes = tuple(k for k in range(1, 16) if depthwise_covers(1, 16, 16, 1, k, 1, k // 2))
    strides = tuple(s for s in range(1, 9) if sizes and depthwise_covers(1, 16, 16, 1, sizes[0], s, sizes[0] // 2))
    return sizes, strides


def _tap_major(weight: torch.Tensor, st: int) -> torch.Tensor:
    """The kernels' weight image ``[K*K][C]`` of a depthwise ``(C,1,K,K)`` weight: FlatTrainer's ``_snn_wt`` (the batched
    transpose of an ``I = 1`` weight IS the tap-major image, refreshed once per step), else built here by one small launch
    - as ``_frag_image`` is for the halo kernels.  The weight's memory is read as ``[C][K*K]`` whatever torch says about its
    layout (for ``I = 1`` OIHW and OHWI coincide)."""
    wt = _kept_view(weight, "_snn_wt")
    if wt is not None:
        return wt
    C, _, KH, KW = weight.shape
    w = weight.detach()
    if not (w.is_contiguous() or is_channels_last(w)):
        w = w.contiguous()
    wt = torch.empty((KH * KW, C), device=w.device, dtype=_F32)
    _hip.call("snn_weight_transpose", w.data_ptr(), wt.data_ptr(), C, KH, KW, 1, st)
    return wt


class _DepthwiseConv2d(Function):
    """nn.Conv2d(C, C, K, stride, padding=K//2, groups=C, bias=False) over all T*B frames (csrc/conv_depthwise.hip).  Returns
    dx to autograd: like ``_Pool`` it takes no part in the ``GradAccumulator`` protocol."""

    @staticmethod
    def forward(ctx, x, weight, stride: int, pad: int, slot=None, dest=None, x_th=None):
        _require_device(x, "depthwise_conv2d input")
        _require_device(weight, "depthwise_conv2d weight")
        T, B, C, H, W = _dims5(x)
        Cw, I, KH, KW = weight.shape
        if Cw != C or I != 1 or KH != KW:
            raise RuntimeError(f"depthwise_conv2d: input has {C} channels, the weight is {tuple(weight.shape)}; expected "
                               f"({C}, 1, K, K)")
        if not depthwise_covers(T * B, H, W, C, KH, stride, pad):
            raise RuntimeError(f"depthwise_conv2d: kernel_size {KH}, stride {stride}, padding {pad} on {T * B} frames of "
                               f"{H}x{W}x{C} is not covered (snn_dwconv_supported: kernel_size in {{3, 5}}, stride in "
                               "{1, 2}, padding = kernel_size // 2)")
        Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        x = _raw_to_cl(x)
        if x_th is not None:   # saved potentials of a LIF layer that wrote no spikes: written out here (dx is d loss / d spikes)
            x = _spikes_dense(x, x_th)
        st = _stream()
        wt = _tap_major(weight, st)
        if _ACTIVITY is not None:
            _ACTIVITY.count_conv((weight,), x, None, None, 1, KH, KW, stride)   # fan-out Cout / groups = 1
        y = _out_tensor(dest, T, B, C, Ho, Wo, x)
        _hip.call("snn_dwconv_fwd", x.data_ptr(), cl_stride(x), wt.data_ptr(), y.data_ptr(), cl_stride(y), T * B, H, W, C, KH,
                  stride, pad, st)
        ctx.save_for_backward(x)
        ctx.weight = weight
        ctx.wt = wt if wt is not getattr(weight, "_snn_wt", None) else None   # (a per-call image is kept; a trainer's is re-read)
        ctx.geom = (T, B, C, H, W, KH, Ho, Wo, stride, pad)
        ctx.slot = slot
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        T, B, C, H, W, K, Ho, Wo, stride, pad = ctx.geom
        gy = _raw_to_cl(gy)
        ldg, ldx = cl_stride(gy), cl_stride(x)
        st = _stream()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            wt = ctx.wt if ctx.wt is not None else _tap_major(ctx.weight, st)
            dx = _new_cl((T, B), C, H, W, x)
            _hip.call("snn_dwconv_dgrad", gy.data_ptr(), ldg, wt.data_ptr(), dx.data_ptr(), cl_stride(dx), T * B, H, W, C, K,
                      stride, pad, st)
        if ctx.needs_input_grad[1]:
            slot = ctx.slot
            n_ws = _hip.query("snn_dwconv_wgrad_workspace_size", T * B, H, W, C, K, stride, pad, 0) // 4
            # (the workspace comes from _WgradLaunch as fp32 words on the launch's stream; the kernels use it as fp64 rows)
            with _WgradLaunch(x.device, slot is not None, 1, 1, n_ws, hold=(x, gy)) as (stream, ws, _):
                if slot is not None:
                    dst, accumulate = slot.buf, slot.claim()
                else:
                    dst, accumulate = torch.empty((C, K * K), device=x.device, dtype=_F32), 0
                _hip.call("snn_dwconv_wgrad", x.data_ptr(), ldx, gy.data_ptr(), ldg, dst.data_ptr(), T * B, H, W, C, K,
                          stride, pad, accumulate, ws.data_ptr(), 0, stream)
            if slot is None:
                dw = dst.view(C, 1, K, K)
        return dx, dw, None, None, None, None, None


def depthwise_conv2d(x: torch.Tensor, weight: torch.Tensor, stride: int = 1, padding: int = 0,
                     dest: Optional[Dest] = None) -> torch.Tensor:
    """Depthwise convolution ``conv2d(x, weight, groups=C)`` with ``weight`` ``(C,1,K,K)``, ``[B,C,H,W]`` or ``[T,B,C,H,W]``.
    Exact fp32 products whatever the session's arithmetic modes say.  ``dest``: write the result into a channel slice of a
    concat buffer.  The weight's ``GradSlot`` (FlatTrainer) receives the weight gradient from the side stream, as a dense
    convolution's does.  bf16 storage: the fp32 kernels between two conversions (``conv2d``'s pattern for head layers).
    Saved potentials (``_snn_spike_threshold``) are written out as spikes first: these kernels do not threshold on load."""
    x_th = getattr(x, "_snn_spike_threshold", None)
    if x.dtype == _BF16:
        xf = to_float32(x)
        if x_th is not None:
            xf._snn_spike_threshold = x_th   # (bf16 -> fp32 is exact: the same comparison)
        y = to_bfloat16(depthwise_conv2d(xf, weight, stride, padding, None))
        return place(y, dest) if dest is not None else y
    seq, single = as_sequence(x)
    y = _DepthwiseConv2d.apply(seq, weight, int(stride), int(padding), _slot_of(weight), dest, x_th)
    return y[0] if single else y


# ------------------------------------------------------------------------------------------- norm + neuron
class NeuronState(NamedTuple):
    """State of a LIF / LI layer: membrane potential and synaptic current, each ``[B,C,h,w]``.

    Same field names / order as norse's ``LIFFeedForwardState`` and ``LIState``.
    """
    v: torch.Tensor
    i: torch.Tensor


class SynapseState(NamedTuple):
    """State of a ``Synapse`` layer: mediator concentration (synapse.py:18-22)."""
    p: torch.Tensor


_SAVES_STEP = (_hip.NEURON_LIF, _hip.NEURON_SLI, _hip.NEURON_SYNAPSE)
SCAN_SEGMENT_T = 32   # backward scans of longer sequences run in segments of this many steps (None: one launch)
# BatchNorm statistics from the producing convolution's epilogue when it offers them (SNN_NO_CONV_BN_STATS: tuning
# aid, the separate snn_bn_stats pass everywhere)
USE_CONV_BN_STATS = not os.environ.get("SNN_NO_CONV_BN_STATS")
# pre-split weight images kept by FlatTrainer (SNN_NO_PRESPLIT_WEIGHTS: tuning aid, conversion in every block)
USE_PRESPLIT_WEIGHTS = not os.environ.get("SNN_NO_PRESPLIT_WEIGHTS")
# ... for the data gradient too: measured neutral (its bf16 split is three bit operations per pair, the forward's fp16 split a
# scale, two conversions and a subtraction), so off by default: one launch and one weight-sized buffer less per step
USE_PRESPLIT_DGRAD = bool(os.environ.get("SNN_PRESPLIT_DGRAD"))
SCAN_FLAGS = 0   # flags of snn_affine_neuron_bwd; tests set _hip.SCAN_WIDE_ADDRESSING to cover the 64-bit-pointer scan
# the reverse LIF scan of a train-mode Norm -> LIF layer does not read the convolution output y: the BatchNorm statistic it
# needs y for is formed from the neuron input rebuilt from the saved potentials (snn_affine_neuron_bwd
# SNN_SCAN_SUMS_FROM_STATE; SNN_NO_SUMS_FROM_STATE: tuning / bisecting aid)
USE_SUMS_FROM_STATE = not os.environ.get("SNN_NO_SUMS_FROM_STATE")

# Opt-in memory lever: a LIF layer whose per-step saved state ([T,B,H,W,C] fp32) is at least this many bytes stores
# checkpoints of (v, i) every snn_lif_ckpt_interval() steps instead and recomputes in the backward scan
# (snn_lif_fwd_ckpt / snn_lif_bwd_ckpt: bit-identical results, half the saved-state memory, speed-neutral).
# None (default) = never, 0 = every LIF layer.  Measured on 1280x720 B=4 T=32: 125 -> 113 GiB live.  Off by default
# because the half-size buffers fragment torch's caching allocator once the live set approaches the whole HBM
# (B=8: 222 GiB live but 287 GiB reserved and a thrashing allocator, against 250 GiB live at full speed without).
LIF_CHECKPOINT_BYTES: Optional[int] = None


def _bn_coefficients(y, ldy, dims, gamma, bias, use_running, eps, momentum, running_mean, running_var, sync_group,
                     bn_hint, st):
    """BatchNorm statistics of ``y`` per (t, c) - the running ones, this process's, or the group's (SyncBatchNorm) - and
    the affine they make with gamma / bias: ``(mean, invstd, alpha, beta)``, each ``[T, C]``."""
    T, M, C = dims
    dev = y.device
    mean, invstd, alpha, beta = (torch.empty((T, C), device=dev, dtype=_F32) for _ in range(4))
    g_ptr = _ptr(gamma.detach()) if gamma is not None else None
    b_ptr = _ptr(bias.detach()) if bias is not None else None
    if use_running:
        if running_mean is None or running_var is None:
            raise RuntimeError("BatchNorm in eval mode needs running statistics")
        _hip.call("snn_bn_stats_finalize", None, 0, 0, T, M, C, g_ptr, b_ptr, eps, momentum,
                  running_mean.data_ptr(), running_var.data_ptr(), 1, mean.data_ptr(), invstd.data_ptr(),
                  alpha.data_ptr(), beta.data_ptr(), st)
        return mean, invstd, alpha, beta
    if bn_hint is not None and bn_hint.data_ptr == y.data_ptr() and bn_hint.dims == (T, M, C) and USE_CONV_BN_STATS:
        # the producing convolution summed y and y^2 on the way out (snn_conv2d_fwd bn_partial)
        partial, chunks, rpc = bn_hint.partial, bn_hint.chunks, bn_hint.rows_per_chunk
    else:
        n_part = _hip.query("snn_bn_stats_partial_size", T, M, C)
        partial = torch.empty((n_part,), device=dev, dtype=torch.float64)
        chunks = rpc = 0
        _hip.call("snn_bn_stats_bf16" if y.dtype == _BF16 else "snn_bn_stats", y.data_ptr(), ldy, T, M, C,
                  partial.data_ptr(), st)
    if sync_group is None:
        _hip.call("snn_bn_stats_finalize", partial.data_ptr(), chunks, rpc, T, M, C, g_ptr, b_ptr, eps, momentum,
                  _ptr(running_mean), _ptr(running_var), 0, mean.data_ptr(), invstd.data_ptr(),
                  alpha.data_ptr(), beta.data_ptr(), st)
    else:
        # SyncBatchNorm (config.yaml:76): ONE all-reduce of [T, C, 2] sums per layer for all timesteps
        import torch.distributed as dist
        world = dist.get_world_size(sync_group[0])
        sums = torch.empty((T, C, 2), device=dev, dtype=torch.float64)
        _hip.call("snn_bn_stats_reduce", partial.data_ptr(), chunks, rpc, T, M, C, sums.data_ptr(), st)
        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=sync_group[0])
        scratch = torch.empty((T * C,), device=dev, dtype=torch.float64)
        _hip.call("snn_bn_stats_from_sums", sums.data_ptr(), T, M * world, C, g_ptr, b_ptr, eps, momentum,
                  _ptr(running_mean), _ptr(running_var), mean.data_ptr(), invstd.data_ptr(),
                  alpha.data_ptr(), beta.data_ptr(), scratch.data_ptr(), st)
    return mean, invstd, alpha, beta


def _sync_bn_bwd_coefficients(sync_group, sums, from_state, gx, y, ldy, dims, gamma, bn_bias, mean, invstd, coef, dg_ptr,
                              db_ptr, acc_flag, st):
    """SyncBatchNorm backward: dy needs the GLOBAL sums (one all-reduce of [T, C, 2]); the parameter gradients use the
    rank-local sums - the data-parallel all-reduce averages them afterwards."""
    import torch.distributed as dist
    T, M, C = dims
    world = dist.get_world_size(sync_group[0])
    raw_local = torch.empty((T, C, 2), device=y.device, dtype=torch.float64)
    if from_state:
        _hip.call("snn_bn_bwd_reduce_from_state", sums.data_ptr(), T, M, C, _ptr(gamma), _ptr(bn_bias),
                  mean.data_ptr(), invstd.data_ptr(), gx.data_ptr(), y.data_ptr(), ldy, raw_local.data_ptr(), st)
    else:
        _hip.call("snn_bn_bwd_reduce", sums.data_ptr(), T, M, C, raw_local.data_ptr(), st)
    raw = raw_local.clone()
    dist.all_reduce(raw, op=dist.ReduceOp.SUM, group=sync_group[0])
    param_sums = torch.empty((T, C, 2), device=y.device, dtype=torch.float64)
    _hip.call("snn_bn_bwd_coef", raw.data_ptr(), raw_local.data_ptr(), param_sums.data_ptr(), T, M * world,
              C, _ptr(gamma), mean.data_ptr(), invstd.data_ptr(), coef[0].data_ptr(), coef[1].data_ptr(),
              coef[2].data_ptr(), dg_ptr, db_ptr, acc_flag, st)


def _ptr_at(t: Optional[torch.Tensor], offset: int) -> Optional[int]:
    return None if t is None else t.data_ptr() + offset


class _NeuronCfg(NamedTuple):
    """The non-tensor arguments of ``_AffineNeuron`` (built by ``affine_neuron``)."""
    neuron: int
    has_bn: bool
    training: bool
    eps: float
    momentum: float
    running_mean: Optional[torch.Tensor]
    running_var: Optional[torch.Tensor]
    params: NeuronParams
    g_slot: Optional[GradSlot]
    b_slot: Optional[GradSlot]
    dest: Optional[Dest]
    sync_group: object
    bn_hint: object
    last_only: bool
    defer_apply: bool
    spikes_out: Optional[list]
    tau_slots: Tuple[Optional[GradSlot], Optional[GradSlot]]
    spike_mask: bool = False   # the consumer is sibling_conv1x1, which can read the spikes as a bit mask


def _bf16_scan_covers(neuron: int, channels: int) -> bool:
    """The Norm -> neuron scans have a bf16-storage form for these neurons on a multiple of 4 channels."""
    return neuron in (_hip.NEURON_NONE, _hip.NEURON_LIF, _hip.NEURON_LI, _hip.NEURON_LI_TANH) and channels % 4 == 0


def _takes_checkpointed_pair(neuron: int, nbytes: int, params: NeuronParams, last_only: bool, sb: bool, tau: bool) -> bool:
    """A layer of ``nbytes`` of saved potentials runs on snn_lif_fwd_ckpt / snn_lif_bwd_ckpt: those write / read all T
    outputs (not the last-step-only read-out), fp32, and have the default gradient rule and the struct's scalar time
    constants only - any other layer takes the plain scan."""
    return (neuron == _hip.NEURON_LIF and LIF_CHECKPOINT_BYTES is not None and not last_only and not sb
            and nbytes >= LIF_CHECKPOINT_BYTES and default_gradient_rule(params) and not tau)


def _grad_pair(slots, needed, n: int, dev):
    """Where the two gradients of a parameter pair (gamma / bias, w_mem / w_syn) go: ``(ptr_a, ptr_b, accumulate, fresh_a,
    fresh_b)``.  Straight into the flat gradient buffer when every needed member has a ``GradSlot`` - both slots are then
    claimed and share one accumulate flag, the first present slot's ``written`` before the claim; into fresh [n] tensors
    (handed back to autograd, flag 0) otherwise."""
    if not any(needed):
        return None, None, 0, None, None
    if all(s_ is not None or not need for s_, need in zip(slots, needed)):
        acc = 1 if (slots[0] or slots[1]).written else 0
        for s_ in slots:
            if s_ is not None:
                s_.claim()
        pa, pb = (s_.buf.data_ptr() if (s_ is not None and need) else None for s_, need in zip(slots, needed))
        return pa, pb, acc, None, None
    fa, fb = (torch.empty((n,), device=dev, dtype=_F32) if need else None for need in needed)
    return _ptr(fa), _ptr(fb), 0, fa, fb


class _AffineNeuron(Function):
    """[BatchNorm2d (per-timestep batch statistics)] -> [LIF | LI | LI+Tanh | nothing], fused.

    inputs : y[T,B,C,H,W], gamma[C]|None, bias[C]|None, v0|None, i0|None, addend[T,B,C,H,W]|None, + non-tensor config
    outputs: out[T,B,C,H,W], vT[B,C,H,W], iT[B,C,H,W]  (vT/iT are dummies when neuron == NONE)

    ``addend`` is a residual shortcut folded into the output store: out = neuron(norm(y)) + addend
    (generator.py:145-146 does stack + sum as a separate pass); its gradient is g_out itself.
    """

    @staticmethod
    def forward(ctx, y, gamma, bias, v0, i0, addend, cfg, w_mem=None, w_syn=None):
        neuron, has_bn, params, dest, sync_group, last_only = (cfg.neuron, cfg.has_bn, cfg.params, cfg.dest, cfg.sync_group,
                                                               cfg.last_only)
        _require_device(y, "norm/neuron input", bf16_ok=True)
        sb = y.dtype == _BF16   # bf16 storage: y, out, the saved per-step state and the gradients; (v, i) and all sums fp32
        # w_mem / w_syn ([1] or [C] each): the raw time-constant parameters of a learnable / per-channel LIF layer
        tau = w_mem is not None
        if tau:
            _tau_refusal(neuron, sb)   # (LIF_CHECKPOINT_BYTES leaves such a layer on the plain scan, see `ckpt`)
            if last_only and (ctx.needs_input_grad[7] or ctx.needs_input_grad[8]):
                raise RuntimeError("last_only is not built for a LIF layer whose time constants are learned (tau=...)")
        if sb and not _bf16_scan_covers(neuron, y.shape[-3]):
            raise RuntimeError("bf16 storage: Norm + none / LIF / LI / LI+Tanh with a multiple of 4 channels only")
        if not default_gradient_rule(params):
            name = next((k for k, v in SURROGATES.items() if v == params.surrogate), params.surrogate)
            rule = f"surrogate={name!r}, detach_reset={bool(params.reset_detached)}"
            if neuron != _hip.NEURON_LIF:
                raise RuntimeError(f"a non-default gradient rule ({rule}) belongs to LIF layers")
            if sb:
                raise RuntimeError(f"bf16 storage has the default LIF gradient rule only, not ({rule}): keep this layer's "
                                   "tensors fp32 or its rule at surrogate='super', detach_reset=False")
        sb_flag = _hip.SCAN_BF16_STORAGE if sb else 0
        ctx.set_materialize_grads(False)  # unused final-state outputs must arrive as None, not as zero tensors
        y = _raw_to_cl(y)
        ldy = cl_stride(y)
        T, B, C, H, W = _dims5(y)
        if (C % 4 == 0 and (y.data_ptr() % (8 if sb else 16) or ldy % 4)
                and (has_bn or neuron in (_hip.NEURON_SLI, _hip.NEURON_SYNAPSE))):
            # a channel slice at an offset or pixel stride that is not a multiple of 4 (a split_channels part): the
            # statistics pass and the reverse scan read y in 4-channel vectors - they get a dense copy
            y = _raw_dense_cl(y)
            ldy = C
        M = B * H * W
        st = _stream()
        dev = y.device
        use_running = has_bn and not cfg.training
        if tau:
            learn = ctx.needs_input_grad[7] or ctx.needs_input_grad[8]
            nig = ctx.needs_input_grad
            sums_wanted = has_bn and ((nig[0] and not use_running) or (gamma is not None and nig[1]) or nig[2])
            if learn and sums_wanted and sync_group is None and SCAN_SEGMENT_T and T > SCAN_SEGMENT_T:
                # the backward pass of such a sequence runs in segments, and the two sums of a segment behind the first
                # one would need the potential in front of it (a look-back that is not built)
                raise RuntimeError(f"learnable time constants (tau=...): a Norm -> LIF sequence of {T} steps is longer than one "
                                   f"scan segment (SCAN_SEGMENT_T = {SCAN_SEGMENT_T}) and the segment look-back of the two "
                                   "gradient sums is not built")
        mean = invstd = alpha = beta = None
        if has_bn:
            mean, invstd, alpha, beta = _bn_coefficients(y, ldy, (T, M, C), gamma, bias, use_running, cfg.eps, cfg.momentum,
                                                         cfg.running_mean, cfg.running_var, sync_group, cfg.bn_hint, st)
        need_grad = any(ctx.needs_input_grad[:5]) or (tau and (ctx.needs_input_grad[7] or ctx.needs_input_grad[8]))
        c_mem = c_syn = None
        if tau:
            c_mem, c_syn = lif_time_constants(w_mem, w_syn, C)
        ckpt_pair = _takes_checkpointed_pair(neuron, T * M * C * 4, params, last_only, sb, tau)
        # spikes_out (a list the caller reads afterwards): the consumer can form the spikes from the saved potentials
        # (snn_conv1x1_spikes_*), so when those are saved anyway no output tensor is written at all
        spikes_out = cfg.spikes_out
        no_out = (spikes_out is not None and USE_SPIKES_FROM_VDEC and neuron == _hip.NEURON_LIF and need_grad and has_bn
                  and addend is None and dest is None and not last_only and not sb and C % 4 == 0 and ldy % 4 == 0
                  and params.v_th >= 0.0 and not ckpt_pair)
        if last_only:
            # only the last timestep's output is kept (snn_affine_neuron_fwd SNN_SCAN_LAST_STEP_ONLY): out is [B,C,H,W]
            if (neuron not in (_hip.NEURON_LIF, _hip.NEURON_LI, _hip.NEURON_LI_TANH) or addend is not None
                    or dest is not None):
                raise RuntimeError("last_only is for LIF / LI / LI+Tanh without shortcut or concat destination")
            out = _new_cl((B,), C, H, W, y)
        elif no_out:
            out = None
        else:
            out = _out_tensor(dest, T, B, C, H, W, y)
        has_state = neuron != _hip.NEURON_NONE
        vT = _new_cl((B,), C, H, W, y, _F32) if has_state else torch.empty(0, device=dev)
        iT = _new_cl((B,), C, H, W, y, _F32) if has_state else torch.empty(0, device=dev)
        vdec = None
        ckpt = False
        if neuron in _SAVES_STEP and need_grad:
            ckpt = ckpt_pair
            if ckpt:
                k = _hip.query("snn_lif_ckpt_interval")
                vdec = torch.empty(((T + k - 1) // k, 2, B, H, W, C), device=dev, dtype=_F32)
            else:
                vdec = torch.empty((T, B, H, W, C), device=dev, dtype=y.dtype)
        count_only = False
        if _ACTIVITY is not None and neuron == _hip.NEURON_LIF and (addend is not None or last_only):
            # the recorder counts this layer's spikes, and the scan leaves none to count: `out` is z + shortcut, or the last
            # step alone.  Potentials are saved anyway when a backward pass follows; otherwise the scan writes them for this
            # one pass, into a buffer that is free again once the count has been enqueued.
            if ckpt:
                raise RuntimeError("activity.record: a LIF layer on the checkpointed scan (LIF_CHECKPOINT_BYTES) with a fused "
                                   "shortcut keeps neither spikes nor potentials to count")
            if vdec is None:
                vdec = torch.empty((T, B, H, W, C), device=dev, dtype=y.dtype)
                count_only = True
        if v0 is not None:
            v0 = _expand_state(v0, (B, C, H, W), dev)
        if i0 is not None:
            i0 = _expand_state(i0, (B, C, H, W), dev)
        ctx.addend_acc = None
        ad_ptr, ld_ad = None, 0
        if addend is not None:
            if neuron == _hip.NEURON_LI_TANH:
                raise RuntimeError("a fused shortcut is not supported after LI+Tanh (its backward reads the output)")
            ctx.addend_acc = _acc_of(addend)
            addend = _raw_to_cl(addend)
            if tuple(addend.shape) != (T, B, C, H, W):
                raise RuntimeError("Residual merge: branch outputs differ in shape")
            if addend.dtype != y.dtype:
                raise RuntimeError("Residual merge: shortcut and branch are stored in different types (fp32 / bf16)")
            ad_ptr, ld_ad = addend.data_ptr(), cl_stride(addend)
        mask = None
        if ckpt:
            _hip.call("snn_lif_fwd_ckpt", y.data_ptr(), ldy, _ptr(alpha), _ptr(beta), _ptr(v0), _ptr(i0),
                      out.data_ptr(), cl_stride(out), ad_ptr, ld_ad, _ptr(vT), _ptr(iT), vdec.data_ptr(), T, M, C,
                      params, st)
        else:
            head = (neuron, y.data_ptr(), ldy, _ptr(alpha), _ptr(beta), _ptr(v0), _ptr(i0),
                    _ptr(out), C if out is None else cl_stride(out), ad_ptr, ld_ad, _ptr(vT) if has_state else None,
                    _ptr(iT) if has_state else None, _ptr(vdec), T, M, C, params)
            fwd_flags = ((_hip.SCAN_LAST_STEP_ONLY if last_only else 0) | sb_flag
                         | (_hip.SCAN_SPIKES_FROM_VDEC if no_out else 0))
            # ... and the spikes as one bit per neuron next to the potentials (snn_conv1x1_mask_*: 32 channels per word)
            if no_out and cfg.spike_mask and USE_SPIKE_MASK and not tau and C % 32 == 0 and T * M * C * 4 >= SPIKE_MASK_MIN_BYTES and all(
                    t is None or t.data_ptr() % 16 == 0 for t in (y, alpha, beta, v0, i0, vT, iT, vdec)):
                mask = torch.empty((T, B, H, W, C // 32), device=dev, dtype=torch.int32)
            if tau:
                _hip.call("snn_lif_tau_fwd", *head, c_mem.data_ptr(), c_syn.data_ptr(), fwd_flags, st)
            elif mask is not None:
                _hip.call("snn_affine_neuron_fwd_mask", *head, fwd_flags | _hip.SCAN_SPIKE_MASK, st, mask.data_ptr(), C // 32)
            else:
                _hip.call("snn_affine_neuron_fwd", *head, fwd_flags, st)
            if no_out:
                # what travels to the consumer is an alias of the saved potentials, marked with the threshold that turns
                # them into this layer's output
                out = _alias(vdec, vdec.storage_offset(), T, B, C, H, W, C)
                spikes_out.append(float(params.v_th))
                if mask is not None:
                    spikes_out.append(mask)
        if _ACTIVITY is not None and neuron == _hip.NEURON_LIF:
            # what this forward produced, cheapest first: the bit mask; the spike tensor, unless a shortcut is folded into
            # its store or only the last step was written; the saved potentials with v_th.  In bf16 storage the last are the
            # STORED (rounded) potentials - the spikes the reverse scan sees, which the scan's own comparison on the
            # unrounded value can differ from for a potential within one bf16 step of the threshold.
            spikes = None if (no_out or addend is not None or last_only) else out
            _ACTIVITY.count_lif(params, mask, spikes, None if ckpt else vdec, float(params.v_th), (T, B, C, H, W))
            if count_only:
                vdec = None
        ctx.ckpt = ckpt
        ctx.sb = sb
        ctx.defer_apply = cfg.defer_apply
        ctx.last_only = last_only
        # (a copy: the cell's struct is mutable - set_lif_gradient between this forward and its backward must not change
        # the rule of a graph already recorded, nor ask the checkpointed pair for a rule it refuses)
        ctx.cfg = (neuron, has_bn, use_running, NeuronParams.from_buffer_copy(params), (T, B, C, H, W))
        ctx.slots = (cfg.g_slot, cfg.b_slot)
        ctx.tau = tau
        ctx.tau_slots = cfg.tau_slots
        ctx.tau_n = w_mem.numel() if tau else 0
        ctx.sync_group = sync_group if (has_bn and not use_running) else None
        ctx.has_v0 = v0 is not None
        ctx.has_i0 = i0 is not None
        if neuron == _hip.NEURON_LI_TANH and need_grad and not is_channels_last(out):
            raise RuntimeError("LI+Tanh output placed in a concat slice is not supported for training")
        state = vdec if neuron in _SAVES_STEP else (out if neuron == _hip.NEURON_LI_TANH else None)
        # (a learnable layer's backward needs the initial potential for the two sums' terms of step 0)
        ctx.save_for_backward(y, gamma, mean, invstd, alpha, beta, state, bias if has_bn else None, c_mem, c_syn,
                              v0 if (tau and need_grad) else None)
        if not has_state:
            ctx.mark_non_differentiable(vT, iT)
        # with a neuron, vT / iT stay differentiable (time-outer BPTT through the carried state)
        if sb and last_only:
            out = _raw_convert(out, _F32)   # the read-out of the last step (a few frames) leaves the bf16 domain here
        return out, vT, iT

    @staticmethod
    def backward(ctx, g_out, g_vT, g_iT):
        y, gamma, mean, invstd, alpha, beta, state, bn_bias, c_mem, c_syn, v0_saved = ctx.saved_tensors
        neuron, has_bn, use_running, params, (T, B, C, H, W) = ctx.cfg
        M = B * H * W
        st = _stream()
        dev = y.device
        has_state = neuron != _hip.NEURON_NONE
        g_addend = None
        if g_out is not None and ctx.needs_input_grad[5]:
            g_addend = g_out
            if ctx.addend_acc is not None:  # lets the shortcut's producer-side dgrad add it in its epilogue
                ctx.addend_acc[0].deposit(ctx.addend_acc[1], g_out)
        sb = ctx.sb
        if g_out is None:
            g_out = torch.zeros((B, H, W, C) if ctx.last_only else (T, B, H, W, C), device=dev, dtype=y.dtype)
            g_out = _cl_view(g_out)
        if g_out.dtype != y.dtype:
            g_out = _raw_convert(g_out, y.dtype)   # (bf16 storage: the fp32 gradient of the last-step read-out)
        g_out = _raw_to_cl(g_out)
        es = y.element_size()
        scan_flags = SCAN_FLAGS | (_hip.SCAN_LAST_STEP_ONLY if ctx.last_only else 0) | (_hip.SCAN_BF16_STORAGE if sb else 0)
        ldg, ldy = cl_stride(g_out), cl_stride(y)
        if not has_state:
            g_vT = g_iT = None
        if g_vT is not None:
            g_vT = _raw_dense_cl(g_vT)
        if g_iT is not None:
            g_iT = _raw_dense_cl(g_iT)
        need_y = ctx.needs_input_grad[0]
        need_gamma = has_bn and gamma is not None and ctx.needs_input_grad[1]
        need_bias = has_bn and ctx.needs_input_grad[2]
        need_sums = has_bn and ((need_y and not use_running) or need_gamma or need_bias)
        gx = torch.empty((T, B, H, W, C), device=dev, dtype=y.dtype)
        g_v0 = _new_cl((B,), C, H, W, y, _F32) if (has_state and ctx.has_v0 and ctx.needs_input_grad[3]) else None
        g_i0 = _new_cl((B,), C, H, W, y, _F32) if (has_state and ctx.has_i0 and ctx.needs_input_grad[4]) else None
        # eval-mode BN has no batch coupling: dy = alpha * gx, applied while gx is written
        apply_scale = 1 if (has_bn and use_running) else 0
        dy = None
        coef = torch.empty((3, T, C), device=dev, dtype=_F32) if need_sums else None
        dg_ptr, db_ptr, acc_flag, dgamma, dbias = _grad_pair(ctx.slots, (need_gamma, need_bias), C, dev)
        # Long sequences in SEGMENTS of SCAN_SEGMENT_T steps, last segment first.  The scan kernel keeps its per-(t, c)
        # BatchNorm sums for ALL T steps in LDS (one slab per wave); at T = 128 that leaves room for 16 channels per
        # block only, i.e. 64-byte runs per pixel - measured 2.6 TB/s against 4.6 at T = 32.  The recurrence crosses a
        # segment boundary through (g_v, g_i), which the kernel already takes and returns: same values bit for bit.
        segmented = (need_sums and has_state and not ctx.ckpt and ctx.sync_group is None and SCAN_SEGMENT_T
                     and T > SCAN_SEGMENT_T)
        # per-channel / learnable time constants: snn_lif_tau_bwd (the y-reading scan), and the partial sums of the two
        # gradients when a raw parameter wants one - into its GradSlot when both have one, as dgamma / dbias
        tau = ctx.tau
        need_wm, need_ws = (ctx.needs_input_grad[7], ctx.needs_input_grad[8]) if tau else (False, False)
        if (need_wm or need_ws) and segmented:   # (the forward refuses what would get here)
            raise RuntimeError("learnable time constants (tau=...): the segment look-back of the two gradient sums is "
                               "not built")
        dwm_ptr, dws_ptr, tau_acc, d_wmem, d_wsyn = _grad_pair(ctx.tau_slots, (need_wm, need_ws), ctx.tau_n, dev)
        # (segments: every segment must be covered; a segment behind the first one finds the neuron state it starts from
        # in the two saved potentials in front of it - SNN_SCAN_STATE_LOOKBACK)
        sums_from_state = bool(
            USE_SUMS_FROM_STATE and need_sums and not ctx.ckpt and not apply_scale and neuron == _hip.NEURON_LIF
            and not tau    # (its query answers for the struct's scalars only)
            and not ctx.has_v0 and not ctx.has_i0 and g_v0 is None and g_i0 is None
            and not (segmented and T % SCAN_SEGMENT_T == 1)    # (a second segment starting at step 1 has one step to look back on)
            and all(_hip.query("snn_affine_neuron_bwd_sums_from_state", neuron, ts_, M, C, ldg, params, scan_flags)
                    for ts_ in ({SCAN_SEGMENT_T, T % SCAN_SEGMENT_T or SCAN_SEGMENT_T} if segmented else {T})))
        # One loop over the segments, last first; an unsegmented scan is the single segment [0, T).
        seg_T = SCAN_SEGMENT_T if segmented else T
        fr_g, fr_y, fr_c = M * ldg * es, M * ldy * es, M * C * es    # bytes per timestep of g_out / y / dense tensors
        gv_in, gi_in = g_vT, g_iT
        g_none = None   # last_only: the output gradient of every segment but the last one is zero
        sums = None
        for t1 in range(T, 0, -seg_T):
            t0 = max(0, t1 - seg_T)
            ts, tc = t1 - t0, t0 * C * 4
            # what a segment hands down: the caller's g_v0 / g_i0 from segment [0, ...), a carry buffer in between
            gv_out, gi_out = g_v0, g_i0
            if segmented and (t0 > 0 or g_v0 is None):
                gv_out = torch.empty((B, H, W, C), device=dev, dtype=_F32)
            if segmented and (t0 > 0 or g_i0 is None):
                gi_out = torch.empty((B, H, W, C), device=dev, dtype=_F32)
            if need_sums:
                n_sums = _hip.query("snn_affine_neuron_bwd_sums_size", ts, M, C)
                sums = torch.empty((n_sums,), device=dev, dtype=torch.float64)
            if not ctx.last_only:
                g_seg = g_out.data_ptr() + t0 * fr_g
            elif t1 == T:
                g_seg = g_out.data_ptr()          # [B,H,W,C] of the last step = the last step of this segment
            else:
                if g_none is None:
                    g_none = torch.zeros_like(g_out)
                g_seg = g_none.data_ptr()
            st_off = 0 if (ctx.last_only and neuron == _hip.NEURON_LI_TANH) else t0 * fr_c   # saved output: last step only
            y_seg, gx_seg = y.data_ptr() + t0 * fr_y, gx.data_ptr() + t0 * fr_c
            # (sums from the state: y is not read - the statistic comes from the neuron input rebuilt from the saved
            # potentials; a segment gets the pointer all the same)
            scan = (g_seg, ldg, _ptr_at(state, st_off), y_seg if (segmented or not sums_from_state) else None, ldy,
                    _ptr(gv_in), _ptr(gi_in), _ptr_at(alpha, tc), _ptr_at(beta, tc), apply_scale, gx_seg, _ptr(gv_out),
                    _ptr(gi_out), _ptr(sums), ts, M, C, params)
            if ctx.ckpt:
                _hip.call("snn_lif_bwd_ckpt", *scan, st)
            elif tau:
                tau_part = None
                if need_wm or need_ws:
                    n_tau = _hip.query("snn_lif_tau_bwd_partial_size", ts, M, C, int(need_sums))
                    tau_part = torch.empty((n_tau,), device=dev, dtype=torch.float64)
                _hip.call("snn_lif_tau_bwd", neuron, *scan, _ptr_at(c_mem, 0), _ptr_at(c_syn, 0),
                          _ptr(v0_saved) if t0 == 0 else None, _ptr(tau_part), scan_flags, st)
                if tau_part is not None:
                    _hip.call("snn_lif_tau_finalize", tau_part.data_ptr(), ts, M, C, int(need_sums), c_mem.data_ptr(),
                              c_syn.data_ptr(), int(ctx.tau_n == 1), dwm_ptr, dws_ptr, tau_acc, st)
            else:
                seg_flags = scan_flags
                if sums_from_state:
                    seg_flags |= _hip.SCAN_SUMS_FROM_STATE | (_hip.SCAN_STATE_LOOKBACK if t0 > 0 else 0)
                _hip.call("snn_affine_neuron_bwd", neuron, *scan, seg_flags, st)
            if need_sums and ctx.sync_group is None:
                # coefficients of this segment's steps; the parameter gradients add up over the segments
                tail = (coef[0].data_ptr() + tc, coef[1].data_ptr() + tc, coef[2].data_ptr() + tc, dg_ptr, db_ptr,
                        acc_flag if t1 == T else 1, st)
                if sums_from_state:
                    _hip.call("snn_bn_bwd_finalize_from_state", sums.data_ptr(), ts, M, C, _ptr(gamma), _ptr(bn_bias),
                              mean.data_ptr() + tc, invstd.data_ptr() + tc, gx_seg, y_seg, ldy, *tail)
                else:
                    _hip.call("snn_bn_bwd_finalize", sums.data_ptr(), ts, M, C, _ptr(gamma), mean.data_ptr() + tc,
                              invstd.data_ptr() + tc, *tail)
            gv_in, gi_in = gv_out, gi_out
        if need_sums:
            if ctx.sync_group is not None:   # (never segmented: `sums` covers all T steps)
                _sync_bn_bwd_coefficients(ctx.sync_group, sums, sums_from_state, gx, y, ldy, (T, M, C), gamma, bn_bias, mean,
                                          invstd, coef, dg_ptr, db_ptr, acc_flag, st)
            if need_y and not use_running and ctx.defer_apply and ctx.sync_group is None:
                # the producing convolution forms dy itself while it reads gx (see PendingBnApply)
                _PENDING_APPLY[gx.data_ptr()] = PendingBnApply(gx, y, coef, (T, B, C, H, W))
            elif need_y and not use_running:
                # in place: dy overwrites gx
                _hip.call("snn_bn_bwd_apply_bf16" if sb else "snn_bn_bwd_apply", gx.data_ptr(), y.data_ptr(), ldy,
                          coef[0].data_ptr(), coef[1].data_ptr(), coef[2].data_ptr(), gx.data_ptr(), C, T, M, C, 0, st)
        if need_y:
            dy = _cl_view(gx)
        return dy, dgamma, dbias, g_v0, g_i0, g_addend, None, d_wmem, d_wsyn


class BwdPlan(NamedTuple):
    """The reverse-scan instance snn_affine_neuron_bwd launches (include/snn_hip.h, snn_affine_neuron_bwd_plan)."""
    vec: int
    mode: int
    buf: int
    np: int
    cvb: int
    gy: int
    gx: int
    rpb: int
    partial_row: int
    lds_bytes: int


def affine_neuron_bwd_plan(neuron: int, T: int, M: int, C: int, ldg: int, ldy: int, with_sums: bool, flags: int = 0,
                           params: Optional[NeuronParams] = None) -> BwdPlan:
    out = (ctypes.c_int64 * 10)()
    _hip.call("snn_affine_neuron_bwd_plan", neuron, T, M, C, ldg, ldy, int(bool(with_sums)), params or neuron_params(),
              flags, ctypes.addressof(out))
    return BwdPlan(*out)


class TauBwdPlan(NamedTuple):
    """The reverse-scan instance snn_lif_tau_bwd launches (include/snn_hip.h, snn_lif_tau_bwd_plan)."""
    scan: BwdPlan
    ordered: int      # the two sums of the time constants' gradients are combined in fixed order (0: LDS float atomics)
    lds_bytes: int


def lif_tau_bwd_plan(T: int, M: int, C: int, ldg: int, ldy: int, with_sums: bool, with_tau_sums: bool = True, flags: int = 0,
                     params: Optional[NeuronParams] = None, neuron: int = _hip.NEURON_LIF) -> TauBwdPlan:
    out = (ctypes.c_int64 * 12)()
    _hip.call("snn_lif_tau_bwd_plan", neuron, T, M, C, ldg, ldy, int(bool(with_sums)), int(bool(with_tau_sums)),
              params or neuron_params(), flags, ctypes.addressof(out))
    return TauBwdPlan(BwdPlan(*out[:10]), int(out[10]), int(out[11]))


def _expand_state(s: torch.Tensor, shape, dev) -> torch.Tensor:
    """State tensors may be 0-dim (LICell's initial v) or NCHW; the kernel wants dense [B,H,W,C]."""
    s = s.detach()
    if s.dim() == 0 or tuple(s.shape) != tuple(shape):
        s = s.to(device=dev, dtype=_F32).expand(shape)
    return _raw_dense_cl(s)


def affine_neuron(y: torch.Tensor, neuron: int, state: Optional[NeuronState] = None, bn=None,
                  params: Optional[NeuronParams] = None, dest: Optional[Dest] = None,
                  addend: Optional[torch.Tensor] = None, last_only: bool = False, spikes_ok: bool = False,
                  tau: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, spike_mask_ok: bool = False):
    """Fused ``[Norm] -> [neuron] [+ addend]`` over a sequence or a single step.

    ``tau=(w_mem, w_syn)`` (LIF, fp32 tensors): per-channel time constants ``c_mem = sigmoid(w_mem)``, ``1 + c_syn =
    sigmoid(w_syn)`` in place of ``params.c_mem`` / ``.c_syn``; each holds one value (the whole layer) or one per channel.
    One that requires a gradient receives it - into its ``GradSlot`` when it has one, through autograd otherwise.

    ``spikes_ok`` (LIF on a sequence; the caller guarantees that the ONLY consumer is ``sibling_conv1x1``): the result may be
    the layer's saved potentials instead of its spikes, marked ``_snn_spike_threshold`` - no spike tensor is written.
    ``spike_mask_ok`` (with ``spikes_ok``; the consumer IS ``sibling_conv1x1``): the scan may also write the spikes as one bit
    per neuron (``_snn_spike_mask``, ``[T,B,H,W,C/32]`` int32), which that convolution reads instead of the potentials.

    ``bn`` is an ``nn.BatchNorm2d``-like module (weight, bias, running stats, eps, momentum, training)
    or None; ``addend`` (same shape as the output) is a residual shortcut added in the output store.
    ``last_only`` (LI / LI+Tanh on a sequence): return the output of the LAST timestep only, ``[B,C,H,W]`` - the other
    T-1 outputs are never written and the backward pass reads no output gradient for them.
    Returns ``(out, NeuronState | None)``.
    """
    if y.dtype == _BF16 and not _bf16_scan_covers(neuron, y.shape[-3]):
        # no bf16-storage form of this scan (SLI / Synapse, channel counts that are not a multiple of 4): see _through_fp32
        if tau is not None:
            _tau_refusal(neuron, True)
        out, new_state = affine_neuron(to_float32(y), neuron, state, bn, params, None,
                                       None if addend is None else to_float32(addend), last_only, False)
        out = out if (last_only and y.dim() == 5) else to_bfloat16(out)
        return (place(out, dest) if dest is not None else out), new_state
    bn_hint = getattr(y, "_snn_bn_partial", None)
    defer_apply = bool(getattr(y, "_snn_defer_apply", False))
    seq, single = as_sequence(y)
    if addend is not None:
        acc = _acc_of(addend)
        addend, _ = as_sequence(addend)
        if acc is not None:
            addend._snn_acc = acc
    params = params or neuron_params()
    has_bn = bn is not None
    gamma = bias = rm = rv = None
    training, eps, momentum = False, 1e-5, 0.1
    if has_bn:
        gamma, bias = bn.weight, bn.bias
        training = bn.training or (bn.running_mean is None and bn.running_var is None)
        rm, rv = bn.running_mean, bn.running_var
        eps = bn.eps
        if bn.momentum is None:
            raise RuntimeError("cumulative-average BatchNorm (momentum=None) is not supported")
        momentum = bn.momentum
        if training and seq.shape[1] * seq.shape[3] * seq.shape[4] <= 1:
            # torch.nn.functional.batch_norm's own check (the reference's per-timestep BatchNorm2d raises it): one value
            # per channel has no variance to normalise with
            raise ValueError("Expected more than 1 value per channel when training, got input size "
                             f"{torch.Size((seq.shape[1], seq.shape[2], seq.shape[3], seq.shape[4]))}")
        if training and bn.num_batches_tracked is not None:
            if _NBT_BATCH is not None:
                _NBT_BATCH.append((bn.num_batches_tracked, int(seq.shape[0])))  # one fused update per forward
            else:
                bn.num_batches_tracked.add_(seq.shape[0])
    v0 = i0 = None
    if state is not None:
        if neuron == _hip.NEURON_SYNAPSE:
            (v0,) = state
        else:
            v0, i0 = state
    sync_group = getattr(bn, "_snn_sync_group", None) if has_bn else None
    spikes_out = [] if (spikes_ok and not single and dest is None and addend is None) else None
    w_mem, w_syn = tau if tau is not None else (None, None)
    cfg = _NeuronCfg(neuron=neuron, has_bn=has_bn, training=training, eps=float(eps), momentum=float(momentum),
                     running_mean=rm, running_var=rv, params=params, g_slot=_slot_of(gamma), b_slot=_slot_of(bias), dest=dest,
                     sync_group=sync_group, bn_hint=bn_hint, last_only=bool(last_only) and not single,
                     defer_apply=defer_apply, spikes_out=spikes_out, tau_slots=(_slot_of(w_mem), _slot_of(w_syn)),
                     spike_mask=bool(spike_mask_ok))
    out, vT, iT = _AffineNeuron.apply(seq, gamma, bias, v0, i0, addend, cfg, w_mem, w_syn)
    if spikes_out:
        out._snn_spike_threshold = spikes_out[0]   # `out` holds v_dec: its consumer thresholds on load
        if len(spikes_out) > 1:
            out._snn_spike_mask = spikes_out[1]    # ... or reads the same spikes as one bit per neuron
    if neuron == _hip.NEURON_NONE:
        new_state = None
    elif neuron == _hip.NEURON_SYNAPSE:
        new_state = SynapseState(vT)
    else:
        new_state = NeuronState(vT, iT)
        if params.v_leak != 0.0:
            vT._snn_rest = float(params.v_leak)   # what state=None starts this potential from (reset_state_ reads it)
    if last_only and not single:
        return out, new_state
    return (out[0] if single else out), new_state


# ------------------------------------------------------------------------------------------- carried state
def _sample_blocks(t: torch.Tensor) -> torch.Tensor:
    """``t[B, ...]`` with every sample's elements in one dense block (as it is, or as a dense copy)."""
    if t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)):
        return t
    return _raw_dense_cl(t) if t.dim() >= 4 else t.contiguous()


def detach_state(state_tree):
    """The state tree with every tensor detached (same nesting and tuple types; the ``_snn_rest`` tags are kept): what is
    carried from one training step to the next, so that no autograd graph is."""
    if state_tree is None:
        return None
    if isinstance(state_tree, torch.Tensor):
        t = state_tree.detach()
        if hasattr(state_tree, "_snn_rest"):
            t._snn_rest = state_tree._snn_rest
        return t
    if isinstance(state_tree, tuple) and hasattr(state_tree, "_fields"):   # NeuronState, SynapseState, norse's tuples
        return type(state_tree)(*(detach_state(t) for t in state_tree))
    if isinstance(state_tree, (list, tuple)):
        return type(state_tree)(detach_state(t) for t in state_tree)
    raise ValueError(f"detach_state: {type(state_tree).__name__} is no part of a state tree")


_RESET_TABLES = []   # pinned staging tables of reset_state_, used in turn: {"pinned", "np", "done": event behind its last copy}
_RESET_RING = 4


def _reset_table(n: int) -> dict:
    """The next of the pinned int64 tables (at least ``n`` entries), free to be written: the copy that last read it has
    completed - it was enqueued ``_RESET_RING`` calls ago, so the wait on its event does not block in practice."""
    slot = {"pinned": None, "np": None, "done": None} if len(_RESET_TABLES) < _RESET_RING else _RESET_TABLES.pop(0)
    _RESET_TABLES.append(slot)
    if slot["done"] is None:
        slot["done"] = torch.cuda.Event()
    elif not slot["done"].query():
        slot["done"].synchronize()
    if slot["pinned"] is None or slot["pinned"].numel() < n:
        slot["pinned"] = torch.empty(max(n, 512), dtype=torch.int64, pin_memory=True)
        slot["np"] = slot["pinned"].numpy()
    return slot


def reset_state_(state_tree, first: torch.Tensor):
    """Put the samples ``b`` with ``first[b] != 0`` back to rest in every tensor of a detector state tree, in place, with
    ONE launch (``snn_state_reset``) and without the host learning which samples those are.

    ``state_tree`` is what ``SODa._forward_impl`` returns: nested lists of ``NeuronState(v, i)``, ``SynapseState(p)``,
    ``(h, c)`` pairs and None.  ``first`` is an integer device tensor ``[B]``.  Every leaf is detached; a 0-dim or
    broadcast leaf of a ``NeuronState`` (norse's initial ``v``) is expanded to its partner's shape by ``_expand_state``'s
    rule.  Rest is what ``state=None`` starts from: zero, except the potential of a neuron whose ``v_leak`` is not zero
    (the scans tag that tensor ``_snn_rest``).  Returns the tree (same nesting; leaves are the detached tensors - a leaf
    that was not dense per sample is replaced by a dense copy)."""
    if not (isinstance(first, torch.Tensor) and first.dim() == 1 and first.is_cuda
            and first.dtype in (torch.int32, torch.int64, torch.bool, torch.uint8)):
        raise ValueError("reset_state_: first must be an integer device tensor [B]")
    B = int(first.numel())
    first = first.to(torch.int32).contiguous()
    rows = []

    def leaf(t: torch.Tensor, like: Optional[torch.Tensor] = None) -> torch.Tensor:
        rest = float(getattr(t, "_snn_rest", 0.0))
        t = t.detach()
        if like is not None and tuple(t.shape) != tuple(like.shape):
            t = _expand_state(t, like.shape, like.device).clone()   # (own memory: an expanded view has none to reset)
        if t.dtype != _F32 or t.dim() < 1 or t.shape[0] != B or t.numel() == 0:
            raise ValueError(f"reset_state_: a state leaf must be float32 [B = {B}, ...], got {t.dtype} {tuple(t.shape)}")
        _require_device(t, "reset_state_ leaf")
        t = _sample_blocks(t)
        if rest != 0.0:
            t._snn_rest = rest
        rows.extend((t.data_ptr(), t.numel() // B, struct.unpack("<I", struct.pack("<f", rest))[0] if rest != 0.0 else 0))
        return t

    def walk(node):
        if node is None:
            return None
        if isinstance(node, torch.Tensor):
            return leaf(node)
        if isinstance(node, NeuronState):
            full = node.i if node.v.dim() < node.i.dim() else node.v
            return NeuronState(leaf(node.v, full), leaf(node.i, full))
        if isinstance(node, SynapseState):
            return SynapseState(leaf(node.p))
        if isinstance(node, (list, tuple)):
            kids = [walk(k) for k in node]
            return kids if isinstance(node, list) else tuple(kids)
        raise ValueError(f"reset_state_: {type(node).__name__} is no part of a state tree")

    tree = walk(state_tree)
    n = len(rows) // 3
    if n > 65535:
        raise ValueError(f"reset_state_: {n} state tensors are more than one launch takes (65535)")
    if n:
        # the addresses change with every step: the table is written into pinned memory and copied on the compute stream
        # in front of the launch
        slot = _reset_table(len(rows))
        slot["np"][:len(rows)] = rows
        table = torch.empty(len(rows), dtype=torch.int64, device=first.device)
        table.copy_(slot["pinned"][:len(rows)], non_blocking=True)
        slot["done"].record(torch.cuda.current_stream(first.device))
        _hip.call("snn_state_reset", table.data_ptr(), n, B, first.data_ptr(), _stream())
    return tree


# ------------------------------------------------------------------------------------------- merges
class _Concat(Function):
    """Dense merge: torch.cat(out, dim=1) per timestep (generator.py:157-158), copying form."""

    @staticmethod
    def forward(ctx, dest, *xs):
        xs = [_raw_to_cl(x) for x in xs]
        T, B, _, H, W = _dims5(xs[0])
        widths = [x.shape[2] for x in xs]
        Ct = sum(widths)
        out = _out_tensor(dest, T, B, Ct, H, W, xs[0])
        off = 0
        for x, c in zip(xs, widths):
            _require_device(x, "concat input", bf16_ok=True)
            if x.shape[0] != T or x.shape[1] != B or x.shape[3] != H or x.shape[4] != W:
                raise RuntimeError("Dense merge: branch outputs differ in shape")
            _copy_cl(x, out.narrow(2, off, c))
            off += c
        ctx.widths = widths
        return out

    @staticmethod
    def backward(ctx, g):
        g = _raw_to_cl(g)
        grads, off = [None], 0
        for k, c in enumerate(ctx.widths):
            grads.append(g.narrow(2, off, c) if ctx.needs_input_grad[k + 1] else None)  # channel-slice views
            off += c
        return tuple(grads)


class _ConcatAssemble(Function):
    """Dense merge without a copy: every branch output already IS its channel slice of ``whole``
    (``ConcatPromise``); this node only ties the autograd graph together.  Backward hands each branch
    the matching channel-slice VIEW of the incoming gradient (the kernels take a pixel stride)."""

    @staticmethod
    def forward(ctx, whole, *xs):
        ctx.widths = [x.shape[2] for x in xs]
        ctx.accs = [_acc_of(x) for x in xs]
        T, B, C, H, W = _dims5(whole)
        return _alias(whole, whole.storage_offset(), T, B, C, H, W, cl_stride(whole))

    @staticmethod
    def backward(ctx, g):
        g = _raw_to_cl(g)
        grads, off = [None], 0
        for k, c in enumerate(ctx.widths):
            gk = g.narrow(2, off, c) if ctx.needs_input_grad[k + 1] else None
            if gk is not None and ctx.accs[k] is not None:
                # a channel range of g that only branch k is handed: whoever accumulates that branch's gradient may
                # write the total over it
                ctx.accs[k][0].deposit(ctx.accs[k][1], gk, exclusive=True)
            grads.append(gk)
            off += c
        return tuple(grads)


class _Sum(Function):
    """Residual merge: torch.stack(out).sum(0) (generator.py:145-146)."""

    @staticmethod
    def forward(ctx, dest, *xs):
        xs = [_raw_to_cl(x) for x in xs]
        for x in xs:
            _require_device(x, "residual input", bf16_ok=True)
            if x.shape != xs[0].shape:
                raise RuntimeError("Residual merge: branch outputs differ in shape")
        T, B, C, H, W = _dims5(xs[0])
        ctx.accs = [_acc_of(x) for x in xs]
        out = _out_tensor(dest, T, B, C, H, W, xs[0])
        _add_cl(xs[0], xs[1], out)
        for x in xs[2:]:
            _add_cl(out, x, out)
        return out

    @staticmethod
    def backward(ctx, g):
        for acc, need in zip(ctx.accs, ctx.needs_input_grad[1:]):
            if acc is not None and need:
                acc[0].deposit(acc[1], g)
        return (None,) + tuple(g if need else None for need in ctx.needs_input_grad[1:])


class _Fanout(Function):
    """One tensor consumed by ``n`` branches of a block (generator.py:181-187 hands every branch the same X).

    Forward returns ``n`` aliases (no copy); backward adds the branch gradients with the strided add
    kernel, so gradient accumulation stays on this library's kernels and accepts channel-sliced grads."""

    @staticmethod
    def forward(ctx, x, n: int):
        ctx.acc = GradAccumulator()
        ctx.outer = ctx.acc.outer = _acc_of(x)
        ctx.acc.grad_in_slot = bool(getattr(x, "_snn_grad_in_slot", False))
        outs = []
        for k in range(n):
            t = torch.empty(0, device=x.device, dtype=x.dtype)
            t.set_(x.untyped_storage(), x.storage_offset(), x.size(), x.stride())
            t._snn_acc = (ctx.acc, k)
            outs.append(t)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        acc = ctx.acc
        total = None
        if acc.result is not None:
            # a data-gradient convolution already holds (its own + the fused deposits'); add only what is missing
            total = acc.result
            for k, g in enumerate(gs):
                if g is None:
                    continue
                if k in acc.fused:
                    if not _same_tensor(g, acc.fused[k]):
                        raise RuntimeError("fanout: a branch input received a gradient the fused accumulation did "
                                           "not expect (the alias was consumed more than once)")
                    continue
                gk = _raw_to_cl(g)
                if total.dim() == 4:
                    _add_cl(total.unsqueeze(0), gk.unsqueeze(0), total.unsqueeze(0))
                else:
                    _add_cl(total, gk, total)
        else:
            live = [g for g in gs if g is not None]
            if not live:
                return None, None
            if len(live) == 1:
                total = live[0]
            else:
                single = live[0].dim() == 4
                seqs = [_raw_to_cl(g.unsqueeze(0) if single else g) for g in live]
                T, B, C, H, W = _dims5(seqs[0])
                out = _new_cl((T, B), C, H, W, seqs[0])
                _add_cl(seqs[0], seqs[1], out)
                for g in seqs[2:]:
                    _add_cl(out, g, out)
                total = out[0] if single else out
        acc.deposits.clear()
        acc.fused.clear()
        acc.exclusive.clear()
        acc.result = None
        if ctx.outer is not None:
            ctx.outer[0].deposit(ctx.outer[1], total)
        return total, None


def fanout(x: torch.Tensor, n: int):
    """``n`` aliases of ``x`` for the ``n`` branches of a block; their gradients are summed by a HIP kernel."""
    if n == 1 or not x.requires_grad:
        return [x] * n
    return list(_Fanout.apply(x, n))


class _Place(Function):
    """Copy a tensor into a destination slice (fallback when a producer could not write there itself)."""

    @staticmethod
    def forward(ctx, x, dest):
        ctx.acc = _acc_of(x)
        x = _raw_to_cl(x)
        T, B, C, H, W = _dims5(x)
        out = dest.tensor(T, B, C, H, W, x)
        _copy_cl(x, out)
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.acc is not None:
            ctx.acc[0].deposit(ctx.acc[1], g)
        return g, None


def place(x: torch.Tensor, dest: Dest) -> torch.Tensor:
    """``x`` as the channel slice ``dest`` of a concat buffer (no-op when it already lives there)."""
    if dest.holds(x):
        return x
    return _Place.apply(x, dest)


def concat_channels(xs: List[torch.Tensor], dest: Optional[Dest] = None) -> torch.Tensor:
    if len(xs) == 1 and dest is None:
        return xs[0]
    seqs = [as_sequence(x) for x in xs]
    out = _Concat.apply(dest, *[s for s, _ in seqs])
    return out[0] if seqs[0][1] else out


def assemble_channels(promise: ConcatPromise, xs: List[torch.Tensor]) -> torch.Tensor:
    """Zero-copy Dense merge of branch outputs that were produced inside ``promise``'s buffer."""
    return _ConcatAssemble.apply(promise.buf, *xs)


def sum_tensors(xs: List[torch.Tensor], dest: Optional[Dest] = None) -> torch.Tensor:
    if len(xs) == 1:
        return xs[0] if dest is None else place(as_sequence(xs[0])[0], dest)
    seqs = [as_sequence(x) for x in xs]
    out = _Sum.apply(dest, *[s for s, _ in seqs])
    return out[0] if seqs[0][1] else out


class _GradReady(Function):
    """Identity whose backward first calls ``fn()``: marks the point of the backward pass at which every gradient
    produced downstream of ``x`` (in forward order) is complete or enqueued - ``FlatTrainer.early_all_reduce``."""

    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        acc = _acc_of(x)
        out = torch.empty(0, device=x.device, dtype=x.dtype)
        out.set_(x.untyped_storage(), x.storage_offset(), x.size(), x.stride())
        if acc is not None:
            out._snn_acc = acc
        return out

    @staticmethod
    def backward(ctx, g):
        ctx.fn()
        return g, None


def grad_ready_hook(x: torch.Tensor, fn) -> torch.Tensor:
    """``x`` unchanged; during the backward pass ``fn()`` runs when the gradient of ``x`` arrives."""
    if fn is None or not x.requires_grad:
        return x
    return _GradReady.apply(x, fn)


# ------------------------------------------------------------------------------------------- spatial pyramid pooling
def spp(x: torch.Tensor, kernel_size: int = 5, levels: int = 3, dest: Optional[Dest] = None) -> torch.Tensor:
    """Spatial pyramid pooling (the SPPF stage of YOLOv5 / v8 without its convolutions): ``[B,C,H,W]`` or ``[T,B,C,H,W]`` ->
    ``[..., (levels + 1) * C, H, W]`` = ``x`` beside ``levels`` chained ``MaxPool2d(kernel_size, 1, kernel_size // 2)`` of
    it.  ``dest``: write the result into a channel slice of a concat buffer.  bf16 storage: the fp32 kernels between two
    conversions, as every pool."""
    if x.dtype == _BF16:
        y = to_bfloat16(spp(to_float32(x), kernel_size, levels, None))
        return place(y, dest) if dest is not None and y.dim() == 5 else y
    seq, single = as_sequence(x)
    y = _SPP.apply(seq, int(kernel_size), int(levels), dest)
    return y[0] if single else y


# ------------------------------------------------------------------------------------------- ConvLSTM
class _LstmCell(Function):
    """Pointwise LSTM update on the gate pre-activations (conv_lstm.py:66-76); one timestep ``[B,*,H,W]``."""

    @staticmethod
    def forward(ctx, gates, c_prev):
        _require_device(gates, "lstm gates")
        gates = _raw_dense_cl(gates)
        B, C4, H, W = gates.shape
        C = C4 // 4
        if c_prev is not None:
            c_prev = _raw_dense_cl(c_prev)
        h = _new_cl((B,), C, H, W, gates)
        c = _new_cl((B,), C, H, W, gates)
        _hip.call("snn_lstm_cell_fwd", gates.data_ptr(), _ptr(c_prev), h.data_ptr(), c.data_ptr(), B * H * W, C,
                  _stream())
        ctx.save_for_backward(gates, c_prev, c)
        return h, c

    @staticmethod
    def backward(ctx, gh, gc):
        gates, c_prev, c = ctx.saved_tensors
        B, C4, H, W = gates.shape
        C = C4 // 4
        gh = _raw_dense_cl(gh) if gh is not None else None
        gc = _raw_dense_cl(gc) if gc is not None else None
        g_gates = _new_cl((B,), C4, H, W, gates)
        g_cp = _new_cl((B,), C, H, W, gates) if (c_prev is not None and ctx.needs_input_grad[1]) else None
        _hip.call("snn_lstm_cell_bwd", gates.data_ptr(), _ptr(c_prev), c.data_ptr(), _ptr(gh), _ptr(gc),
                  g_gates.data_ptr(), _ptr(g_cp), B * H * W, C, _stream())
        return g_gates, g_cp


def lstm_cell(gates: torch.Tensor, c_prev: Optional[torch.Tensor]):
    if gates.dtype == _BF16:   # (see _through_fp32) the cell state c stays fp32 across the steps
        h, c = _LstmCell.apply(to_float32(gates), None if c_prev is None else to_float32(c_prev))
        return to_bfloat16(h), c
    return _LstmCell.apply(gates, c_prev)


# One launch per pass over the whole sequence instead of a time-outer loop of concat + gate conv + cell (bisecting aid).
USE_LSTM_SCAN = not os.environ.get("SNN_NO_LSTM_SCAN")


def conv_lstm_scan_covers(in_channels: int, hidden_channels: int, ldx: int) -> bool:
    """``snn_convlstm_seq_supported``: the function the launchers check (host-only, no device needed)."""
    return bool(_hip.query("snn_convlstm_seq_supported", int(in_channels), int(hidden_channels), int(ldx)))


def conv_lstm_scan_tile(in_channels: int, hidden_channels: int, pixels: int) -> int:
    """Pixels per workgroup of the two scan kernels for ``pixels = B*H*W`` (``snn_convlstm_seq_tile``; 0: not covered)."""
    return int(_hip.query("snn_convlstm_seq_tile", int(in_channels), int(hidden_channels), int(pixels)))


class _ConvLstmSeq(Function):
    """ConvLSTM with 1x1 gates over ``[T,B,Cin,H,W]`` (conv_lstm.py:51-78): one scan kernel forward, one backward, and ONE
    weight-gradient launch over the ``T*B`` frames of ``[x ; h_prev]`` with ``dy = dgates``."""

    @staticmethod
    def forward(ctx, x, weight, h0, c0, slot, bwd_prec):
        _require_device(x, "conv_lstm_sequence input")
        _require_device(weight, "conv_lstm_sequence weight")
        x = _raw_to_cl(x)
        T, B, Cin, H, W = _dims5(x)
        C4, K, KH, KW = weight.shape
        Ch = C4 // 4
        if (KH, KW) != (1, 1) or K != Cin + Ch or C4 != 4 * Ch:
            raise RuntimeError(f"conv_lstm_sequence: weight {tuple(weight.shape)} is no 1x1 gate weight for {Cin} inputs")
        w = weight.detach()
        w_ohwi = w if is_channels_last(w) else _raw_dense_cl(w)
        if h0 is not None:
            h0, c0 = _raw_dense_cl(h0), _raw_dense_cl(c0)
        M = B * H * W
        hs = _new_cl((T, B), Ch, H, W, x)
        cT = _new_cl((B,), Ch, H, W, x)
        save_g = save_c = None
        if any(ctx.needs_input_grad[:4]):   # (eval / no_grad / predict_sequence: nothing but hs and c_T is written)
            save_g = torch.empty((T, M, C4), device=x.device, dtype=_F32)
            save_c = torch.empty((T, M, Ch), device=x.device, dtype=_F32)
        _hip.call("snn_convlstm_seq_fwd", x.data_ptr(), cl_stride(x), w_ohwi.data_ptr(), _ptr(h0), _ptr(c0), hs.data_ptr(),
                  cT.data_ptr(), _ptr(save_g), _ptr(save_c), T, M, Cin, Ch, _stream())
        hT = hs[T - 1].clone()
        ctx.save_for_backward(x, w_ohwi, h0, c0, hs, save_g, save_c)
        ctx.geom = (T, B, Cin, Ch, H, W)
        ctx.slot, ctx.prec = slot, bwd_prec
        ctx.set_materialize_grads(False)
        return hs, hT, cT

    @staticmethod
    def backward(ctx, ghs, ghT, gcT):
        x, w_ohwi, h0, c0, hs, save_g, save_c = ctx.saved_tensors
        T, B, Cin, Ch, H, W = ctx.geom
        M, K, C4 = B * H * W, Cin + Ch, 4 * Ch
        ghs, ghT, gcT = (None if g is None else _raw_dense_cl(g) for g in (ghs, ghT, gcT))
        st = _stream()
        dgates = _new_cl((T, B), C4, H, W, x)
        dx = _new_cl((T, B), Cin, H, W, x) if ctx.needs_input_grad[0] else None
        dh0 = _new_cl((B,), Ch, H, W, x) if (h0 is not None and ctx.needs_input_grad[2]) else None
        dc0 = _new_cl((B,), Ch, H, W, x) if (c0 is not None and ctx.needs_input_grad[3]) else None
        _hip.call("snn_convlstm_seq_bwd", w_ohwi.data_ptr(), save_g.data_ptr(), save_c.data_ptr(), _ptr(c0), _ptr(ghs),
                  _ptr(ghT), _ptr(gcT), dgates.data_ptr(), _ptr(dx), Cin, _ptr(dh0), _ptr(dc0), T, M, Cin, Ch, st)
        dw = None
        if ctx.needs_input_grad[1]:
            # xh = [x ; h_prev] per frame, h_prev = h0 followed by hs[0 .. T-2]
            xh = _new_cl((T, B), K, H, W, x)
            _hip.call("snn_copy_channels", x.data_ptr(), cl_stride(x), xh.data_ptr(), K, T * M, Cin, st)
            hp = xh.narrow(2, Cin, Ch)
            if h0 is None:
                hp[0].zero_()
            else:
                _hip.call("snn_copy_channels", h0.data_ptr(), Ch, hp.data_ptr(), K, M, Ch, st)
            if T > 1:
                _hip.call("snn_copy_channels", hs.data_ptr(), Ch, hp[1].data_ptr(), K, (T - 1) * M, Ch, st)
            splitk = _hip.query("snn_conv2d_wgrad_splitk", T * B, H, W, K, H, W, C4, 1, 1, 1, 0, ctx.prec)
            slot = ctx.slot
            with _WgradLaunch(x.device, slot is not None, splitk, C4, K, hold=(xh, dgates)) as (stream, ws, _):
                if slot is not None:
                    dst, accumulate = slot.buf, slot.claim()
                else:
                    dst, accumulate = torch.empty((C4, 1, 1, K), device=x.device, dtype=_F32), 0
                _hip.call("snn_conv2d_wgrad", xh.data_ptr(), K, dgates.data_ptr(), C4, dst.data_ptr(), T * B, H, W, K, H, W,
                          C4, 1, 1, 1, 0, accumulate, ws.data_ptr(), splitk, ctx.prec, stream)
            if slot is None:
                dw = dst.permute(0, 3, 1, 2)
        return dx, dw, dh0, dc0, None, None


def conv_lstm_sequence(X: torch.Tensor, weight: torch.Tensor, state: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                       backward_precision: Optional[str] = None):
    """ConvLSTM with 1x1 gates over a whole sequence ``[T,B,Cin,H,W]`` -> ``(hs, (h_T, c_T))``; ``weight`` is the gate
    convolution's ``[4Ch, Cin+Ch, 1, 1]`` (gate order input, forget, output, candidate), ``state`` an ``(h0, c0)`` pair of
    ``[B,Ch,H,W]`` or None for zeros.  The gate products are exact fp32 (fp32 MFMA); ``backward_precision`` is the weight
    gradient's arithmetic (None = the session default).  Shapes outside ``conv_lstm_scan_covers`` are an error here:
    ``layer_gen.ConvLSTM`` routes them to the stepwise path."""
    h0, c0 = (None, None) if state is None else state
    if (h0 is None) != (c0 is None):
        raise RuntimeError("conv_lstm_sequence: the state is an (h, c) pair or None")
    hs, hT, cT = _ConvLstmSeq.apply(X, weight, h0, c0, _slot_of(weight), _prec_codes(None, backward_precision)[1])
    return hs, (hT, cT)


class _StackTime(Function):
    """``torch.stack`` over per-timestep ``[B,C,H,W]`` results into one channels-last ``[T,B,C,H,W]``."""

    @staticmethod
    def forward(ctx, *xs):
        xs = [_raw_to_cl(x) for x in xs]
        B, C, H, W = xs[0].shape
        out = _new_cl((len(xs), B), C, H, W, xs[0])
        M, st = B * H * W, _stream()
        for t, x in enumerate(xs):
            _hip.call("snn_copy_channels", x.data_ptr(), cl_stride(x), out[t].data_ptr(), C, M, C, st)
        return out

    @staticmethod
    def backward(ctx, g):
        return tuple(g[t] for t in range(g.shape[0]))


def stack_time(xs: List[torch.Tensor]) -> torch.Tensor:
    if xs and xs[0].dtype == _BF16:
        return torch.stack(list(xs))   # (time-outer loops are off the layer-major path) torch's copy
    return _StackTime.apply(*xs)
