"""Activity monitor: per-layer LIF firing rates and the synaptic operations of a forward pass.

    with activity.record(model, per_step=False) as rec:     # sets functional._ACTIVITY, restores it on exit
        model.training_step(batch)                          # or forward / validation_step / predict_sequence; steps add up
    rep = rec.report(process_group=None)                    # the only host synchronisation

While a recorder is set, every LIF layer (``functional._AffineNeuron.forward``) and every convolution
(``functional.conv2d`` / ``sibling_conv1x1``) enqueues one ``snn_activity_count`` launch on whatever its forward produced or
read; nothing else changes, and without a recorder nothing is counted, launched or allocated.  The counts are exact int64
sums kept on the device; ``report`` brings them to the host once and does the arithmetic there in Python / fp64.

LIF layers are keyed by the cell's qualified name in ``model.named_modules()``.  The source of a layer's count is, in this
order: the spike bit mask of a stage-entry scan; the spike tensor, when no shortcut is folded into its store and all steps
were written; the saved potentials, compared with ``v_th`` as the scans compare them.  A layer that has none of the three - a
fused shortcut or a last-step-only read-out under ``no_grad`` - gets a potentials buffer for that pass, free again after
the count.  In bf16 storage the potentials of a layer with a fused shortcut are the STORED (rounded) ones: the count is of
the spikes the reverse scan sees, which can differ from the forward's for a potential within one bf16 step of the
threshold.  LI, LI + Tanh, SLI and Synapse layers do not spike and are not recorded; nor is ``ConvLSTM``.

Convolutions are keyed by the weight's parameter name (a fused group - the C2f entry composed with the branch-opening
1x1 convolutions - by the names of its weights joined with ``+``: it runs, and is counted, as the one convolution it is
executed as).  Counted are the non-zero elements of the operand the kernels read: plain values, potentials above the
threshold, or mask bits.

The synaptic-operation estimate is the usual one, borders ignored: every non-zero input element feeds ``Cout * KH * KW /
stride^2`` accumulates, so ``synops = nonzero_inputs * Cout * KH * KW / stride^2``, and ``macs`` is the same with every input
element (the dense equivalent).  At a padded border fewer taps exist, so both are slight over-estimates, by the same
factor.  A depthwise convolution (``Conv(groups="depthwise")``) is recorded with the fan-out ``Cout / groups = 1``:
``synops = nonzero_inputs * KH * KW / stride^2``.
"""

import contextlib
from typing import Dict, List, Optional, Sequence

import torch

from . import _hip
from . import functional as HF


class _LifEntry:
    __slots__ = ("counts", "channels", "neurons", "sources")

    def __init__(self, counts: torch.Tensor, channels: int):
        self.counts, self.channels = counts, channels
        self.neurons = 0       # sum of T * M over the recorded forwards: neuron-timesteps per channel
        self.sources = {}      # "mask" / "spikes" / "potentials" -> forwards counted from it


class _ConvEntry:
    __slots__ = ("counts", "geometry", "inputs")

    def __init__(self, counts: torch.Tensor, geometry):
        self.counts, self.geometry = counts, geometry   # geometry: (Cout, KH, KW, stride)
        self.inputs = 0        # input elements of the recorded forwards


class Recorder:
    """What ``record`` yields: the device-side counts of the forwards run inside the block."""

    def __init__(self, model: torch.nn.Module, per_step: bool = False):
        from .layer_gen import ConvLSTM, LIFCell
        self.per_step = bool(per_step)
        # a cell is recognised by its parameter struct (what the operator receives), a weight by the parameter object
        self._cells = {id(m.params): name for name, m in model.named_modules() if isinstance(m, LIFCell)}
        self._weights = {id(p): name for name, p in model.named_parameters()}
        self._skipped = {id(m.conv.weight) for m in model.modules() if isinstance(m, ConvLSTM)}
        self._keep = model   # (ids stay valid while the objects live)
        self.lif: Dict[str, _LifEntry] = {}
        self.convs: Dict[str, _ConvEntry] = {}

    # ------------------------------------------------------------------ called by the operators
    def count_lif(self, params, mask, spikes, potentials, v_th: float, dims) -> None:
        """One LIF forward: ``mask`` (int32 ``[T,B,H,W,C/32]``), ``spikes`` (``[T,B,C,H,W]`` channels-last, possibly a
        channel slice) or ``potentials`` (dense ``[T,B,H,W,C]``, compared with ``v_th``) - the first that is not None.  In
        bf16 storage the potentials are the stored (rounded) ones: the spikes the reverse scan sees."""
        T, B, C, H, W = dims
        M = B * H * W
        name = self._cells.get(id(params))
        if name is None:
            name = f"<LIF not in the recorded model, {C} channels>"
        e = self.lif.get(name)
        fresh = e is None
        if fresh:
            shape = (T, C) if self.per_step else (C,)
            like = mask if mask is not None else (spikes if spikes is not None else potentials)
            e = self.lif[name] = _LifEntry(torch.empty(shape, device=like.device, dtype=torch.int64), C)
        elif e.channels != C or (self.per_step and e.counts.shape[0] != T):
            raise RuntimeError(f"activity.record: LIF layer {name} was first recorded with {tuple(e.counts.shape)} counts; "
                               f"this forward has T = {T}, C = {C} (per_step needs forwards of one length)")
        if mask is not None:
            src, args = "mask", (mask.data_ptr(), _hip.ACTIVITY_MASK, mask.shape[-1], 0.0)
        elif spikes is not None:
            bf = spikes.dtype == torch.bfloat16
            src, args = "spikes", (spikes.data_ptr(), _hip.ACTIVITY_NONZERO_BF16 if bf else _hip.ACTIVITY_NONZERO_F32,
                                   HF.cl_stride(spikes), 0.0)
        elif potentials is not None:
            bf = potentials.dtype == torch.bfloat16
            src, args = "potentials", (potentials.data_ptr(), _hip.ACTIVITY_ABOVE_BF16 if bf else _hip.ACTIVITY_ABOVE_F32,
                                       C, v_th)
        else:
            raise RuntimeError(f"activity.record: LIF layer {name} left neither mask, spikes nor potentials to count")
        HF._activity_launch(*args, T, M, C, self.per_step, e.counts, not fresh)
        e.neurons += T * M
        e.sources[src] = e.sources.get(src, 0) + 1

    def count_conv(self, weights: Sequence[torch.Tensor], x: torch.Tensor, x_th: Optional[float], mask, cout: int, kh: int,
                   kw: int, stride: int) -> None:
        """One convolution forward over the operand it reads: ``x`` (``[T,B,C,H,W]`` channels-last) as plain values, as
        potentials above ``x_th``, or as the bit ``mask``."""
        if any(id(w) in self._skipped for w in weights):
            return   # the gate convolution of a ConvLSTM (its step-by-step path; the scan path never comes here)
        key = "+".join(self._weights.get(id(w), f"<weight {tuple(w.shape)} not in the recorded model>") for w in weights)
        T, B, C, H, W = x.shape
        e = self.convs.get(key)
        fresh = e is None
        if fresh:
            e = self.convs[key] = _ConvEntry(torch.empty((C,), device=x.device, dtype=torch.int64), (cout, kh, kw, stride))
        elif e.counts.shape[0] != C:
            raise RuntimeError(f"activity.record: convolution {key} changed its input channels")
        if mask is not None:
            args = (mask.data_ptr(), _hip.ACTIVITY_MASK, mask.shape[-1], 0.0)
        else:
            bf = x.dtype == torch.bfloat16
            if x_th is not None:
                args = (x.data_ptr(), _hip.ACTIVITY_ABOVE_BF16 if bf else _hip.ACTIVITY_ABOVE_F32, HF.cl_stride(x), x_th)
            else:
                args = (x.data_ptr(), _hip.ACTIVITY_NONZERO_BF16 if bf else _hip.ACTIVITY_NONZERO_F32, HF.cl_stride(x), 0.0)
        HF._activity_launch(*args, T, B * H * W, C, False, e.counts, not fresh)
        e.inputs += T * B * H * W * C

    # ------------------------------------------------------------------ read-out
    def report(self, process_group=None) -> dict:
        """The counts as a report (``make_report``); with ``process_group`` summed over its ranks first, by ONE all-reduce.
        One device-to-host copy: the only host synchronisation of the recorder."""
        lif_names, conv_names = list(self.lif), list(self.convs)
        tensors = [self.lif[n].counts for n in lif_names] + [self.convs[n].counts for n in conv_names]
        host = [self.lif[n].neurons for n in lif_names] + [self.convs[n].inputs for n in conv_names]
        if not tensors:
            return make_report({}, {})
        if process_group is not None:
            # (the host-side tallies travel in the same vector)
            tensors = all_reduce_counts(tensors + [torch.tensor(host, dtype=torch.int64).to(tensors[0].device)], process_group)
        flat = torch.cat([t.reshape(-1) for t in tensors]).cpu()
        parts = [p.reshape(t.shape) for p, t in zip(torch.split(flat, [t.numel() for t in tensors]), tensors)]
        if process_group is not None:
            host = [int(v) for v in parts.pop()]
        n = len(lif_names)
        lif = {name: (parts[k], host[k]) for k, name in enumerate(lif_names)}
        convs = {name: (int(parts[n + k].sum()), host[n + k], *self.convs[name].geometry) for k, name in enumerate(conv_names)}
        rep = make_report(lif, convs)
        for name in lif_names:
            rep["layers"][name]["sources"] = dict(self.lif[name].sources)
        return rep


def all_reduce_counts(tensors: List[torch.Tensor], process_group=None) -> List[torch.Tensor]:
    """Sum every int64 tensor of the list over the ranks of ``process_group`` with ONE all-reduce of one concatenated
    vector (device tensors over the device backend, CPU tensors over gloo); returns the sums in the shapes given."""
    import torch.distributed as dist
    flat = torch.cat([t.reshape(-1) for t in tensors])
    if flat.dtype != torch.int64:
        raise RuntimeError("all_reduce_counts: counts are int64")
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=process_group)
    return [p.reshape(t.shape) for p, t in zip(torch.split(flat, [t.numel() for t in tensors]), tensors)]


def make_report(lif: dict, convs: dict) -> dict:
    """Host arithmetic (Python integers and fp64) of a report.

    ``lif``: ``{name: (spikes int64 [C] or [T,C], neurons)}`` with ``neurons`` the neuron-timesteps per channel (sum of T * M
    over the recorded forwards).  ``convs``: ``{name: (nonzero_inputs, inputs, Cout, KH, KW, stride)}``.

    -> ``{"layers": {name: {spikes, neurons, rate, channel_rate, dead_channels, saturated_channels}},
    "convs": {name: {nonzero_inputs, inputs, density, synops, macs}}, "totals": {synops, macs, rate, spikes, neurons}}``:
    ``rate`` is spikes per neuron-timestep (the layer's mean; ``channel_rate`` fp64 ``[C]``), a dead channel never spiked, a
    saturated one spiked at every neuron-timestep; ``synops = nonzero_inputs * Cout * KH * KW / stride^2`` and ``macs`` the
    same for all ``inputs`` - the border-free estimate; the total ``rate`` weighs every layer by its neurons."""
    layers, total_spikes, total_neurons = {}, 0, 0
    for name, (spikes, neurons) in lif.items():
        spikes = spikes.to(torch.int64).cpu()
        per_channel = spikes if spikes.dim() == 1 else spikes.sum(0)
        C = per_channel.numel()
        neurons = int(neurons)
        n_spikes = int(per_channel.sum())
        layers[name] = {
            "spikes": spikes,
            "neurons": neurons,
            "rate": n_spikes / (neurons * C) if neurons else 0.0,
            "channel_rate": per_channel.to(torch.float64) / neurons if neurons else torch.zeros(C, dtype=torch.float64),
            "dead_channels": [int(c) for c in torch.nonzero(per_channel == 0).flatten()],
            "saturated_channels": [int(c) for c in torch.nonzero(per_channel == neurons).flatten()] if neurons else [],
        }
        total_spikes += n_spikes
        total_neurons += neurons * C
    out_convs, synops, macs = {}, 0.0, 0.0
    for name, (nonzero, inputs, cout, kh, kw, stride) in convs.items():
        fan = cout * kh * kw / float(stride * stride)
        out_convs[name] = {"nonzero_inputs": int(nonzero), "inputs": int(inputs),
                           "density": int(nonzero) / int(inputs) if inputs else 0.0,
                           "synops": int(nonzero) * fan, "macs": int(inputs) * fan}
        synops += out_convs[name]["synops"]
        macs += out_convs[name]["macs"]
    return {"layers": layers, "convs": out_convs,
            "totals": {"synops": synops, "macs": macs, "spikes": total_spikes, "neurons": total_neurons,
                       "rate": total_spikes / total_neurons if total_neurons else 0.0}}


def format_report(rep: dict) -> str:
    """The per-layer table ``tools/activity_report.py`` prints."""
    lines = [f"{'LIF layer':<58}{'C':>5}{'rate':>9}{'dead':>6}{'sat':>5}  source"]
    for name, r in rep["layers"].items():
        C = r["channel_rate"].numel()
        lines.append(f"{name:<58}{C:>5}{r['rate']:>9.4f}{len(r['dead_channels']):>6}{len(r['saturated_channels']):>5}  "
                     + ",".join(sorted(r.get("sources", {}))))
    lines.append(f"{'convolution':<58}{'density':>10}{'MSynOps':>12}{'MMACs':>12}")
    for name, r in rep["convs"].items():
        short = name if len(name) <= 57 else name[:27] + "..." + name[-27:]
        lines.append(f"{short:<58}{r['density']:>10.4f}{r['synops'] / 1e6:>12.2f}{r['macs'] / 1e6:>12.2f}")
    t = rep["totals"]
    lines.append(f"total: {t['synops'] / 1e9:.3f} GSynOps of {t['macs'] / 1e9:.3f} GMACs dense "
                 f"({t['synops'] / t['macs'] if t['macs'] else 0.0:.4f}); mean firing rate {t['rate']:.4f} over "
                 f"{t['neurons']} neuron-timesteps")
    return "\n".join(lines)


@contextlib.contextmanager
def record(model: torch.nn.Module, per_step: bool = False):
    """Count the spikes of every LIF layer and the non-zero operands of every convolution of ``model`` in the forwards run
    inside the block; ``per_step``: LIF counts per timestep (``[T,C]``; the forwards must then have one length).  A
    ``Recorder`` in place of the model is switched on again and keeps adding to its counts."""
    rec = model if isinstance(model, Recorder) else Recorder(model, per_step)
    previous = HF._ACTIVITY
    HF._ACTIVITY = rec
    try:
        yield rec
    finally:
        HF._ACTIVITY = previous
