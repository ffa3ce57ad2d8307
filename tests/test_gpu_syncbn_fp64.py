"""SyncBatchNorm (config/config.yaml:76) of the fused Norm -> neuron layer against the float64 restatement of
tests/norm_neuron_ref.py: the group's statistics (snn_bn_stats_reduce, snn_bn_stats_from_sums), the backward's sums and
coefficients (snn_bn_bwd_reduce[_from_state], snn_bn_bwd_coef), the glue of ``functional._bn_coefficients`` /
``_sync_bn_bwd_coefficients``, and the reverse scan such a layer launches ONCE over a sequence of any length.

Rows, inputs, device run, reference and checks are those of tests/test_gpu_norm_neuron_fp64.py; nothing here has a
tolerance of its own.  The SyncBatchNorm path differs from the single-process one in the order of fp64 additions and in
one fp64 -> fp32 rounding of the same quantities, so FWD_REL, TOL_LINEAR, TOL_STATE, the spike rule and the term-magnitude
scales of ``check_grads`` hold as derived there; the sum of two ranks' fp32 dgamma / dbias stays inside tol * sum|terms|
because each rank's part is bounded by tol times its own share of the terms.

* one rank: a group of one (gloo over an in-process HashStore) must reproduce the reference on every train-mode row of
  that table, and on long sequences whose one launch caps the channels per block by LDS;
* two ranks: a pair of workers, each with half of the batch, on the one GPU of the test box (gloo on 127.0.0.1 - the
  production transport is RCCL); the concatenated halves must match the reference of the FULL batch, the ranks' dgamma /
  dbias add up to its gradients, and the ranks' running statistics are bit-equal.
Every run proves by the names of its C-ABI calls that it went through the SyncBatchNorm kernels.
The observed maxima (error / bound) per row go to the SNN_FP64_RECORD file under ``<row>/sync1_<variant>`` and
``<row>/sync2_<variant>``.
"""
import datetime
import os
import socket
import zlib
from collections import OrderedDict

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import norm_neuron_ref as R
from tests.test_gpu_norm_neuron_fp64 import (CASES, Case, D, DevResult, _is_prod, _record, batch_share, check_forward,
                                             check_grads, make_inputs, plan_classes, plan_of, run_device, run_ref)

pytestmark = pytest.mark.gpu

SYNC_VARIANTS = ("default", "no_yfree")
# ---- a group of one: every non-production train-mode row of the table, and TinyYolo's 15x19 LIF layer
ONE_RANK = [(cs, v) for cs in CASES if cs.bn == "train" and (not _is_prod(cs) or cs.id == "prod_lif256_15x19")
            for v in cs.variants if v in SYNC_VARIANTS]
# ---- long sequences: a SyncBatchNorm layer's reverse scan is never segmented, the slabs of all T steps are in LDS
ONE_LAUNCH = [
    Case("lif_c64_t70_one", R.LIF, 70, 2, 64, 5, 6, classes=("mode1", "lds_capped", "cvb4"), variants=SYNC_VARIANTS),
    Case("lif_c64_t128_one", R.LIF, 128, 2, 64, 5, 6, classes=("mode1", "lds_capped", "cvb4")),
    Case("li_c100_t128_one", R.LI, 128, 1, 100, 3, 4, classes=("mode2", "lds_capped")),
    # (8 channel groups and room for 12: the one launch that is NOT capped)
    Case("litanh_c32_t40_last_one", R.LI_TANH, 40, 2, 32, 5, 9, last_only=True, classes=("mode1", "cvb8")),
]
# ---- two ranks; B is the global batch, each rank takes one half of it
TWO_RANK = [
    Case("lif_c4", R.LIF, 8, 2, 4, 7, 7, variants=SYNC_VARIANTS),              # odd pixel count per rank
    Case("lif_c3_vec1", R.LIF, 6, 2, 3, 9, 10, variants=SYNC_VARIANTS),
    Case("lif_c64", R.LIF, 6, 2, 64, 5, 6, variants=SYNC_VARIANTS),
    Case("lif_c512_gy", R.LIF, 32, 2, 512, 6, 7, variants=SYNC_VARIANTS),
    Case("li_c16_state0d", R.LI, 5, 2, 16, 6, 7, state=True, v0_scalar=True),
    Case("litanh_c32_last", R.LI_TANH, 7, 2, 32, 5, 9, last_only=True),
    Case("none_c24_mode2", R.NONE, 6, 2, 24, 7, 8),
    Case("sli_c36_mode2", R.SLI, 5, 2, 36, 6, 6),
    Case("lif_y_slice_offset1", R.LIF, 6, 2, 16, 6, 7, y_off=1, variants=SYNC_VARIANTS),
    Case("lif_addend", R.LIF, 6, 2, 16, 6, 7, addend=True, variants=SYNC_VARIANTS),
    Case("lif_dest", R.LIF, 6, 2, 16, 6, 7, dest=True, variants=SYNC_VARIANTS),
    Case("lif_c64_t70_one", R.LIF, 70, 2, 64, 5, 6, variants=SYNC_VARIANTS),
    Case("li_c100_t128_one", R.LI, 128, 2, 100, 3, 4),
    Case("lif_rpb_gt1", R.LIF, 8, 4, 16, 90, 100, variants=SYNC_VARIANTS),    # more than one pixel block per rank
]
TWO_RANK_RUNS = [(cs, v) for cs in TWO_RANK for v in cs.variants]
WORLD = 2
SYNC_CALLS = ("snn_bn_stats_reduce", "snn_bn_stats_from_sums", "snn_bn_bwd_coef")


def _seed(cs):
    return zlib.crc32(cs.id.encode()) % 10007


def _ids(runs):
    return [f"{cs.id}-{v}" for cs, v in runs]


@pytest.fixture(scope="module")
def HF(hip_lib):
    from snn_for_object_detection_amd import functional
    return functional


@pytest.fixture(scope="module")
def group(hip_lib):
    """A process group of this process alone, over an in-process store."""
    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        yield dist.group.WORLD
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def ref_of():
    """The reference of a row, computed once and shared by the row's variants and controls (the two latest rows are kept)."""
    kept = OrderedDict()

    def get(tag, cs, inp, z, dev):
        key = (tag, cs)
        if key not in kept:
            while len(kept) >= 2:
                kept.popitem(last=False)
            kept[key] = (z, run_ref(cs, inp, z, dev))
        kept.move_to_end(key)
        z0, ref = kept[key]
        if z is not None:
            assert torch.equal(z, z0.to(z.device)), f"{cs.id}: the spikes differ from the row's first variant's"
        return ref

    yield get
    kept.clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------ the calls of a run
class _Names:
    def __init__(self):
        self.names = []

    def before(self, name, args):
        self.names.append(name)

    def after(self, token):
        pass


def run_recorded(HF, cs, inp, variant, **kw):
    """``run_device`` and the names of the C-ABI calls it made."""
    from snn_for_object_detection_amd import _hip
    _hip.PROFILER = spy = _Names()
    try:
        res = run_device(HF, cs, inp, variant, **kw)
    finally:
        _hip.PROFILER = None
    return res, spy.names


def plain_takes_state_sums(HF, cs, inp, variant, **kw):
    """The run of this row and variant WITHOUT SyncBatchNorm forms the backward's second sum from the saved potentials.

    One exception is not the row's but the segmentation's: a plain sequence of SCAN_SEGMENT_T * k + 1 steps reads y because
    its second segment, one step long, has a single potential to look back on.  The one launch of a SyncBatchNorm layer has
    no such segment, so for such a length the plain run is asked unsegmented - after showing that it is this rule alone
    that kept the segmented run from the state-derived sums."""
    _, names = run_recorded(HF, cs, inp, variant, **kw)
    took = "snn_bn_bwd_finalize_from_state" in names
    seg = HF.SCAN_SEGMENT_T
    if seg and cs.T > seg and cs.T % seg == 1:
        assert not took, "a plain scan whose second segment is one step long reads y"
        with HF.levers(SCAN_SEGMENT_T=None):
            _, names = run_recorded(HF, cs, inp, variant, **kw)
        assert names.count("snn_affine_neuron_bwd") == 1
        took = "snn_bn_bwd_finalize_from_state" in names
    return took


def check_sync_calls(cs, names, from_state, segment_t, fails, who=""):
    """The run went through the SyncBatchNorm kernels - the reduce the plain run's choice of sums asks for - and through
    none of the single-process ones, and scanned a long sequence in one launch."""
    for n in SYNC_CALLS:
        if n not in names:
            fails.append(f"calls{who}: no {n}")
    want, other = "snn_bn_bwd_reduce_from_state", "snn_bn_bwd_reduce"
    if not from_state:
        want, other = other, want
    if want not in names or other in names:
        fails.append(f"calls{who}: expected {want}, not {other}")
    single = [n for n in names if n == "snn_bn_stats_finalize" or n.startswith("snn_bn_bwd_finalize")]
    if single:
        fails.append(f"calls{who}: single-process BatchNorm kernels {sorted(set(single))}")
    if cs.T > segment_t and names.count("snn_affine_neuron_bwd") != 1:
        fails.append(f"calls{who}: {names.count('snn_affine_neuron_bwd')} reverse-scan launches for T = {cs.T}")


# ------------------------------------------------------------------------------------------------------ one rank
def _one_rank(HF, group, ref_of, cs, variant):
    inp = make_inputs(cs, _seed(cs))
    res, names = run_recorded(HF, cs, inp, variant, sync_group=group)
    from_state = plain_takes_state_sums(HF, cs, inp, variant)
    ref = ref_of("sync1", cs, inp, res.z, "cuda" if _is_prod(cs) else "cpu")
    pl = plan_of(HF, cs, variant, one_launch=True)
    fails, rec = [], {"plan": list(pl)}
    check_forward(cs, res, ref, fails, rec)
    check_grads(cs, res, ref, fails, rec)
    check_sync_calls(cs, names, from_state, HF.SCAN_SEGMENT_T, fails)
    _record(cs, f"sync1_{variant}", rec)
    assert not fails, f"{cs.id} [{variant}]:\n  " + "\n  ".join(fails)
    return pl, from_state


@pytest.mark.parametrize("cs, variant", ONE_RANK, ids=_ids(ONE_RANK))
def test_group_of_one_against_fp64(HF, group, ref_of, cs, variant):
    _one_rank(HF, group, ref_of, cs, variant)


ONE_LAUNCH_RUNS = [(cs, v) for cs in ONE_LAUNCH for v in cs.variants]


@pytest.mark.parametrize("cs, variant", ONE_LAUNCH_RUNS, ids=_ids(ONE_LAUNCH_RUNS))
def test_long_sequence_in_one_launch_against_fp64(HF, group, ref_of, cs, variant):
    assert cs.T > HF.SCAN_SEGMENT_T
    got = plan_classes(plan_of(HF, cs, variant, one_launch=True))
    assert set(cs.classes) <= got, (cs.id, got)
    # max_cvb = 64 KiB / (slabs * T * 8 * vec): 4 of 16 channel groups at C = 64 (T = 70: 7, T = 128: 4, kept a power of
    # two), 16 of 25 at C = 100 on the one slab of the LDS-atomics plan, 12 >= 8 at C = 32, T = 40
    assert ("lds_capped" in got) == (cs.id != "litanh_c32_t40_last_one"), (cs.id, got)
    _, from_state = _one_rank(HF, group, ref_of, cs, variant)
    if cs.neuron == R.LIF and cs.C == 64:
        assert from_state == (variant == "default"), "the y-free scan is what a Norm -> LIF layer of 64 channels takes"


# ------------------------------------------------------------------------------------------------------ two ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _host(res):
    """A DevResult as a dict of host tensors (fp32: the values came from fp32 tensors, nothing is rounded)."""
    h = lambda t: None if t is None else t.to(torch.float32).cpu()   # noqa: E731
    d = res._asdict()
    return {k: ({n: h(g) for n, g in v.items()} if k == "grads" else v if k == "guard_ok" else h(v)) for k, v in d.items()}


def _two_rank_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
    try:
        from snn_for_object_detection_amd import functional as HF
        runs = {}
        for cs, variant in TWO_RANK_RUNS:
            inp = make_inputs(cs, _seed(cs))   # the full batch from the row's seed; this rank runs its half
            half = cs.B // world
            share = slice(rank * half, (rank + 1) * half)
            res, names = run_recorded(HF, cs, inp, variant, sync_group=dist.group.WORLD, batch=share)
            runs[f"{cs.id}/{variant}"] = {"res": _host(res), "names": names,
                                          "from_state": plain_takes_state_sums(HF, cs, inp, variant, batch=share)}
        torch.cuda.synchronize()
        torch.save(runs, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(hip_lib, tmp_path_factory):
    """One pair of workers runs the whole table; a worker that fails ends the fixture."""
    out_dir = tmp_path_factory.mktemp("syncbn_fp64")
    mp.spawn(_two_rank_worker, args=(WORLD, _free_port(), str(out_dir)), nprocs=WORLD, join=True)
    return [torch.load(out_dir / f"rank{k}.pt") for k in range(WORLD)]


def combine(cs, parts):
    """The ranks' results as one of the full batch: per-sample tensors concatenated along B, the rank-local parameter
    gradients (and the gradient of LI's 0-dim initial v) added in fp64, rank 0's running statistics."""
    def cat(k, dim):
        return None if parts[0][k] is None else torch.cat([p[k] for p in parts], dim).to(D)
    grads = {}
    for k, g0 in parts[0]["grads"].items():
        gs = [p["grads"][k] for p in parts]
        if g0 is None:
            grads[k] = None
        elif k in ("dgamma", "dbias") or g0.dim() == 0:
            grads[k] = sum(g.to(D) for g in gs)
        else:
            grads[k] = torch.cat(gs, 1 if k in ("dy", "daddend") else 0).to(D)
    return DevResult(cat("out", 0 if cs.last_only else 1), cat("z", 1), cat("vT", 0), cat("iT", 0), parts[0]["rm"].to(D),
                     parts[0]["rv"].to(D), grads, all(p["guard_ok"] for p in parts))


def _two_rank_row(two_ranks, ref_of, cs, variant="default"):
    runs = [r[f"{cs.id}/{variant}"] for r in two_ranks]
    res = combine(cs, [r["res"] for r in runs])
    inp = make_inputs(cs, _seed(cs))
    return runs, res, inp, ref_of("sync2", cs, inp, res.z, "cpu")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("cs, variant", TWO_RANK_RUNS, ids=_ids(TWO_RANK_RUNS))
def test_two_ranks_against_fp64_of_the_full_batch(HF, two_ranks, ref_of, cs, variant):
    assert cs.B % WORLD == 0
    runs, res, inp, ref = _two_rank_row(two_ranks, ref_of, cs, variant)
    fails, rec = [], {}
    check_forward(cs, res, ref, fails, rec)
    check_grads(cs, res, ref, fails, rec)
    for k, r in enumerate(runs):
        check_sync_calls(cs, r["names"], r["from_state"], HF.SCAN_SEGMENT_T, fails, f" of rank {k}")
    for name in ("rm", "rv"):
        if not torch.equal(runs[0]["res"][name], runs[1]["res"][name]):
            fails.append(f"running statistics: the ranks' {name} differ")
    _record(cs, f"sync2_{variant}", rec)
    assert not fails, f"{cs.id} [{variant}]:\n  " + "\n  ".join(fails)


# ------------------------------------------------------------------------------------------------------ negative controls
# Each check family must fail against a deliberately wrong reference of the two-rank run.
CONTROL_ROWS = [next(c for c in TWO_RANK if c.id == i) for i in ("lif_rpb_gt1", "lif_c64")]
_control = pytest.mark.parametrize("cs", CONTROL_ROWS, ids=[c.id for c in CONTROL_ROWS])


@pytest.mark.timeout(300)
@_control
def test_control_statistics_of_each_half_batch(two_ranks, ref_of, cs):
    """A reference that normalises each rank's half with the half's own statistics: spikes and dy must fail."""
    runs, res, inp, ref = _two_rank_row(two_ranks, ref_of, cs)
    half = cs.B // WORLD
    halves = []
    for k in range(WORLD):
        share = slice(k * half, (k + 1) * half)
        cs_k, inp_k = batch_share(cs, inp, share)
        halves.append(run_ref(cs_k, inp_k, res.z[:, share], "cpu"))
    fails = []
    check_forward(cs, res, ref._replace(vdec=torch.cat([h.vdec for h in halves], 1)), fails, {})
    assert any(f.startswith("spikes") for f in fails), fails
    fails = []
    check_grads(cs, res, ref, fails, {}, grads=dict(ref.grads, dy=torch.cat([h.grads["dy"] for h in halves], 1)))
    assert any(f.startswith("dy per") for f in fails), fails


@pytest.mark.timeout(300)
@_control
def test_control_parameter_gradients_of_rank_0_alone(two_ranks, ref_of, cs):
    """dgamma / dbias summed over the samples of rank 0 only: both must fail."""
    runs, res, inp, ref = _two_rank_row(two_ranks, ref_of, cs)
    half = cs.B // WORLD
    s1, s2 = R.bn_backward_sums(ref.gx[:, :half], ref.bn.xhat[:, :half])
    # (over all samples the sums are autograd's gradients: the control differs from the reference only by the samples)
    a1, a2 = R.bn_backward_sums(ref.gx, ref.bn.xhat)
    assert float((a2.sum(0) - ref.grads["dgamma"]).norm() / ref.grads["dgamma"].norm()) < 1e-12
    assert float((a1.sum(0) - ref.grads["dbias"]).norm() / ref.grads["dbias"].norm()) < 1e-12
    fails = []
    check_grads(cs, res, ref, fails, {}, grads=dict(ref.grads, dgamma=s2.sum(0), dbias=s1.sum(0)))
    for fam in ("dgamma", "dbias"):
        assert any(f.startswith(fam) for f in fails), (fam, fails)


@pytest.mark.timeout(300)
@_control
def test_control_running_variance_unbiased_over_the_local_pixels(two_ranks, ref_of, cs):
    """Running variance with M / (M - 1) of one rank's pixel count M instead of the group's: running_var must fail,
    running_mean must not."""
    runs, res, inp, ref = _two_rank_row(two_ranks, ref_of, cs)
    m = (cs.B // WORLD) * cs.H * cs.W
    rv = inp.rv.to(D)
    for t in range(cs.T):
        rv = 0.9 * rv + 0.1 * ref.bn.var[t] * (m / (m - 1.0))   # momentum 0.1, as the reference updates
    fails = []
    check_forward(cs, res, ref._replace(rv=rv), fails, {})
    assert any(f.startswith("running_var") for f in fails) and not any(f.startswith("running_mean") for f in fails), fails
