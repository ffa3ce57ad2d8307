"""Gradient clipping and the non-finite step skip under data parallelism: two ranks with different shards, both on the
one GPU of the test box, exchanging through gloo (fresh child processes, as tests/test_gpu_dp_model.py).  The clip acts
on the AVERAGED gradient - the norm kernel runs inside ``FlatTrainer.step()`` behind the exchange - so both ranks clip by
the same factor and skip the same steps without a collective of their own."""
import datetime
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.util import synthetic_events, synthetic_labels

pytestmark = pytest.mark.gpu
T, B_RANK, H, W = 3, 2, 32, 48
LR = 1e-3
CLIP = 5e-6     # below half the averaged gradient's norm of this model and batch (the test asserts it): the clip is active


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir, overlap, inject):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
    try:
        import snn_for_object_detection_amd as S
        from snn_for_object_detection_amd.trainer import FlatTrainer, broadcast_parameters
        torch.manual_seed(100 + rank)            # ranks start from different weights; the broadcast aligns them
        model = S.TinyYolo(num_classes=2, time_window=0).cuda().train()
        kw = {"skip_nonfinite": True} if inject else {"gradient_clip_val": CLIP}
        tr = FlatTrainer(model, lr=LR, overlap_grad_exchange=overlap, **kw)
        assert (tr._early_lo is not None) == overlap
        broadcast_parameters(tr)
        start = tr.flat_param.detach().cpu().clone()
        X, labels = synthetic_events(T, B_RANK, H, W, p=0.08, seed=10 + rank), synthetic_labels(B_RANK, seed=20 + rank)
        tr.zero_grad()
        model.training_step((X.cuda(), labels.cuda())).backward()
        tr.synchronize()     # the neck / head part is the rank SUM already when the exchange is overlapped
        if inject and rank == 1:
            assert tr._early_lo is None or 5 < tr._early_lo     # a part that is still this rank's own
            tr.flat_grad[5] = float("inf")
        local = tr.flat_grad.detach().cpu().clone()
        tr.step()
        torch.cuda.synchronize()
        torch.save({"start": start, "local": local, "early_lo": tr._early_lo, "numel": tr.numel,
                    "after": tr.flat_param.detach().cpu().clone(), "exp_inf": tr.exp_inf.detach().cpu().clone(),
                    "norm": float(tr.last_grad_norm), "skipped": tr.skipped_steps, "steps": list(tr.param_steps),
                    "world": dist.get_world_size(), "offsets": list(tr._offsets)},
                   os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def _averaged(r):
    """The two ranks' gradients averaged, from what each rank held between backward() and step()."""
    lo = r[0]["early_lo"] if r[0]["early_lo"] is not None else r[0]["local"].numel()
    assert torch.equal(r[0]["local"][lo:], r[1]["local"][lo:])          # already summed by the overlapped exchange
    total = torch.cat([r[0]["local"][:lo].double() + r[1]["local"][:lo].double(), r[0]["local"][lo:].double()])
    return (total / 2)[: r[0]["numel"]]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("overlap", [True, False], ids=["overlapped-exchange", "one-exchange"])
def test_two_ranks_clip_the_averaged_gradient(tmp_path, hip_lib, overlap):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), overlap, False), nprocs=world, join=True)
    r = [torch.load(tmp_path / f"rank{k}.pt") for k in range(world)]
    assert r[0]["world"] == 2 and torch.equal(r[0]["start"], r[1]["start"])
    assert not torch.equal(r[0]["local"], r[1]["local"])                # different shards
    assert torch.equal(r[0]["after"], r[1]["after"])                    # the replicas stayed together, bit for bit
    # CPU restatement: average, clip_grad_norm_, Adamax - on fp64 copies
    numel = r[0]["numel"]
    p = torch.nn.Parameter(r[0]["start"][:numel].double())
    p.grad = _averaged(r)
    total = float(torch.nn.utils.clip_grad_norm_([p], CLIP))
    assert total > 2 * CLIP                                             # the clip is active
    torch.optim.Adamax([p], lr=LR).step()
    for k in range(world):                                              # the norm of the AVERAGED gradient, on both ranks
        assert abs(r[k]["norm"] - total) <= 1e-6 * total, (k, r[k]["norm"], total)
    # the yardstick of tests/test_gpu_grad_clip.py: twice the deviation the unclipped step shows against the same fp64
    # reference - here for this very step, on the same averaged gradient
    got = r[0]["after"].double()
    off = r[0]["offsets"]
    dev = max(float((got[lo:hi] - p.detach()[lo:hi]).norm() / p.detach()[lo:hi].norm().clamp_min(1e-30))
              for lo, hi in zip(off[:-1], off[1:]))
    print(f"two-rank clipped step: largest relative parameter deviation {dev:.3e}")
    assert dev <= 2 * _unclipped_deviation(r), dev
    assert r[0]["skipped"] == r[1]["skipped"] == 0


def _unclipped_deviation(r):
    """The same yardstick as tests/test_gpu_grad_clip.py, for THIS step: the fused Adamax without a clip (the plain C-ABI
    step on the averaged gradient) against torch.optim.Adamax in fp64, largest relative deviation over the parameters."""
    from snn_for_object_detection_amd import _hip
    numel = r[0]["numel"]
    avg = _averaged(r)
    p = torch.nn.Parameter(r[0]["start"][:numel].double())
    p.grad = avg.clone()
    torch.optim.Adamax([p], lr=LR).step()
    dp, dg = r[0]["start"][:numel].cuda(), avg.float().cuda()
    m, u = torch.zeros_like(dp), torch.zeros_like(dp)
    _hip.call("snn_adamax_step", dp.data_ptr(), dg.data_ptr(), m.data_ptr(), u.data_ptr(), numel, LR, 0.9, 0.999, 1e-8, 1,
              1.0, torch.cuda.current_stream().cuda_stream)
    got, off = dp.double().cpu(), r[0]["offsets"]
    dev = max(float((got[lo:hi] - p.detach()[lo:hi]).norm() / p.detach()[lo:hi].norm().clamp_min(1e-30))
              for lo, hi in zip(off[:-1], off[1:]))
    print(f"unclipped step on the same averaged gradient: largest relative parameter deviation {dev:.3e}")
    return dev


@pytest.mark.timeout(300)
def test_an_inf_on_one_rank_makes_both_ranks_skip(tmp_path, hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), True, True), nprocs=world, join=True)
    r = [torch.load(tmp_path / f"rank{k}.pt") for k in range(world)]
    assert torch.isfinite(r[0]["local"]).all() and not torch.isfinite(r[1]["local"]).all()   # rank 1 alone
    for k in range(world):
        assert torch.equal(r[k]["after"], r[k]["start"]), k             # parameters bit-unchanged
        assert float(r[k]["exp_inf"].abs().max()) == 0.0                # ... and so are the moments
        assert r[k]["skipped"] == 1 and set(r[k]["steps"]) == {0}, k
        assert r[k]["norm"] == float("inf")
