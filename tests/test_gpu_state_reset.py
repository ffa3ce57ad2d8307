"""``functional.reset_state_`` / ``snn_state_reset``: the samples marked in ``first`` go back to rest in every tensor of a
state tree with one launch, and nothing else changes - per element, bit for bit, against a NumPy restatement.  Every
tensor lies inside a larger buffer of random bits, so that a store in front of, behind or between the marked blocks
shows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3
GUARD = 37                                                 # floats on either side of every tensor
FIRSTS = ([0, 0, 0], [1, 1, 1], [0, 1, 0], [1, 0, 0], [0, 0, 1])
# elements per sample: 1, 3 (blocks unaligned to 16 bytes whatever the base), 5, 4k, 4k + 2, and one that a block walks
# more than once (16 chunks x 256 threads x 4 floats = 16384 per pass)
SIZES = (1, 3, 5, 8, 10, 4 * 5000 + 2)


@pytest.fixture(scope="module")
def HF(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from snn_for_object_detection_amd import functional
    return functional


class Guarded:
    """A float32 tensor ``shape`` (``[B, ...]``) at ``offset`` floats (mod 4: its alignment) inside a buffer of random
    bits with ``GUARD`` floats on either side."""

    def __init__(self, shape, offset, seed, channels_last=False):
        n = int(np.prod(shape))
        rng = np.random.default_rng(seed)
        bits = rng.integers(0, 1 << 32, size=offset + GUARD + n + GUARD, dtype=np.uint32)
        bits = np.where((bits & 0x7F800000) == 0x7F800000, bits & 0x807FFFFF, bits)   # (no NaN / Inf patterns)
        self.before = bits.astype(np.uint32)
        self.buf = torch.from_numpy(self.before.view(np.int32).copy()).cuda().view(torch.float32)
        self.lo, self.n = offset + GUARD, n
        flat = self.buf[self.lo:self.lo + n]
        if channels_last:
            b, c, h, w = shape
            self.t = flat.view(b, h, w, c).permute(0, 3, 1, 2)
        else:
            self.t = flat.view(*shape)
        assert self.t.data_ptr() % 16 == (self.buf.data_ptr() + 4 * self.lo) % 16

    def want(self, first, rest=0.0):
        out = self.before.copy()
        per = self.n // B
        for b, f in enumerate(first):
            if f:
                out[self.lo + b * per:self.lo + (b + 1) * per] = np.float32(rest).view(np.uint32)
        return out

    def got(self):
        return self.buf.view(torch.int32).cpu().numpy().view(np.uint32)


def _flat_leaves(tree):
    if isinstance(tree, torch.Tensor):
        return [tree]
    if isinstance(tree, (list, tuple)):
        return [t for k in tree for t in _flat_leaves(k)]
    return []


@pytest.mark.parametrize("first", FIRSTS, ids=lambda f: "".join(map(str, f)))
def test_marked_samples_go_to_rest_and_every_other_byte_stays(HF, first):
    g = [Guarded((B, n), offset=k % 4, seed=10 + k) for k, n in enumerate(SIZES)]
    g += [Guarded((B, 3), offset=k, seed=30 + k) for k in (1, 2, 3)]              # 3 per sample at every alignment
    g += [Guarded((B, 4, 3, 5), offset=2, seed=40, channels_last=True),           # what the scans return: [B,C,H,W] over [B,H,W,C]
          Guarded((B, 4, 3, 5), offset=1, seed=41, channels_last=True),
          Guarded((B, 10), offset=3, seed=42)]
    v_leak = g[4].t
    v_leak._snn_rest = -0.375                                                     # a potential that rests at v_leak != 0
    tree = [[HF.NeuronState(g[6].t, g[7].t), None, HF.SynapseState(g[0].t)],
            [[(g[1].t, g[5].t), None], HF.NeuronState(v_leak, g[11].t), HF.SynapseState(g[2].t)],
            None,
            [HF.NeuronState(g[9].t, g[10].t), (g[3].t, g[8].t)]]
    f_dev = torch.tensor(first, dtype=torch.int32).cuda()
    out = HF.reset_state_(tree, f_dev)
    torch.cuda.synchronize()
    for k, x in enumerate(g):
        assert np.array_equal(x.got(), x.want(first, -0.375 if k == 4 else 0.0)), (k, first)
    # the tree comes back with the same nesting, its leaves the same memory, detached, the rest tag kept
    assert out[2] is None and out[0][1] is None and out[1][0][1] is None
    assert isinstance(out[0][0], HF.NeuronState) and isinstance(out[0][2], HF.SynapseState)
    assert isinstance(out[1][0][0], tuple) and isinstance(out[3], list)
    assert [t.data_ptr() for t in _flat_leaves(out)] == [t.data_ptr() for t in _flat_leaves(tree)]
    assert all(not t.requires_grad for t in _flat_leaves(out))
    assert out[1][1].v._snn_rest == -0.375


@pytest.mark.parametrize("first", ([0, 1, 0], [1, 1, 1]), ids=("010", "111"))
def test_one_tensor_alone_and_a_tree_of_many(HF, first):
    one = Guarded((B, 7), offset=1, seed=50)
    f_dev = torch.tensor(first, dtype=torch.int32).cuda()
    HF.reset_state_([one.t], f_dev)
    many = [Guarded((B, 1 + k % 9), offset=k % 4, seed=60 + k) for k in range(300)]   # 300 table rows, one launch
    HF.reset_state_([[HF.SynapseState(x.t)] for x in many], f_dev.to(torch.int64))    # (any integer type of first)
    torch.cuda.synchronize()
    assert np.array_equal(one.got(), one.want(first))
    for k, x in enumerate(many):
        assert np.array_equal(x.got(), x.want(first)), k


def test_leaves_that_require_grad_or_broadcast_and_the_refusals(HF):
    first = torch.tensor([0, 1, 0], dtype=torch.int32).cuda()
    i = torch.rand(B, 4, 3, 5, device="cuda")
    v0 = torch.tensor(0.5, device="cuda")                                          # norse's 0-dim initial potential
    w = torch.rand(B, 6, device="cuda", requires_grad=True)
    grown = (w * 2.0)                                                              # a leaf with a graph behind it
    keep_i, keep_g = i.clone(), grown.detach().clone()
    out = HF.reset_state_([HF.NeuronState(v0, i), grown], first)
    v, i2 = out[0]
    assert tuple(v.shape) == tuple(i.shape) and i2.data_ptr() == i.data_ptr()
    assert torch.equal(v[0], torch.full_like(v[0], 0.5)) and torch.equal(v[2], torch.full_like(v[2], 0.5))
    assert not v[1].any() and not i2[1].any() and torch.equal(i2[0], keep_i[0]) and torch.equal(i2[2], keep_i[2])
    assert out[1].grad_fn is None and not out[1].requires_grad
    assert not out[1][1].any() and torch.equal(out[1][0], keep_g[0]) and torch.equal(out[1][2], keep_g[2])
    assert HF.reset_state_([None, [None]], first) == [None, [None]]                # nothing to launch
    with pytest.raises(ValueError, match="float32"):
        HF.reset_state_([torch.zeros(B, 4, device="cuda", dtype=torch.float64)], first)
    with pytest.raises(ValueError, match=r"\[B = 3"):
        HF.reset_state_([torch.zeros(2, 4, device="cuda")], first)
    with pytest.raises(ValueError, match="first must be"):
        HF.reset_state_([torch.zeros(B, 4, device="cuda")], first.float())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.reset_state_([torch.zeros(B, 4)], first)
    with pytest.raises(ValueError, match="no part of a state tree"):
        HF.reset_state_([{"v": i}], first)
