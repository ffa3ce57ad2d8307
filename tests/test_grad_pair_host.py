"""``functional._grad_pair``: where the two gradients of (gamma, bias) / (w_mem, w_syn) go.  The rules, from the code it
replaced in ``_AffineNeuron.backward``: the pair goes into GradSlots only when every NEEDED member has one; the shared
accumulate flag is the first present slot's ``written`` before the claim; both slots are claimed even if one gradient
is needed.  Otherwise fresh tensors for the needed members (flag 0, slots untouched); nothing at all when none is needed."""
import itertools

import pytest
import torch

# (slot a present, slot b present, a needed, b needed) -> where the pair goes; written out by hand
WHERE = {
    (0, 0, 0, 0): "none", (0, 0, 0, 1): "fresh", (0, 0, 1, 0): "fresh", (0, 0, 1, 1): "fresh",
    (0, 1, 0, 0): "none", (0, 1, 0, 1): "slots", (0, 1, 1, 0): "fresh", (0, 1, 1, 1): "fresh",
    (1, 0, 0, 0): "none", (1, 0, 0, 1): "fresh", (1, 0, 1, 0): "slots", (1, 0, 1, 1): "fresh",
    (1, 1, 0, 0): "none", (1, 1, 0, 1): "slots", (1, 1, 1, 0): "slots", (1, 1, 1, 1): "slots",
}


@pytest.mark.parametrize("first_written", (False, True))
@pytest.mark.parametrize("key", sorted(WHERE))
def test_grad_pair(key, first_written):
    from snn_for_object_detection_amd import functional as HF
    has_a, has_b, need_a, need_b = key
    n, dev = 5, torch.device("cpu")
    a = HF.GradSlot(torch.zeros(n)) if has_a else None
    b = HF.GradSlot(torch.zeros(n)) if has_b else None
    if a is not None:
        a.written = first_written
    if b is not None:
        b.written = not first_written      # the flag must come from the FIRST present slot
    before = [None if s is None else s.written for s in (a, b)]
    pa, pb, acc, fa, fb = HF._grad_pair((a, b), (bool(need_a), bool(need_b)), n, dev)
    where = WHERE[key]
    if where == "none":
        assert (pa, pb, acc, fa, fb) == (None, None, 0, None, None)
        assert [None if s is None else s.written for s in (a, b)] == before          # nothing claimed
    elif where == "slots":
        assert fa is None and fb is None
        assert pa == (a.buf.data_ptr() if need_a else None)
        assert pb == (b.buf.data_ptr() if need_b else None)
        assert acc == int(first_written if has_a else not first_written)
        assert all(s.written for s in (a, b) if s is not None)                        # both claimed
    else:
        assert acc == 0
        assert [None if s is None else s.written for s in (a, b)] == before          # slots untouched
        for need, f, p in ((need_a, fa, pa), (need_b, fb, pb)):
            if need:
                assert f.shape == (n,) and f.dtype == torch.float32 and p == f.data_ptr()
            else:
                assert f is None and p is None


def test_the_table_is_complete():
    assert set(WHERE) == set(itertools.product((0, 1), repeat=4))
