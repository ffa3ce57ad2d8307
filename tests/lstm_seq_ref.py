"""fp64 CPU restatement of a ConvLSTM over a sequence: autograd over ``oracle.net.ConvLSTM`` cast to double, stepped over
``t`` as the reference's time loop does.  Shared by the whole-sequence scan tests (tests/test_gpu_lstm_seq.py)."""
from typing import Dict, Optional, Tuple

import torch

from oracle import net as ON


def conv_lstm_fp64(x: torch.Tensor, weight: torch.Tensor, state: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                   gh: Optional[torch.Tensor] = None, ghT: Optional[torch.Tensor] = None,
                   gcT: Optional[torch.Tensor] = None, *, x_grad: bool = True, weight_grad: bool = True,
                   state_grad: bool = True) -> Dict[str, Optional[torch.Tensor]]:
    """``x [T,B,Cin,H,W]``, ``weight [4Ch,Cin+Ch,1,1]``, ``state = (h0, c0)`` or None; the loss is
    ``sum(hs * gh) + sum(h_T * ghT) + sum(c_T * gcT)`` over the terms given.  Returns fp64 ``hs``, ``c_T``, ``dx``, ``dw``,
    ``dh0`` and ``dc0`` (the last two None without a state).  ``x_grad`` / ``weight_grad`` / ``state_grad``: which of the
    three require a gradient (default: all); the gradients of the others come back None, and with none of them nothing
    is differentiated."""
    Ch = weight.shape[0] // 4
    cell = ON.ConvLSTM(x.shape[2], Ch).double()
    with torch.no_grad():
        cell.conv.weight.copy_(weight.detach().double().cpu())
    cell.conv.weight.requires_grad_(weight_grad)
    x64 = x.detach().double().cpu().requires_grad_(x_grad)
    st = None
    if state is not None:
        st = tuple(s.detach().double().cpu().requires_grad_(state_grad) for s in state)
    cur, outs = st, []
    for t in range(x64.shape[0]):
        h, cur = cell(x64[t], cur)
        outs.append(h)
    hs = torch.stack(outs)
    loss = hs.sum() * 0.0
    for out, g in ((hs, gh), (cur[0], ghT), (cur[1], gcT)):
        if g is not None:
            loss = loss + (out * g.detach().double().cpu()).sum()
    if loss.requires_grad:
        loss.backward()
    return {"hs": hs.detach(), "c_T": cur[1].detach(), "dx": x64.grad, "dw": cell.conv.weight.grad,
            "dh0": None if st is None else st[0].grad, "dc0": None if st is None else st[1].grad}
