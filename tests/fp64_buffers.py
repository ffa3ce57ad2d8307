"""Guarded device buffers and operand generators shared by the per-element fp64 tests of the convolution kernels
(test_gpu_halo_fp64.py, test_gpu_gemm_fp64.py)."""
import torch

SENT = 77.0          # guard channels / pixels around every slice
GUARD = 4            # guard pixels at each end of a buffer
V_TH = 1.0
BF16_ROUND = 2.0 ** -8   # one bf16 rounding of the stored result (SBF)


# fields of snn_conv2d_gather_plan's out[17] and snn_conv2d_wgrad_plan's out[18] (include/snn_hip.h)
GATHER_KEYS = ("ok loader bn out_vec mtiles mtiles_per_xcd ntiles blocks idle nkh nkw ktot ohc owc nphases bn_chunks "
               "bn_rows").split()
WGRAD_PLAN_KEYS = ("ok kernel tile bm bn tiles_m tiles_n stage splitk pps last_pix empty reducer kg groups per rblocks "
                   "grid").split()


def _st():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """[N,H,W,C] channels-last = channels off .. off+C of a [GUARD + N*H*W + GUARD, ld] buffer of SENT."""

    def __init__(self, shape, off=0, ld=None, values=None, fill=None, dtype=torch.float32):
        N, H, W, C = shape
        ld = C if ld is None else ld
        P = N * H * W
        self.shape, self.ld = tuple(shape), ld
        self.buf = torch.full((P + 2 * GUARD, ld), SENT, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + P, off:off + C]
        if values is not None:
            self.view.copy_(values.reshape(P, C))
        elif fill is not None:
            self.view.fill_(fill)
        self.ptr = self.view.data_ptr()
        self.mask = torch.zeros(self.buf.shape, dtype=torch.bool, device="cuda")
        self.mask[GUARD:GUARD + P, off:off + C] = True
        self.before = self.buf.clone()

    def value(self):
        return self.view.double().cpu().reshape(self.shape)

    def guards_intact(self, whole=False):
        it = torch.int32 if self.buf.dtype == torch.float32 else torch.int16
        keep = torch.ones_like(self.mask) if whole else ~self.mask
        return torch.equal(self.buf.view(it)[keep], self.before.view(it)[keep])


def _exact_operands(shape, seed, spikes=False, lim=4):
    g = torch.Generator().manual_seed(seed)
    if spikes:
        return torch.randint(0, 2, shape, generator=g).float()
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def _exact_weights(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-31, 32, shape, generator=g).float() * 2.0 ** -6


def _random(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale
