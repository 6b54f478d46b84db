"""1-D ResNet on the temporal basis R of the DSLR family (r1d = dl_cs/models/resnet1d.py),
MI355X build.

Same classes, constructor arguments and state_dict keys as the reference (r1d:108-271);
the network of resnet2d.py with Conv1d weights and the circular time pad of r1d:225-248:

    u   = circular_pad(cat(re, im), pad_size)        pad_size = 2 num_resblocks + 2
    out = crop(conv_f(r_L) + u, pad_size)

It runs on the same fused node (resnet2d.embedded_forward / embedded_backward): the N
sequences [N, C, T'] are laid out as the (depth, height) positions of one
(1, N / 4, 4, T') grid, time along W, and every 3-tap weight sits in the centre depth
and centre height tap of a 27-tap weight, so sequences do not mix.  The W border is the
conv's own zero padding only if the grid is not padded along W: T' = T + 2 pad_size
must be a multiple of 4 (NotImplementedError otherwise).

Compute dtype bf16 runs resnet2d's plane node with KH = 1: the N sequences are the rows
[N T', ld] themselves, 3 taps along time, any T' <= 256 and no padding of N.
"""
import torch
from torch import nn

from . import resnet2d as r2d


class ConvBlock(r2d.ConvBlock):
    """r1d:108-156 -- Norm -> Act -> Conv1d (pre-activation)."""
    NAME, CONV = 'Conv1D', nn.Conv1d


class ResBlock(r2d.ResBlock):
    """r1d:159-195."""
    BLOCK = ConvBlock


def _embed_w(w):
    """[cout, cin, 3] -> [cout, cin, 3, 3, 3] with the weight in the centre depth and height taps."""
    w3 = torch.zeros(w.shape[:2] + (3, 3, 3), dtype=w.dtype, device=w.device)
    w3[:, :, 1, 1] = w
    return w3


class ResNet(r2d.ResNet):
    """r1d:198-271 -- the 1-D ResNet: complex [N, C, T] -> the same shape."""
    NAME, BLOCK, RES = "ResNet1D", ConvBlock, ResBlock
    EMBED = staticmethod(_embed_w)
    CENTRE = staticmethod(lambda g3: g3[:, :, 1, 1])
    KH = 1

    def forward(self, input):
        N, C, T = input.shape
        if not self.circular_pad:
            raise NotImplementedError("dl_cs HIP ResNet1D: CIRCULAR_PAD: True (configs/config_dslr.yaml)")
        pad = self.pad_size
        Tp = T + 2 * pad
        if r2d.get_compute_dtype() == torch.bfloat16:
            u = torch.cat((input.real, input.imag), dim=1)
            u = nn.functional.pad(u, (pad, pad), mode='circular')
            o = self._run(u.unsqueeze(2))[:, :, 0, pad:Tp - pad]
            return torch.complex(o[:, :C].contiguous(), o[:, C:].contiguous())
        if Tp % 4:
            raise NotImplementedError(f"dl_cs HIP ResNet1D: T + 2 pad_size = {Tp} must be a multiple of 4 (the conv grid)")
        u = torch.cat((input.real, input.imag), dim=1)                              # r1d:225-229
        u = nn.functional.pad(u, (pad, pad), mode='circular')                       # r1d:231-234
        N16 = (N + 15) // 16 * 16
        x = nn.functional.pad(u, (0, 0, 0, 0, 0, N16 - N))                          # whole 4 x 4 (depth, height) patches
        x = x.permute(1, 0, 2).reshape(1, 2 * C, N16 // 4, 4, Tp)
        o = self._run(x).reshape(2 * C, N16, Tp)[:, :N, pad:Tp - pad].permute(1, 0, 2)      # r1d:238-240
        return torch.complex(o[:, :C].contiguous(), o[:, C:].contiguous())          # r1d:242-248
