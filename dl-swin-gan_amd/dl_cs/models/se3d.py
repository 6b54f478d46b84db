"""Squeeze-excitation 3D ResNet regularizer (MODEL_TYPE 'SE') of the reference's
unrolledSE network, MI355X build.

Same classes, constructor arguments and state_dict keys as the reference
(se3d = dl_cs/models/se3d.py:302-515).  The conv trunk is resnet3d's gated trunk
(gated_forward / gated_backward: the same generic Conv3d k3 kernels, patch-blocked
channels-last rows); in it the per-(batch item, channel) gate, SeGate below, runs on
the dlcs_se_* kernels (se.hip).

As in resnet3d.py the pre-activation ReLUs are in place (se3d:416-417 build the
ConvBlocks of resnet3d), so a block's residual adds relu(input) and every block
output is only ever consumed through a ReLU; the HIP forward stores r = relu(.)
directly.  With N = Tp Y X voxels per batch item (time pad included; on a grid that
the trunk pads to multiples of 4 still the true grid's count, the added rows hold
zeros), R = rr the hidden width (se3d:325 passes rr straight to FC(out_chans, rr)):

    u   = pre(x)                                cat(re, im), circular T pad
    r0  = relu(conv0(u))
    t_k = relu(conv_a(r_k))
    o_k = conv_b(t_k)                           bias, no ReLU
    m_k = mean over voxels of o_k               GlobalAvgPool (se3d:92)
    h_k = relu(W1 m_k + b1);  s_k = sigmoid(W2 h_k + b2)
    r_{k+1} = relu(s_k o_k + r_k)               se3d:435-438 + the next in-place ReLU
    out = conv_f(r_L) + u ;  x' = post(out)

Backward of one block from g = dL/dr_{k+1}:

    gz = g [r_{k+1} > 0]                        also the residual gradient into r_k
    ds = sum over voxels of gz o_k
    dz2 = ds s (1 - s);  dW2 += dz2^T h;  db2 += sum_b dz2
    dh = (dz2 W2) [h > 0];  dW1 += dh^T m;  db1 += sum_b dh;  dm = dh W1
    do_k = gz s + dm / N                        conv_b's output gradient
"""
from functools import partial

from torch import nn

from . import _ops as K
from .resnet3d import _TrunkNet, _wb, gated_backward, gated_forward
from .swin3D import Activation, ConvBlock

_FUSED = "dl_cs: runs inside SeResNet's fused HIP node"


class GlobalAvgPool(nn.Module):
    """se3d:80-97 -- mean over (T, Y, X) of each channel."""

    def __init__(self):
        super().__init__()
        self.gpool = nn.Identity()

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class FC(nn.Module):
    """se3d:100-114 -- nn.Linear."""

    def __init__(self, in_chans, out_chans):
        super().__init__()
        self.fc = nn.Linear(in_chans, out_chans)

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class SeBlock(nn.Module):
    """se3d:302-348 -- GlobalAvgPool -> FC(out_chans, rr) -> ReLU -> FC(rr, out_chans) -> sigmoid."""

    def __init__(self, out_chans, rr, norm_type='none', is_complex=False):
        super().__init__()
        if is_complex:
            raise NotImplementedError("dl_cs HIP SeResNet: COMPLEX: False")
        self.is_complex = is_complex
        self.layers = nn.Sequential(GlobalAvgPool(), FC(out_chans, rr), Activation("relu"), FC(rr, out_chans),
                                    Activation("sigmoid"))

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class SeResBlock(nn.Module):
    """se3d:401-438 -- two pre-activation ConvBlocks scaled by a SeBlock's gate, plus the residual."""

    def __init__(self, chans, kernel_size, rr, act_type='relu', is_complex=False):
        super().__init__()
        self.layers1 = nn.Sequential(
            ConvBlock(chans, chans, kernel_size, act_type=act_type, is_complex=is_complex),
            ConvBlock(chans, chans, kernel_size, act_type=act_type, is_complex=is_complex))
        self.layers2 = SeBlock(chans, rr, is_complex=is_complex)

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class SeGate:
    """The gate of one SeResBlock for resnet3d's gated trunk: w = (W1, b1, W2, b2) and
    gw their gradients, saved = (m, h, s); the equations are in the module docstring."""

    @staticmethod
    def pool(o, grid, F, N):
        """m [B, F] = the mean of o over a batch item's N voxels; o is zero on the rows of a
        padded grid that lie outside them, so the mean over all rows is rescaled."""
        rows = grid[1] * grid[2] * grid[3]
        m = K.se_pool(o, grid[0], rows, F)
        return m if rows == N else K.scaled_copy(m, m.dtype, rows / N)

    @staticmethod
    def fwd(o, r_prev, w, grid, F, N):
        B, rows = grid[0], grid[1] * grid[2] * grid[3]
        m = SeGate.pool(o, grid, F, N)
        h, s = K.se_gate(m, *w)
        return K.se_scale_res_relu(o, s, r_prev, B, rows, F), (m, h, s)

    @staticmethod
    def bwd(g, r_next, o, saved, w, gw, grid, F, N):
        B, rows = grid[0], grid[1] * grid[2] * grid[3]
        (m, h, s), (w1, _, w2, _) = saved, w
        ds = K.se_bwd_reduce(g, r_next, o, B, rows, F)
        dm = K.se_gate_bwd(ds, s, h, m, w1, w2, 1.0 / N, *gw)
        return K.se_bwd_apply(g, r_next, s, dm, B, rows, F)                         # g is now gz


class SeResNet(_TrunkNet):
    """se3d:441-515 -- init ConvBlock (no activation), num_resblocks SeResBlocks,
    final pre-activation ConvBlock back to in_chans, plus the input residual."""
    NAME, CONFIG, BLOCK, BLOCKS = "SeResNet", "configs/config_se.yaml", SeResBlock, "se_res_blocks"
    TRUNK = (partial(gated_forward, gate=SeGate), partial(gated_backward, gate=SeGate))

    def __init__(self, num_resblocks, in_chans, chans, kernel_size, rr, act_type='relu', use_complex_layers=False,
                 circular_pad=True):
        super().__init__(num_resblocks, in_chans, chans, kernel_size, act_type, use_complex_layers, circular_pad, rr)

    def _block_keys(self, b):
        return (self.c(f"{b}.layers1.0") + self.c(f"{b}.layers1.1") +
                _wb(f"{b}.layers2.layers.1.fc") + _wb(f"{b}.layers2.layers.3.fc"))

