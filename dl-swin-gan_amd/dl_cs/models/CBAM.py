"""CBAM 3D ResNet regularizer (MODEL_TYPE 'CBAM') of the reference's unrolledCBAM
network, MI355X build.

Same classes, constructor arguments and state_dict keys as the reference
(CBAM = dl_cs/models/CBAM.py:60-134, 371-521, 565-639).  The conv trunk is resnet3d's
gated trunk (gated_forward / gated_backward) with CbamGate below in it: the channel gate
(CABlock: the max-pool branch is commented out in the reference, CBAM:411,421) is se3d's
on the dlcs_se_* kernels, and the spatial gate (SABlock: mean over channels ->
Conv3d(1, 1, 5, padding 2), no sigmoid, no max map) runs on the dlcs_cbam_* kernels
(cbam.hip).

As in se3d.py the pre-activation ReLUs are in place (CBAM:491-494 build resnet3d's
ConvBlocks), so a block's residual adds relu(input) and every block output is only
consumed through a ReLU.  With F channels, N = Tp Y X voxels per batch item (time pad
included) and taps outside the grid reading 0:

    o   = conv_b(relu(conv_a(r_k)))
    m   = mean_v o ;  h = relu(W1 m + b1) ;  s = sigmoid(W2 h + b2)        CBAM:518
    a[b, v] = (1 / F) sum_c s[b, c] o[b, v, c]                              map
    q[b, v] = b5 + sum_d w5[d] a[b, v + d]                                  map, CBAM:519
    r_{k+1} = relu(q[b, v] s[b, c] o[b, v, c] + r_k)                        CBAM:521 + the next ReLU

Backward of one block from g = dL/dr_{k+1}, gz = g [r_{k+1} > 0] (also the residual
gradient into r_k):

    dq[b, v] = sum_c gz s[b, c] o[b, v, c]
    db5 += sum dq ;  dw5[d] += sum_{b, v} dq[b, v] a[b, v + d]
    da[b, v] = sum_d w5[d] dq[b, v - d]
    e = gz q[b, v] + da[b, v] / F ;  ds[b, c] = sum_v e o  -> se_gate_bwd -> dm[b, c]
    do = e s[b, c] + dm[b, c]                               conv_b's output gradient
"""
from functools import partial

from torch import nn

from . import _ops as K
from .resnet3d import _TrunkNet, _wb, gated_backward, gated_forward
from .se3d import SeGate
from .swin3D import Activation, ConvBlock, Conv3d

_FUSED = "dl_cs: runs inside CBAMResNet's fused HIP node"


def _pool_type(type):
    if type not in ('channel', 'spatial'):
        raise ValueError('Invalid type')
    return type


class GlobalMaxPool(nn.Module):
    """CBAM:60-87 -- max over (T, Y, X) ('channel') or over channels ('spatial'); the
    reference constructs it and never calls it."""

    def __init__(self, type):
        super().__init__()
        self.mpool = nn.Identity()
        self.type = _pool_type(type)

    def forward(self, input):
        raise NotImplementedError("dl_cs HIP CBAMResNet: the max-pool branches are disabled in the reference")


class GlobalAvgPool(nn.Module):
    """CBAM:90-117 -- mean over (T, Y, X) ('channel') or over channels ('spatial')."""

    def __init__(self, type):
        super().__init__()
        self.apool = nn.Identity()
        self.type = _pool_type(type)

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class FC(nn.Module):
    """CBAM:120-134 -- nn.Linear."""

    def __init__(self, in_chans, out_chans):
        super().__init__()
        self.fc = nn.Linear(in_chans, out_chans)

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class CABlock(nn.Module):
    """CBAM:371-422 -- GlobalAvgPool -> FC(out_chans, rr) -> ReLU -> FC(rr, out_chans) -> sigmoid."""

    def __init__(self, out_chans, rr, norm_type='none', is_complex=False):
        super().__init__()
        if is_complex:
            raise NotImplementedError("dl_cs HIP CBAMResNet: COMPLEX: False")
        self.is_complex = is_complex
        self.layers = nn.Sequential(FC(out_chans, rr), Activation("relu"), FC(rr, out_chans), Activation("sigmoid"))
        self.avgpool = nn.Sequential(GlobalAvgPool("channel"))

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class SABlock(nn.Module):
    """CBAM:425-475 -- mean over channels -> Conv3d(1, 1, kernel_size=5, padding=2)."""

    def __init__(self, act_type='relu', norm_type='none', is_complex=False):
        super().__init__()
        if is_complex:
            raise NotImplementedError("dl_cs HIP CBAMResNet: COMPLEX: False")
        self.is_complex = is_complex
        self.avgpool = nn.Sequential(GlobalAvgPool("spatial"))
        self.layers = nn.Sequential(Conv3d(in_chans=1, out_chans=1, kernel_size=5))

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class CBAMResBlock(nn.Module):
    """CBAM:477-521 -- two pre-activation ConvBlocks scaled by the channel gate, then by
    the spatial map of the scaled tensor, plus the residual."""

    def __init__(self, chans, kernel_size, rr, act_type='relu', is_complex=False):
        super().__init__()
        self.layers1 = nn.Sequential(
            ConvBlock(chans, chans, kernel_size, act_type=act_type, is_complex=is_complex),
            ConvBlock(chans, chans, kernel_size, act_type=act_type, is_complex=is_complex))
        self.CAmodule = nn.Sequential(CABlock(chans, rr, is_complex=is_complex))
        self.SAmodule = nn.Sequential(SABlock(is_complex=is_complex))

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class CbamGate:
    """The gate of one CBAMResBlock for resnet3d's gated trunk: w = (W1, b1, W2, b2, w5, b5)
    and gw their gradients, saved = (m, h, s, a, q); the equations are in the module docstring."""

    @staticmethod
    def fwd(o, r_prev, w, grid, F, N):
        w1, b1, w2, b2, w5, b5 = w
        m = SeGate.pool(o, grid, F, N)
        h, s = K.se_gate(m, w1, b1, w2, b2)
        a = K.cbam_chan_mean(o, s, grid, F)
        q = K.cbam_stencil5(a, w5, b5, grid)
        return K.cbam_scale_res_relu(o, s, q, r_prev, grid, F), (m, h, s, a, q)

    @staticmethod
    def bwd(g, r_next, o, saved, w, gw, grid, F, N):
        (m, h, s, a, q), (w1, _, w2, _, w5, _) = saved, w
        gw1, gb1, gw2, gb2, gw5, gb5 = gw
        dq = K.cbam_bwd_rowdot(g, r_next, o, s, grid, F)
        K.cbam_stencil5_wgrad(dq, a, grid, gw5, gb5)
        da = K.cbam_stencil5(dq, w5, None, grid, transposed=True)
        ds = K.cbam_bwd_reduce(g, r_next, o, q, da, grid, F)
        dm = K.se_gate_bwd(ds, s, h, m, w1, w2, 1.0 / N, gw1, gb1, gw2, gb2)
        return K.cbam_bwd_apply(g, r_next, s, q, da, dm, grid, F)                   # g is now gz


class CBAMResNet(_TrunkNet):
    """CBAM:565-639 -- init ConvBlock (no activation), num_resblocks CBAMResBlocks,
    final pre-activation ConvBlock back to in_chans, plus the input residual."""
    NAME, CONFIG, BLOCK, BLOCKS = "CBAMResNet", "configs/config_cbam.yaml", CBAMResBlock, "se_res_blocks"
    TRUNK = (partial(gated_forward, gate=CbamGate), partial(gated_backward, gate=CbamGate))

    def __init__(self, num_resblocks, in_chans, chans, kernel_size, rr, act_type='relu', use_complex_layers=False,
                 circular_pad=True):
        super().__init__(num_resblocks, in_chans, chans, kernel_size, act_type, use_complex_layers, circular_pad, rr)

    def _block_keys(self, b):
        return (self.c(f"{b}.layers1.0") + self.c(f"{b}.layers1.1") + _wb(f"{b}.CAmodule.0.layers.0.fc") +
                _wb(f"{b}.CAmodule.0.layers.2.fc") + _wb(f"{b}.SAmodule.0.layers.0.conv"))

