"""Unrolled reconstruction networks with the CBAM ResNet regularizer
(MODEL_TYPE 'CBAM', configs/config_cbam.yaml), MI355X build.

Same classes, config keys and state_dict schema as the reference
(ucb = dl_cs/models/unrolledCBAM.py:15-168): unrolled.py's keys plus RR, the hidden
width of the channel gate.  The data-consistency steps are the Swin path's (the fused
SENSE normal operator for PGD, ucb:87-118, and the device-resident conjugate
gradient for HQS, ucb:135-168); the regularizer is CBAM.CBAMResNet.
"""
import torch
from torch import nn

from .CBAM import CBAMResNet
from . import unrolledswin as _us


class UnrolledCBAMResNet(nn.Module):
    """ucb:15-70 -- abstract unrolled network with CBAMResNet regularizers."""

    def __init__(self, config):
        super().__init__()
        P = config.MODEL.PARAMETERS
        self.num_unrolls = P.NUM_UNROLLS
        self.num_resblocks = P.NUM_RESBLOCKS
        self.rr = P.RR
        self.num_features = P.NUM_FEATURES
        self.kernel_size = P.CONV_BLOCK.KERNEL_SIZE[0]
        self.num_emaps = P.NUM_EMAPS
        self.share_weights = P.SHARE_WEIGHTS
        self.fix_step_size = P.FIX_STEP_SIZE
        self.use_complex_layers = P.CONV_BLOCK.COMPLEX
        self.circular_pad = P.CONV_BLOCK.CIRCULAR_PAD
        self.do_checkpoint = P.GRAD_CHECKPOINT
        self.cnn_update = self.init_nets()

    def init_nets(self):
        """ucb:38-64"""
        in_chans = self.num_emaps if self.use_complex_layers else 2 * self.num_emaps
        params = dict(in_chans=in_chans, chans=self.num_features, num_resblocks=self.num_resblocks,
                      use_complex_layers=self.use_complex_layers, kernel_size=self.kernel_size,
                      circular_pad=self.circular_pad, rr=self.rr)
        if self.share_weights:
            return nn.ModuleList([CBAMResNet(**params)] * self.num_unrolls)
        return nn.ModuleList([CBAMResNet(**params) for _ in range(self.num_unrolls)])

    def forward(self, y, A, x0=None):
        raise NotImplementedError


class ProximalGradientDescent(UnrolledCBAMResNet):
    """ucb:73-118 -- x <- R_i(x + s (A^H A x - A^H y)), s = -2 (learnable unless FIX_STEP_SIZE)."""

    def __init__(self, config):
        super().__init__(config)
        self.step_size = nn.Parameter(torch.tensor([-2.0], dtype=torch.float32),
                                      requires_grad=(not self.fix_step_size))

    forward = _us.ProximalGradientDescent.forward


class HalfQuadraticSplitting(UnrolledCBAMResNet):
    """ucb:121-168 -- z = R_i(x); x <- CG(A^H A + lamda I, A^H y + lamda z)."""

    def __init__(self, config):
        super().__init__(config)
        self.num_cg_iter = config.MODEL.PARAMETERS.MODL.NUM_CG_STEPS
        self.lamda = nn.Parameter(torch.tensor([0.1], dtype=torch.float32),
                                  requires_grad=(not self.fix_step_size))

    _normal = _us.HalfQuadraticSplitting._normal
    forward = _us.HalfQuadraticSplitting.forward
