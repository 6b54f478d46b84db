"""Unrolled reconstruction networks with the CBAM ResNet regularizer
(MODEL_TYPE 'CBAM', configs/config_cbam.yaml), MI355X build.

Same classes, config keys and state_dict schema as the reference
(ucb = dl_cs/models/unrolledCBAM.py:15-168): unrolled.py's keys plus RR, the hidden
width of the channel gate.  The data-consistency steps are the Swin path's (the fused
SENSE normal operator for PGD, ucb:87-118, and the device-resident conjugate
gradient for HQS, ucb:135-168); the regularizer is CBAM.CBAMResNet.
"""
from .CBAM import CBAMResNet
from . import unrolled as _ur, unrolledswin as _us


class UnrolledCBAMResNet(_ur.UnrolledNet):
    """ucb:15-70 -- abstract unrolled network with CBAMResNet regularizers (self.rr = RR)."""
    NET = CBAMResNet
    EXTRA = {"rr": "RR"}


class ProximalGradientDescent(_us.PGDSteps, UnrolledCBAMResNet):
    """ucb:73-118"""


class HalfQuadraticSplitting(_us.HQSSteps, UnrolledCBAMResNet):
    """ucb:121-168"""
