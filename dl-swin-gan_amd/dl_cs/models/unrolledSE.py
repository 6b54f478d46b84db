"""Unrolled reconstruction networks with the squeeze-excitation ResNet regularizer
(MODEL_TYPE 'SE', configs/config_se.yaml), MI355X build.

Same classes, config keys and state_dict schema as the reference
(use = dl_cs/models/unrolledSE.py:15-168): unrolled.py's keys plus RR, the hidden
width of the SE gate.  The data-consistency steps are the Swin path's (the fused
SENSE normal operator for PGD, use:87-118, and the device-resident conjugate
gradient for HQS, use:135-168); the regularizer is se3d.SeResNet.
"""
from .se3d import SeResNet
from . import unrolled as _ur, unrolledswin as _us


class UnrolledSeResNet(_ur.UnrolledNet):
    """use:15-70 -- abstract unrolled network with SeResNet regularizers (self.rr = RR)."""
    NET = SeResNet
    EXTRA = {"rr": "RR"}


class ProximalGradientDescent(_us.PGDSteps, UnrolledSeResNet):
    """use:73-118"""


class HalfQuadraticSplitting(_us.HQSSteps, UnrolledSeResNet):
    """use:121-168"""
