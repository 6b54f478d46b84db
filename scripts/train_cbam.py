"""Training entry point of the CBAM-ResNet-unrolled cine reconstruction on MI355X:
the reference's scripts/train_cbam.py by name.  The trainer is scripts/train_swin.py
(same command line and training semantics) with this file's build_model, which maps
MODEL_TYPE 'CBAM' (configs/config_cbam.yaml) to dl_cs.models.unrolledCBAM and
refuses every other type (those train through train_swin.py / train_se.py).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import train_swin  # noqa: E402
from train_swin import create_arg_parser  # noqa: E402,F401


def build_model(config):
    from dl_cs.models import unrolledCBAM
    if config.MODEL.MODEL_TYPE.upper() != 'CBAM':
        raise NotImplementedError(f"MODEL_TYPE {config.MODEL.MODEL_TYPE}: train_cbam.py builds CBAM only")
    arch = config.MODEL.META_ARCHITECTURE
    if arch == 'dlespirit':
        return unrolledCBAM.ProximalGradientDescent(config)
    if arch == 'modl':
        return unrolledCBAM.HalfQuadraticSplitting(config)
    raise ValueError('Meta architecture in config file not recognized!')


def main(argv=None):
    train_swin.main(argv, builder=build_model)


if __name__ == "__main__":
    main()
