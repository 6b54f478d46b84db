"""Inference entry point for the CBAM-ResNet-unrolled model on MI355X: BART CFL
k-space in, CFL images out.  scripts/reconstruct.py's command line, file handling and
main, with this file's build_model, which maps MODEL_TYPE 'CBAM'
(configs/config_cbam.yaml) to dl_cs.models.unrolledCBAM and refuses every other type
(the reference reconstructs CBAM through reconstruct_h5.py --model CBAM; H5 input is
not built for this family).
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import reconstruct  # noqa: E402
from reconstruct import create_arg_parser, logger  # noqa: E402,F401


def build_model(config):
    from dl_cs.models import unrolledCBAM
    if config.MODEL.MODEL_TYPE != 'CBAM':
        raise NotImplementedError(f"MODEL_TYPE {config.MODEL.MODEL_TYPE}: reconstruct_cbam.py builds CBAM only")
    if config.MODEL.META_ARCHITECTURE == 'dlespirit':
        return unrolledCBAM.ProximalGradientDescent(config)
    if config.MODEL.META_ARCHITECTURE == 'modl':
        return unrolledCBAM.HalfQuadraticSplitting(config)
    raise ValueError('Meta architecture in config file not recognized!')


def main(args):
    reconstruct.main(args, builder=build_model)


if __name__ == '__main__':
    a = create_arg_parser().parse_args(sys.argv[1:])
    t0 = time.time()
    main(a)
    logger.info('Script complete.')
    logger.info(f'Elapsed time (total): {time.time() - t0} s')
