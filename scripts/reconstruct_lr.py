"""Inference entry point of the DSLR family (deep subspace learning on locally low-rank
blocks) on MI355X: BART CFL k-space in, CFL images out -- the reference's
scripts/reconstruct_lr.py by name and command line, plus --dtype as scripts/reconstruct.py.

scripts/reconstruct.py's file handling (CflDataset: one example per (echo, slice), echo
major; output [x, y, sl, 1, emap, echo, 1, phase]) with the three things reconstruct_lr.py
changes:

  * model: train_lr.ARCHS by META_ARCHITECTURE ('dslr-cg-v2' builds AltMinCGv1, as the
    reference's LitUnrolled does), loaded through dl_cs.checkpoint;
  * transform: the inference preprocessing of dl_cs.data.preprocess.DataTransform on the GPU
    (mask from the data, fftmod, 95th-percentile scale of the time-averaged adjoint,
    sliding-window initial image when SLWIN_INIT), then lowrank.Decompose of the initial image
    into the block factors L_init, R_init: the truncated SVD runs on the host, or with
    --svd device on the GPU (dlcs_lr_decompose; use the setting the checkpoint was trained with);
  * forward: model(y, A=SenseModel(maps, weights=mask), BlockOp=ArrayToBlocks(block size,
    image shape), L0, R0) under no_grad, one ArrayToBlocks per image shape; the images are
    rescaled by the transform's scale.

The block operators take one image: --batch-size above 1 and --multi-gpu raise
NotImplementedError.  --dtype bf16 runs the two CNNs on the plane conv (resnet2d.py); CG, the
block operators and the SENSE model stay fp32.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import reconstruct  # noqa: E402
from reconstruct import CflDataset, logger  # noqa: E402,F401
import train_lr  # noqa: E402

from dl_cs import checkpoint  # noqa: E402
from dl_cs.config import load_cfg  # noqa: E402


def create_arg_parser():
    """reconstruct.py's command line plus --svd."""
    parser = reconstruct.create_arg_parser()
    parser.add_argument('--svd', choices=['host', 'device'], default='host',
                        help='factor the initial image on the host (torch.linalg.svd) or on the GPU (block SVD kernel)')
    return parser


class LrTransform:
    """reconstruct_lr.py's DataTransform: (kspace, maps, mask, L_init, R_init, scale) of one
    example, kspace [C, T, Y, X] and maps [E, C, 1, Y, X] as CflDataset yields them."""

    def __init__(self, config, device, svd='host'):
        from dl_cs.data.preprocess import DataTransform
        self.svd = svd
        D = config.MODEL.PARAMETERS.DSLR
        self.block_size, self.num_basis, self.overlapping = D.BLOCK_SIZE, D.NUM_BASIS, D.OVERLAPPING
        self.base = DataTransform(config, device=device)
        self._decompose = {}

    def decompose(self, shape):
        """lowrank.Decompose of an image shape, built once per shape."""
        from dl_cs.mri import lowrank
        if shape not in self._decompose:
            self._decompose[shape] = lowrank.Decompose(self.block_size, self.num_basis, list(shape),
                                                       overlapping=self.overlapping, svd=self.svd)
        return self._decompose[shape]

    def __call__(self, kspace, maps):
        kspace, maps, mask, init, scale = self.base(kspace, maps)
        init = init.unsqueeze(0)                                            # [1, E, T, Y, X]
        L_init, R_init = self.decompose(tuple(init.shape))(init)
        return kspace, maps, mask, L_init, R_init, scale


def run(model, transform, dataset, block_size, overlapping, device):
    """Every example through the model, one at a time -> [n_examples, emap, phase, y, x]."""
    from dl_cs.mri import lowrank, transforms as T
    block_ops = {}
    out = []
    with torch.cuda.device(device), torch.no_grad():
        for i in range(len(dataset)):
            kspace, maps, mask, L_init, R_init, scale = transform(*dataset[i])
            shape = (1, maps.shape[0]) + tuple(kspace.shape[1:])            # [1, E, T, Y, X]
            if shape not in block_ops:
                block_ops[shape] = lowrank.ArrayToBlocks(block_size, list(shape), overlapping=overlapping).to(device)
            images = model(y=kspace.unsqueeze(0), A=T.SenseModel(maps.unsqueeze(0), weights=mask.unsqueeze(0)),
                           BlockOp=block_ops[shape], L0=L_init, R0=R_init)
            out.append((scale * images)[0])
    return np.stack([im.cpu().numpy() for im in out])


def main(args):
    from dl_cs.models import swin3D
    if args.batch_size != 1:
        raise NotImplementedError("DSLR: --batch-size 1 (the block operators take one image)")
    if args.multi_gpu:
        raise NotImplementedError("DSLR: one GPU (--device N); the block operators take one image, so there is "
                                  "no batch to spread over devices")
    if args.device < 0:
        raise RuntimeError("the DSLR networks run on the GPU (HIP kernels): pass --device N")
    swin3D.set_compute_dtype(torch.bfloat16 if args.dtype == 'bf16' else torch.float32)
    device = torch.device('cuda', args.device)
    logger.info(f'Running on GPU device #{args.device}...')
    logger.info(f'Loading model {args.ckpt}...')
    config = load_cfg(args.config_file)
    model = train_lr.build_model(config)
    checkpoint.load_model(model, args.ckpt)
    model.eval()
    for p in model.parameters():                                            # freeze()
        p.requires_grad_(False)
    model = model.to(device)
    logger.info('Loading CFL data...')
    data = CflDataset(os.path.join(args.directory, args.kspace), os.path.join(args.directory, args.maps))
    logger.info('Running inference...')
    start = time.time()
    D = config.MODEL.PARAMETERS.DSLR
    images = run(model, LrTransform(config, device, svd=getattr(args, 'svd', 'host')), data, D.BLOCK_SIZE, D.OVERLAPPING, device)
    logger.info(f'Elapsed time (reconstruction): {time.time() - start} s')
    logger.info('Writing images...')
    data.write(os.path.join(args.directory, args.out), images)


if __name__ == '__main__':
    a = create_arg_parser().parse_args(sys.argv[1:])
    t0 = time.time()
    main(a)
    logger.info('Script complete.')
    logger.info(f'Elapsed time (total): {time.time() - t0} s')
