"""Inference entry point for H5 cine data: reconstruct every slice of one H5 file
with a trained unrolled model on MI355X.

Same command line, data handling and output as the reference's
scripts/reconstruct_h5.py (rh5; CLI :488-500, Hdf5Dataset :157-260,
DataTransform :263-312, DataTransformSS :314-368, main :370-485):

  * H5 layout (prepare_stage2.py:232-242): kspace [sl, coils, T, Y, X], maps
    [sl, emaps, coils, 1, Y, X], target [sl, emaps, T, Y, X];
  * --acceleration A > 1: the fully-sampled k-space is undersampled with the
    VDkt k-t mask at (A, A) and the config's partial kx / ky, seed 1000 (:336),
    then reconstructed; A = 1: the mask comes from the data and the output is the
    scaled A^H y initial guess itself (:459-461, no network call);
  * no fftmod (commented out in :281-283, :339-341); 95th-percentile scale,
    sliding-window initial guess when SLWIN_INIT; images rescaled (:455);
  * --model SWIN (unrolledswin, LitUnrolledSWIN :98-122) or RES (unrolled,
    LitUnrolledResNet :46-70); the Lightning checkpoint's 'model.' prefix is
    stripped (dl_cs.checkpoint, torch.load(weights_only=True));
  * output <out-directory>/<file stem>_<A>accel.im.{cfl,hdr}, dims [x, y, sl,
    emap, phase, 1, 1, 1] column-major (:209-240).
The preprocessing runs on the GPU (dl_cs.data.preprocess.DataTransform: the HIP
SENSE adjoint, device top-k); --multi-gpu spreads slices over every visible GPU.
h5py reads the file when installed; a .npz with the same three arrays is read
without it (this image has no h5py).
"""
import argparse
import logging
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dl-swin-gan_amd"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from dl_cs import checkpoint  # noqa: E402
from dl_cs.config import load_cfg  # noqa: E402
from dl_cs.fileio import cfl  # noqa: E402

logging.basicConfig(level=logging.INFO)
logger = logging.getLogger("reconstruct_h5")


class Hdf5Dataset:
    """rh5:157-260 -- one example per slice of an H5 (or .npz) file."""

    def __init__(self, file):
        self.file = file
        if file.endswith(".npz"):
            self._h5 = None
            d = np.load(file)
            self._arr = {k: d[k] for k in ("kspace", "maps")}
        else:
            try:
                import h5py
            except ImportError as e:
                raise ImportError("reconstruct_h5: reading .h5 needs h5py (or pass the same arrays as a .npz)") from e
            self._h5 = h5py.File(file, 'r')
            self._arr = {k: self._h5[k] for k in ("kspace", "maps")}
        ks, maps = self._arr["kspace"], self._arr["maps"]
        # rh5:195-206 -- [sl, coils, phases, y, x] and [sl, emaps, ...]
        self.image_dims = (ks.shape[0], maps.shape[1], ks.shape[2], ks.shape[3], ks.shape[4])

    def __len__(self):
        return self.image_dims[0]

    def __getitem__(self, sl):
        return np.asarray(self._arr["kspace"][sl]), np.asarray(self._arr["maps"][sl])

    def write(self, file_im, images):
        """rh5:209-240 -- [n, emap, phase, y, x] -> [x, y, sl, emap, phase, 1, 1, 1] (column-major)."""
        im = np.reshape(np.asarray(images), self.image_dims)
        im = np.transpose(im, (4, 3, 0, 1, 2))[:, :, :, :, :, None, None, None]
        cfl.write(file_im, im, order='F')


def build_model(config, model_type):
    """rh5:398-406 -- the Lit* wrapper by --model: SWIN (:98-122), RES (:46-70) or SE (unrolledSE)."""
    from dl_cs.models import unrolled, unrolledSE, unrolledswin
    mods = {'SWIN': unrolledswin, 'RES': unrolled, 'SE': unrolledSE}
    if model_type not in mods:
        raise NotImplementedError(f"--model {model_type}: SWIN, RES and SE are built for MI355X")
    if config.MODEL.META_ARCHITECTURE == 'dlespirit':
        return mods[model_type].ProximalGradientDescent(config)
    if config.MODEL.META_ARCHITECTURE == 'modl':
        return mods[model_type].HalfQuadraticSplitting(config)
    raise ValueError('Meta architecture in config file not recognized!')


def main(args):
    from dl_cs.data.preprocess import DataTransform
    from dl_cs.models import swin3D
    from dl_cs.mri import transforms as T
    swin3D.set_compute_dtype(torch.bfloat16 if args.dtype == 'bf16' else torch.float32)
    accel = args.acceleration
    stem = os.path.splitext(os.path.basename(args.file))[0]
    file_images = os.path.join(args.out_directory, f"{stem}_{accel}accel.im")             # rh5:375
    if args.multi_gpu:
        devices = [torch.device('cuda', i) for i in range(torch.cuda.device_count())]
        logger.info(f'Running on {len(devices)} GPU devices...')
    else:
        if args.device < 0:
            raise RuntimeError("the unrolled model runs on the GPU (HIP kernels): pass --device N")
        devices = [torch.device('cuda', args.device)]
    config = load_cfg(args.config_file)
    models, tfs = {}, {}
    for d in devices:
        if accel > 1:
            m = build_model(config, args.model)
            checkpoint.load_model(m, args.ckpt)
            m.eval()
            for p in m.parameters():                                              # freeze() (rh5:408)
                p.requires_grad_(False)
            models[d] = m.to(d)
        tfs[d] = DataTransform(config, device=d, fftmod=False, acceleration=accel)
    logger.info(f'Loading H5 data {args.file}...')
    data = Hdf5Dataset(args.file)
    logger.info('Running inference...')
    start = time.time()
    out = [None] * len(data)
    bs = args.batch_size
    for b0 in range(0, len(data), bs):
        d = devices[(b0 // bs) % len(devices)]
        with torch.cuda.device(d):
            items = [tfs[d](*data[i]) for i in range(b0, min(len(data), b0 + bs))]
            kspace, maps, mask, init, scale = (torch.stack([it[k] for it in items]) for k in range(5))
            if accel > 1:
                with torch.no_grad():
                    images = models[d](y=kspace, A=T.SenseModel(maps, weights=mask), x0=init)
            else:
                images = init                                                     # rh5:459-461
            im = (scale.view(-1, 1, 1, 1, 1) * images).cpu().numpy()              # rh5:455
        for j in range(im.shape[0]):
            out[b0 + j] = im[j]
    logger.info(f'Elapsed time (reconstruction): {time.time() - start} s')
    logger.info(f'Writing images to {file_images}')
    data.write(file_images, np.stack(out))


def create_arg_parser():
    parser = argparse.ArgumentParser(description="Inference script for unrolled MRI recon (H5 input).")
    parser.add_argument('--file', type=str, required=True, help='Name of the H5 file with kspace, mask, and map')
    parser.add_argument('--model', type=str, required=True, help='SWIN (Swin-unrolled), RES (unrolled ResNet) or SE (unrolled SE-ResNet)')
    parser.add_argument('--acceleration', type=int, default=1, help='Undersampling Accelration Factor')
    parser.add_argument('--out-directory', type=str, required=True, help='Output Directory')
    parser.add_argument('--ckpt', type=str, required=True, help='Model checkpoint file')
    parser.add_argument('--batch-size', type=int, default=1, help='Slices per batch')
    parser.add_argument('--config-file', type=str, required=True, help='Training config file (yaml)')
    parser.add_argument('--device', type=int, default=-1, help='GPU device')
    parser.add_argument('--multi-gpu', action='store_true', help='Uses multiple GPUs for inference (overrides device flag)')
    parser.add_argument('--verbose', action='store_true', help='Turn on debug statements')
    parser.add_argument('--dtype', choices=['fp32', 'bf16'], default='fp32', help='compute dtype of the regularizer')
    return parser


if __name__ == '__main__':
    main(create_arg_parser().parse_args())
