"""Training entry point of the DSLR family (deep subspace learning on locally low-rank
blocks) on MI355X: the reference's scripts/train_lr.py by name.

The trainer is scripts/train_swin.py's (same command line, loop, optimiser, scheduler
and checkpoint conventions) with the three things train_lr.py changes:

  * model: META_ARCHITECTURE 'dslr-pgd' -> AltMinPGD, 'dslr-cg-v1' -> AltMinCGv1,
    'dslr-cg-v2' -> AltMinCGv1, 'modslr-v1' -> AltMinMoDLv1, 'modslr-v2' -> AltMinMoDLv2
    (train_lr.py:39-50).  'dslr-cg-v2' builds AltMinCGv1 exactly as the reference does,
    so that checkpoints written under either name agree; AltMinCGv2 is reachable from
    Python only;
  * data: CinePreprocess(lr_decom=True), whose 8-tuple carries the initial block
    factors L_init, R_init (train_lr.py:118, :186-200); --svd device factors them on the
    GPU (dlcs_lr_decompose) instead of the host, with the kernel's phase convention;
  * forward: model(y, A=SenseModel(maps, weights=mask), BlockOp=ArrayToBlocks(block
    size, target shape), L0, R0) (train_lr.py:120-125), batch size 1.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import train_swin as TS  # noqa: E402

ARCHS = {'dslr-pgd': 'AltMinPGD', 'dslr-cg-v1': 'AltMinCGv1', 'dslr-cg-v2': 'AltMinCGv1',
         'modslr-v1': 'AltMinMoDLv1', 'modslr-v2': 'AltMinMoDLv2'}


def build_model(config):
    """train_lr.py:39-50."""
    from dl_cs.models import dslr
    arch = config.MODEL.META_ARCHITECTURE
    if arch not in ARCHS:
        raise ValueError('Meta architecture in config file not recognized!')
    return getattr(dslr, ARCHS[arch])(config)


class LrTrainer(TS.Trainer):
    def __init__(self, config, args, rank, world, device):
        D = config.MODEL.PARAMETERS.DSLR
        self.block_size, self.overlapping = D.BLOCK_SIZE, D.OVERLAPPING
        self._block_ops = {}
        P = config.MODEL.PARAMETERS
        if world > 1 and P.SHARE_WEIGHTS and P.GRAD_CHECKPOINT:
            # a shared network's parameters accumulate once per checkpointed unroll, so the
            # per-parameter hook would start a bucket's all-reduce before the last unroll's gradients
            raise NotImplementedError("DSLR on several GPUs: SHARE_WEIGHTS with GRAD_CHECKPOINT is not supported")
        super().__init__(config, args, rank, world, device)

    def preprocess(self, cls, use_seed):
        return cls(self.cfg, lr_decom=True, use_seed=use_seed, device=self.device,
                   lr_svd=getattr(self.args, 'svd', 'host'))

    def block_op(self, shape):
        """ArrayToBlocks of an image shape, built once per shape (train_lr.py:121 builds one per step)."""
        from dl_cs.mri import lowrank
        key = tuple(shape)
        if key not in self._block_ops:
            self._block_ops[key] = lowrank.ArrayToBlocks(self.block_size, list(shape),
                                                         overlapping=self.overlapping).to(self.device)
        return self._block_ops[key]

    def _forward(self, batch):
        from dl_cs.mri import transforms as T
        kspace, mask, maps, L_init, R_init, init, scale, target = batch   # preprocess.py:178
        if target.shape[0] != 1:
            raise NotImplementedError("DSLR: batch size 1 (the block operators take one image)")
        pred = self.model(y=kspace, A=T.SenseModel(maps, weights=mask), BlockOp=self.block_op(target.shape),
                          L0=L_init.squeeze(0), R0=R_init.squeeze(0))
        if self.cfg.MODEL.RECON_LOSS.RENORMALIZE_DATA:                     # train_lr.py:128-131
            s = scale.view(-1, 1, 1, 1, 1)
            pred, target = pred * s, target * s
        return pred, target


def create_arg_parser():
    p = TS.create_arg_parser()
    p.add_argument('--svd', choices=['host', 'device'], default='host',
                   help="where the initial image is factored into L, R: torch.linalg.svd on the host (the "
                        "reference's) or the block SVD kernel on the GPU; its factors carry other phases, so "
                        "reconstruct with the setting a checkpoint was trained with")
    return p


def main(argv=None):
    args = create_arg_parser().parse_args(argv)
    args.builder = build_model
    args.trainer = 'lr'
    TS.main_args(args)


if __name__ == "__main__":
    main()
