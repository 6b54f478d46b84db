"""Deep subspace learning on locally low-rank blocks (DSLR; dslr = dl_cs/models/dslr.py),
MI355X build: the five unrolled alternating-minimisation networks over the block
factors L [N, E b^2, r] and R [N, T, r] of

    argmin_{L, R} || Y - A(L R^H) ||_F^2 + Psi(L) + Phi(R)

Same classes, constructor, attributes and state_dict keys as the reference
(spatial_cnn_update.*, temporal_cnn_update.*, lambda_l, lambda_r).  Every application of
the low-rank model runs on the fused block kernels (mri/lowrank.py):

    images     = compose(L, R)                         dslr:128-137, one kernel
    x          = A^H A images                          SenseModel.normal (dlcs_sense_normal)
    x R        = project_l(x, R),  x^H L = project_r(x, L)

so the block tensor BlockOp(x) [N, E b^2, T] of dslr:278-279 is never stored; ATy is
kept as an image and projected the same way.  The CNNs are resnet2d / resnet1d on the
HIP conv kernels.  COMPLEX: True and the RNN variant raise NotImplementedError.
"""
import torch
from torch import nn
import torch.utils.checkpoint as cp

from .resnet1d import ResNet as ResNet1D
from .resnet2d import ResNet as ResNet2D
from ..mri import lowrank
from ..mri.algorithms import ConjugateGradient, PowerMethod


class _DenseGrad(torch.autograd.Function):
    """Identity whose gradient is made contiguous.  The gradient of a CNN's input leaves the
    permutes of cnn_update_L / cnn_update_R as a strided view.  Under the re-entrant checkpoint
    an output of the segment that nothing reads downstream (L and R of the MoDL v2 state) gets a
    materialised, contiguous zero gradient first, so the sum with that view is contiguous, while
    the single backward pass hands the view on; torch's reductions in the CG backward then add
    in another order and the two modes differ in the last fp32 bits.  In compute dtype bf16 such
    a difference moves gradient elements across a bf16 rounding boundary in the next CNN
    (2^-8 each), so there both modes are given the same layout; fp32 keeps what it had."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.contiguous()


def _dense_grad(x):
    from .swin3D import get_compute_dtype
    return _DenseGrad.apply(x) if get_compute_dtype() == torch.bfloat16 and x.requires_grad else x


class UnrolledLRNet(nn.Module):
    """dslr:18-170 -- abstract unrolled network over (L, R)."""

    def __init__(self, config):
        super().__init__()
        P = config.MODEL.PARAMETERS
        self.num_unrolls = P.NUM_UNROLLS
        self.num_resblocks = P.NUM_RESBLOCKS
        self.num_features = P.NUM_FEATURES
        self.kernel_size = P.CONV_BLOCK.KERNEL_SIZE[0]
        self.num_emaps = P.NUM_EMAPS
        self.share_weights = P.SHARE_WEIGHTS
        self.fix_step_size = P.FIX_STEP_SIZE
        self.use_complex_layers = P.CONV_BLOCK.COMPLEX
        self.circular_pad = P.CONV_BLOCK.CIRCULAR_PAD
        self.do_checkpoint = P.GRAD_CHECKPOINT
        self.block_size = P.DSLR.BLOCK_SIZE
        self.num_basis = P.DSLR.NUM_BASIS
        if self.use_complex_layers:
            raise NotImplementedError("dl_cs HIP DSLR: COMPLEX: False (configs/config_dslr.yaml)")
        self.spatial_cnn_update = self.init_spatial_nets()
        self.temporal_cnn_update = self.init_temporal_nets()

    def _nets(self, net, in_chans, circular_pad):
        params = dict(in_chans=in_chans, chans=self.num_features, num_resblocks=self.num_resblocks,
                      use_complex_layers=self.use_complex_layers, kernel_size=self.kernel_size,
                      circular_pad=circular_pad)
        if self.share_weights:
            return nn.ModuleList([net(**params)] * self.num_unrolls)      # copies of the same network
        return nn.ModuleList([net(**params) for _ in range(self.num_unrolls)])

    def init_spatial_nets(self):
        """dslr:43-69 -- the spatial basis needs no circular pad."""
        return self._nets(ResNet2D, 2 * self.num_emaps * self.num_basis, False)

    def init_temporal_nets(self):
        """dslr:71-97"""
        return self._nets(ResNet1D, 2 * self.num_basis, self.circular_pad)

    def bucket_nets(self):
        """The networks whose gradients dl_cs.distributed.GradBuckets reduces one bucket each."""
        return list(self.spatial_cnn_update) + list(self.temporal_cnn_update)

    def init_recurrent_nets(self):
        raise NotImplementedError("dl_cs HIP DSLR: the RNN variant (dslr:99-120) is not built")

    def btranspose(self, matrix: torch.Tensor) -> torch.Tensor:
        return matrix.conj().permute(0, 2, 1)

    def compose(self, L, R, BlockOp):
        """dslr:128-137 -- (L, R) -> images, fused."""
        return lowrank.compose(L, R, BlockOp)

    def normal_image(self, L, R, A, BlockOp):
        """A^H A compose(L, R): the image the projections of every model_normal read."""
        return A.normal(self.compose(L, R, BlockOp), 0.0)

    def cnn_update_L(self, L, iter):
        """dslr:139-153"""
        L = _dense_grad(L)
        num_blocks = L.shape[0]
        shape_before = (num_blocks, self.num_basis * self.num_emaps, self.block_size, self.block_size)
        shape_after = (num_blocks, self.num_basis, self.num_emaps * (self.block_size ** 2))
        L = L.permute(0, 2, 1).reshape(shape_before)
        L = self.spatial_cnn_update[iter](L)
        return L.reshape(shape_after).permute(0, 2, 1)

    def cnn_update_R(self, R, iter):
        """dslr:155-164"""
        return self.temporal_cnn_update[iter](_dense_grad(R).permute(0, 2, 1)).permute(0, 2, 1)

    def _unroll(self, update, state):
        """The loop of dslr:245-250: one (checkpointed) update per unroll over the state tuple."""
        if self.training and self.do_checkpoint:
            for t in state:
                t.requires_grad_()                                        # needed by the re-entrant checkpoint
        for i in range(self.num_unrolls):
            if self.training and self.do_checkpoint:
                state = cp.checkpoint(update(i), *state, use_reentrant=True)
            else:
                state = update(i)(*state)
        return state

    def forward(self, y, A, BlockOp, L0, R0):
        raise NotImplementedError


class AltMinPGD(UnrolledLRNet):
    """dslr:173-255 -- gradient steps on L and R with power-method step sizes."""

    def __init__(self, config):
        super().__init__(config)
        self.power_method = PowerMethod(num_iter=10)

    def get_step_sizes(self, L, R, alpha=0.9, v0=None):
        """dslr:187-199; v0 = (start vector for R, for L) or None (torch.rand)."""
        v0 = v0 or (None, None)
        step_size_L = -1.0 * alpha / self.power_method(R, v0[0]).max()
        step_size_R = -1.0 * alpha / self.power_method(L, v0[1]).max()
        return step_size_L, step_size_R

    def dc_update(self, L_prev, R_prev, A, BlockOp, ATy, v0=None):
        """dslr:201-216 -- both projections of the one gradient image."""
        grad_x = self.normal_image(L_prev, R_prev, A, BlockOp) - ATy
        grad_L = lowrank.project_l(grad_x, R_prev, BlockOp)
        grad_R = lowrank.project_r(grad_x, L_prev, BlockOp)
        step_size_L, step_size_R = self.get_step_sizes(L_prev, R_prev, v0=v0)
        return L_prev + step_size_L * grad_L, R_prev + step_size_R * grad_R

    def forward(self, y, A, BlockOp, L0, R0, v0=None):
        """v0: per unroll, the power method's start vectors (for R, for L); None draws them."""
        ATy = A(y, adjoint=True)

        def update(i):
            def update_fn(L, R):
                L, R = self.dc_update(L, R, A, BlockOp, ATy, None if v0 is None else v0[i])
                return self.cnn_update_L(L, i), self.cnn_update_R(R, i)
            return update_fn

        Li, Ri = self._unroll(update, (L0, R0))
        return self.compose(Li, Ri, BlockOp)


class _AltMinCG(UnrolledLRNet):
    """What the CG and MoDL variants share: the two data-consistency solves
    (dslr:271-301, :452-482, :550-586)."""

    def __init__(self, config):
        super().__init__(config)
        self.num_cg_iter = config.MODEL.PARAMETERS.DSLR.NUM_CG_STEPS

    def penalty(self, which):
        return None

    def dc_update_L(self, L_update, R_fixed, A, ATy, BlockOp, L_cnn=None):
        lamda = None if L_cnn is None else self.penalty("l")

        def model_normal(L):
            out = lowrank.project_l(self.normal_image(L, R_fixed, A, BlockOp), R_fixed, BlockOp)
            return out if lamda is None else lamda * L + out

        rhs = lowrank.project_l(ATy, R_fixed, BlockOp)
        if lamda is not None:
            rhs = lamda * L_cnn + rhs
        return ConjugateGradient(model_normal, self.num_cg_iter)(L_update, rhs)

    def dc_update_R(self, R_update, L_fixed, A, ATy, BlockOp, R_cnn=None):
        lamda = None if R_cnn is None else self.penalty("r")

        def model_normal(R):
            out = lowrank.project_r(self.normal_image(L_fixed, R, A, BlockOp), L_fixed, BlockOp)
            return out if lamda is None else lamda * R + out

        rhs = lowrank.project_r(ATy, L_fixed, BlockOp)
        if lamda is not None:
            rhs = lamda * R_cnn + rhs
        return ConjugateGradient(model_normal, self.num_cg_iter)(R_update, rhs)


class AltMinCGv1(_AltMinCG):
    """dslr:258-341 -- CG on L, CG on R, then both CNNs."""

    def forward(self, y, A, BlockOp, L0, R0):
        ATy = A(y, adjoint=True)

        def update(i):
            def update_fn(L, R):
                L = self.dc_update_L(L, R, A, ATy, BlockOp)
                R = self.dc_update_R(R, L, A, ATy, BlockOp)
                return self.cnn_update_L(L, i), self.cnn_update_R(R, i)
            return update_fn

        Li, Ri = self._unroll(update, (L0, R0))
        return self.compose(Li, Ri, BlockOp)


class AltMinCGv2(_AltMinCG):
    """dslr:344-425 -- CG and CNN on L, then CG and CNN on R."""

    def forward(self, y, A, BlockOp, L0, R0):
        ATy = A(y, adjoint=True)

        def update(i):
            def update_fn(L, R):
                L = self.cnn_update_L(self.dc_update_L(L, R, A, ATy, BlockOp), i)
                R = self.cnn_update_R(self.dc_update_R(R, L, A, ATy, BlockOp), i)
                return L, R
            return update_fn

        Li, Ri = self._unroll(update, (L0, R0))
        return self.compose(Li, Ri, BlockOp)


class AltMinMoDLv1(_AltMinCG):
    """dslr:428-522 -- MoDL sub-problems with penalties lambda_l, lambda_r."""

    def __init__(self, config):
        super().__init__(config)
        self.lambda_l = nn.Parameter(torch.tensor([1.0], dtype=torch.float32), requires_grad=(not self.fix_step_size))
        self.lambda_r = nn.Parameter(torch.tensor([2.0], dtype=torch.float32), requires_grad=(not self.fix_step_size))

    def penalty(self, which):
        return self.lambda_l if which == "l" else self.lambda_r

    def forward(self, y, A, BlockOp, L0, R0):
        ATy = A(y, adjoint=True)

        def update(i):
            def update_fn(L, R):
                L = self.dc_update_L(L, R, A, ATy, BlockOp, L_cnn=self.cnn_update_L(L, i))
                R = self.dc_update_R(R, L, A, ATy, BlockOp, R_cnn=self.cnn_update_R(R, i))
                return L, R
            return update_fn

        Li, Ri = self._unroll(update, (L0, R0))
        return self.compose(Li, Ri, BlockOp)


class AltMinMoDLv2(_AltMinCG):
    """dslr:525-635 -- MoDL with the CNN outputs as the fixed factor and scaled, clamped penalties."""

    def __init__(self, config):
        super().__init__(config)
        self.lambda_l = nn.Parameter(torch.tensor([5e-3], dtype=torch.float32), requires_grad=(not self.fix_step_size))
        self.lambda_r = nn.Parameter(torch.tensor([5e-3], dtype=torch.float32), requires_grad=(not self.fix_step_size))
        self.lambda_scale = 1e2                                           # raises the penalties' learning rate

    def penalty(self, which):
        return self.lambda_scale * torch.clamp(self.lambda_l if which == "l" else self.lambda_r, min=0.0, max=None)

    def forward(self, y, A, BlockOp, L0, R0):
        ATy = A(y, adjoint=True)

        def update(i):
            def update_fn(L, zL, R, zR):
                # the fixed R: the initial guess first, then the previous unroll's CNN output
                L = self.dc_update_L(L, R if i == 0 else zR, A, ATy, BlockOp, L_cnn=zL)
                zL = self.cnn_update_L(L, i)
                R = self.dc_update_R(R, zL, A, ATy, BlockOp, R_cnn=zR)
                zR = self.cnn_update_R(R, i)
                return L, zL, R, zR
            return update_fn

        _, zLi, _, zRi = self._unroll(update, (L0, torch.zeros_like(L0), R0, torch.zeros_like(R0)))
        return self.compose(zLi, zRi, BlockOp)
