"""Locally low-rank block operators of the DSLR family (lr = dl_cs/mri/lowrank.py).

ArrayToBlocks cuts one dynamic image [1, E, T, Y, X] into N overlapping b x b blocks
[N, E b^2, T] (stride b / 2, sqrt-Hann window, zero pad; lr:47-96, :149-161) and folds
them back (lr:98-178).  Decompose factors every block into L [N, E b^2, r] and
R [N, T, r] by a truncated SVD: on the host (lr:213-238), or with svd='device' by
dlcs_lr_decompose, one Jacobi SVD per block in LDS, straight from the GPU image.

On GPU tensors the dlcs_lr_* kernels do the work: extract, combine, and the fused
compose (L, R -> image), project_l (image, R -> extract(image) R) and project_r
(image, L -> extract(image)^H L), which never store the block tensor.  There is no
fallback for GPU tensors outside the kernels' range (NotImplementedError).  CPU tensors
go through plain torch ops: preprocessing runs in loader workers.  GPU tensors need an
operator that was moved to the same GPU (`.to(device)`) and complex64 data; an operator left
on the host (Decompose(svd='host')'s always is: its SVD runs there) raises DlcsError, as mixed devices
do in SenseModel.

The `divide` flag of the kernels: combine(divide=1) is the reference's combine (fold,
crop, / (weights + 1e-8)); divide=0 leaves the division out, which makes it the exact
adjoint of extract.  extract(divide=1) divides the image first: the adjoint of
combine(divide=1).  Autograd is four Functions over these.
"""
from typing import List, Optional, Tuple

import torch
from torch import nn

from . import utils
from .. import _lib
from ..models import _ops

EPS = 1e-8


# ------------------------------------------------------------------ torch path (CPU)
def _t_extract(op, image, divide):
    """image [E, T, Y, X] -> blocks [N, E b^2, T] (lr:79-96, :149-161)."""
    b, s = op.block_size, op.block_stride
    if divide:
        image = image / (op.weights2d.to(image.device) + EPS)
    x = nn.functional.pad(image, tuple(op.pad_x) + tuple(op.pad_y), mode='constant')
    x = x.unfold(2, b, s).unfold(3, b, s)                         # [E, T, nby, nbx, b, b]
    x = x.permute(2, 3, 0, 4, 5, 1).reshape(op.num_blocks, op.ne * b * b, op.nt)
    return x * op.win.to(image.device)


def _t_combine(op, blocks, divide):
    """blocks [N, E b^2, T] -> image [E, T, Y, X]: overlap-add of the windowed blocks,
    centre crop, / (weights + 1e-8) (lr:98-178)."""
    b, s = op.block_size, op.block_stride
    x = (blocks * op.win.to(blocks.device)).reshape(op.num_blocks_y, op.num_blocks_x, op.ne, b, b, op.nt)
    x = x.permute(2, 5, 0, 3, 1, 4)                               # [E, T, nby, b, nbx, b]
    out = x.new_zeros((op.ne, op.nt, op.ny_pad, op.nx_pad))
    for oy in (0, 1):
        for ox in (0, 1):
            part = x[:, :, oy::2, :, ox::2, :]
            ny, nx = part.shape[2] * b, part.shape[4] * b
            out[:, :, oy * s:oy * s + ny, ox * s:ox * s + nx] += part.reshape(op.ne, op.nt, ny, nx)
    out = utils.center_crop(out, shapes=[op.ny, op.nx], dims=[-2, -1])
    if divide:
        out = out / (op.weights2d.to(blocks.device) + EPS)
    return out


def _bt(m):
    return m.conj().transpose(1, 2)


# ------------------------------------------------------------------ raw ops (kernel or torch)
def _c(t):
    """A kernel operand: complex64 (anything else raises, as in the rest of the HIP path), contiguous."""
    if t.dtype != torch.complex64:
        raise _lib.DlcsError(f"low-rank block kernels take complex64 tensors, not {t.dtype}")
    return t.contiguous()


def _nb(op, *mats):
    """The kernels size their launches from the geometry: every block matrix must have op's N."""
    for m in mats:
        assert m.dim() == 3 and m.shape[0] == op.num_blocks, (tuple(m.shape), op.num_blocks)


def _extract_raw(op, image, divide):
    if image.is_cuda:
        return _ops.lr_extract(_c(image), op.weights2d, op.win1d, op.block_size, op.num_blocks, divide)
    return _t_extract(op, image, divide)


def _combine_raw(op, blocks, divide):
    _nb(op, blocks)
    if blocks.is_cuda:
        return _ops.lr_combine(_c(blocks), op.weights2d, op.win1d, op.block_size, op.shape4, divide)
    return _t_combine(op, blocks, divide)


def _compose_raw(op, L, R, divide):
    _nb(op, L, R)
    if L.is_cuda:
        return _ops.lr_compose(_c(L), _c(R), op.weights2d, op.win1d, op.block_size, op.shape4, divide)
    return _t_combine(op, torch.bmm(L, _bt(R)), divide)


def _project_l_raw(op, image, R, divide):
    _nb(op, R)
    if image.is_cuda:
        return _ops.lr_project_l(_c(image), _c(R), op.weights2d, op.win1d, op.block_size, divide)
    return torch.bmm(_t_extract(op, image, divide), R)


def _project_r_raw(op, image, L, divide):
    _nb(op, L)
    if image.is_cuda:
        return _ops.lr_project_r(_c(image), _c(L), op.weights2d, op.win1d, op.block_size, divide)
    return torch.bmm(_bt(_t_extract(op, image, divide)), L)


# ------------------------------------------------------------------ autograd
class _ExtractFn(torch.autograd.Function):
    """extract(divide) <-> combine(divide)."""

    @staticmethod
    def forward(ctx, image, op, divide):
        ctx.op, ctx.divide = op, divide
        return _extract_raw(op, image, divide)

    @staticmethod
    def backward(ctx, g):
        return _combine_raw(ctx.op, g, ctx.divide), None, None


class _CombineFn(torch.autograd.Function):
    """combine(divide) <-> extract(divide)."""

    @staticmethod
    def forward(ctx, blocks, op, divide):
        ctx.op, ctx.divide = op, divide
        return _combine_raw(op, blocks, divide)

    @staticmethod
    def backward(ctx, g):
        return _extract_raw(ctx.op, g, ctx.divide), None, None


class _ComposeFn(torch.autograd.Function):
    """image = combine_d(L R^H): dL = extract_d(g) R, dR = extract_d(g)^H L."""

    @staticmethod
    def forward(ctx, L, R, op, divide):
        ctx.op, ctx.divide = op, divide
        ctx.save_for_backward(L, R)
        return _compose_raw(op, L, R, divide)

    @staticmethod
    def backward(ctx, g):
        L, R = ctx.saved_tensors
        dL = _ProjectFn.apply(g, R, ctx.op, ctx.divide, False) if ctx.needs_input_grad[0] else None
        dR = _ProjectFn.apply(g, L, ctx.op, ctx.divide, True) if ctx.needs_input_grad[1] else None
        return dL, dR, None, None


class _ProjectFn(torch.autograd.Function):
    """right=False: extract_d(image) M (M = R); right=True: extract_d(image)^H M (M = L).
    d image = combine_d(G M^H) resp. combine_d(M G^H); dM is the other projection of the
    image with G."""

    @staticmethod
    def forward(ctx, image, M, op, divide, right):
        ctx.op, ctx.divide, ctx.right = op, divide, right
        ctx.save_for_backward(image, M)
        return (_project_r_raw if right else _project_l_raw)(op, image, M, divide)

    @staticmethod
    def backward(ctx, g):
        image, M = ctx.saved_tensors
        dimg = dM = None
        if ctx.needs_input_grad[0]:
            LR = (M, g) if ctx.right else (g, M)
            dimg = _ComposeFn.apply(LR[0], LR[1], ctx.op, ctx.divide)
        if ctx.needs_input_grad[1]:
            dM = _ProjectFn.apply(image, g, ctx.op, ctx.divide, not ctx.right)
        return dimg, dM, None, None, None


def _img4(op, image):
    assert tuple(image.shape[-4:]) == op.shape4 and image.numel() == op.ne * op.nt * op.ny * op.nx, \
        (tuple(image.shape), op.shape4)                           # batch 1 (lr:86-87)
    return image.reshape(op.shape4)


def compose(L, R, block_op, divide=True):
    """combine(L R^H) [1, E, T, Y, X] (lr:247-253) in one pass."""
    return _ComposeFn.apply(L, R, block_op, bool(divide)).unsqueeze(0)


def project_l(image, R, block_op, divide=False):
    """extract(image) R: [N, E b^2, r]."""
    return _ProjectFn.apply(_img4(block_op, image), R, block_op, bool(divide), False)


def project_r(image, L, block_op, divide=False):
    """extract(image)^H L: [N, T, r]."""
    return _ProjectFn.apply(_img4(block_op, image), L, block_op, bool(divide), True)


# ------------------------------------------------------------------ modules
class ArrayToBlocks(nn.Module):
    """lr:13-187 -- the array <-> blocks operator.
      - extract() converts [1, E, T, Y, X] into blocks [N, E b^2, T]
      - combine() folds blocks back into [1, E, T, Y, X] and divides by the window weights
    """

    def __init__(self, block_size: int, image_shape: List[int], overlapping: Optional[bool] = False) -> None:
        super().__init__()
        assert overlapping is True                                # lr:25-26
        self.block_size = block_size
        self.image_shape = image_shape
        _, self.ne, self.nt, self.ny, self.nx = image_shape
        self.shape4 = (self.ne, self.nt, self.ny, self.nx)
        self.block_stride = block_size // 2
        win1d = torch.hann_window(block_size, dtype=torch.float32) ** 0.5
        win = win1d[None, :, None] * win1d[None, None, :]
        win = win.repeat(self.ne, 1, 1).reshape((1, self.ne * (block_size ** 2), 1))
        self.register_buffer('win', win)
        self.pad_x, self.pad_y = self._get_pad_sizes()
        self.nx_pad = self.pad_x[0] + self.nx + self.pad_x[1]
        self.ny_pad = self.pad_y[0] + self.ny + self.pad_y[1]
        self.num_blocks_x = int((self.nx_pad - self.block_size) / self.block_stride + 1)
        self.num_blocks_y = int((self.ny_pad - self.block_size) / self.block_stride + 1)
        self.num_blocks = self.num_blocks_x * self.num_blocks_y
        # the reference's buffers (in its state_dict) and the kernels' fp32 operands (not)
        self.register_buffer('win1d', win1d, persistent=False)
        self.register_buffer('weights2d', torch.zeros(self.ny, self.nx), persistent=False)
        self.register_buffer('weights', None)
        ones = torch.ones(self.shape4, dtype=torch.complex64)
        weights = _t_combine(self, _t_extract(self, ones, False), False)      # lr:57-60
        self.weights = weights.unsqueeze(0)
        self.weights2d = weights[0, 0].real.contiguous()

    def _get_pad_sizes(self) -> Tuple[Tuple[int]]:
        """lr:62-77 -- pad so that a whole number of blocks fits; an odd size pads one more on the right."""
        b = self.block_size
        left_x = (b * (self.nx // b + 1) - self.nx) // 2
        left_y = (b * (self.ny // b + 1) - self.ny) // 2
        return ((left_x, left_x if self.nx % 2 == 0 else left_x + 1),
                (left_y, left_y if self.ny % 2 == 0 else left_y + 1))

    def extract(self, data: torch.Tensor) -> torch.Tensor:
        return _ExtractFn.apply(_img4(self, data), self, False)

    def combine(self, data: torch.Tensor) -> torch.Tensor:
        return _CombineFn.apply(data, self, True).unsqueeze(0)

    def extract_adjoint(self, data: torch.Tensor) -> torch.Tensor:
        """combine without the division: the exact adjoint of extract."""
        return _CombineFn.apply(data, self, False).unsqueeze(0)

    def combine_adjoint(self, data: torch.Tensor) -> torch.Tensor:
        """extract of data / (weights + 1e-8): the exact adjoint of combine."""
        return _ExtractFn.apply(_img4(self, data), self, True)

    def forward(self, input: torch.Tensor, adjoint: Optional[bool] = False) -> torch.Tensor:
        return self.combine(input) if adjoint else self.extract(input)


def decompose_blocks(image, op, rank, return_s=False, return_info=False):
    """The raw dlcs_lr_decompose call: image [E, T, Y, X] (or [1, E, T, Y, X]) complex64 on the
    GPU -> (L [N, E b^2, r], R [N, T, r][, S [N, r]][, sweeps [N]]) of the truncated SVD of
    every block of op's geometry; op's win1d must be on the image's GPU."""
    return _ops.lr_decompose(_img4(op, image), op.win1d, op.block_size, rank, want_s=return_s, want_info=return_info)


class Decompose(nn.Module):
    """lr:190-262 -- blocks of [1, E, T, Y, X] factored into L [N, E b^2, r] and
    R [N, T, r] (L = U sqrt(S), R = V sqrt(S) of the truncated SVD), and compose().

    svd='host' (the default) is the reference's path: blocks and torch.linalg.svd on the host,
    the factors copied to the image's device.  svd='device' takes a GPU image and factors every
    block in one dlcs_lr_decompose launch (one-sided Jacobi in LDS); the factors stay on the
    GPU.  Its singular pairs carry the kernel's phase convention (the largest entry of R_k real
    and positive), not LAPACK's: L R^H is the same, L and R differ by a unit phase per column."""

    def __init__(self, block_size: int, rank: int, image_shape: List[int], overlapping: Optional[bool] = False,
                 device: str = 'cpu', svd: str = 'host') -> None:
        super().__init__()
        assert device == 'cpu'                                    # the SVD runs on the host (lr:206-207)
        assert svd in ('host', 'device'), svd
        self.block_size = block_size
        self.rank = rank
        self.svd = svd
        self.block_op = ArrayToBlocks(block_size, image_shape, overlapping).to(device)
        self._gpu_ops = {}                                        # svd='device': the operator per GPU

    def _op_on(self, device):
        """The operator whose buffers live on `device` (built lazily, one per GPU)."""
        if device.type != 'cuda':
            return self.block_op
        if device not in self._gpu_ops:
            self._gpu_ops[device] = ArrayToBlocks(self.block_size, self.block_op.image_shape, True).to(device)
        return self._gpu_ops[device]

    def decompose(self, images: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        rk = self.rank
        if self.svd == 'device':
            if not images.is_cuda:
                raise _lib.DlcsError("Decompose(svd='device') takes an image on the GPU")
            return decompose_blocks(images, self._op_on(images.device), rk)
        dev = images.device
        blocks = self.block_op(images.cpu() if images.is_cuda else images)
        U, S, Vh = torch.linalg.svd(blocks, full_matrices=False)
        s_sqrt = S[:, None, :rk].sqrt()
        L = U[:, :, :rk] * s_sqrt
        R = _bt(Vh)[:, :, :rk] * s_sqrt
        return L.contiguous().to(dev), R.contiguous().to(dev)

    def btranspose(self, matrix_batch: torch.Tensor) -> torch.Tensor:
        return _bt(matrix_batch)

    def compose(self, L: torch.Tensor, R: torch.Tensor) -> torch.Tensor:
        return compose(L, R, self._op_on(L.device) if self.svd == 'device' else self.block_op)

    def forward(self, data, adjoint=False):
        if adjoint:
            L, R = data
            return self.compose(L, R)
        return self.decompose(data)
