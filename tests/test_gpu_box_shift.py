"""dlcs_box_shift (csrc/box.hip): the centre crop of the DiT / Latte unpatchify2 as a voxel
shift of the box inside the padded grid, and its adjoint, against a numpy gather.  The shift
is a permutation with zero fill, so everything is compared with torch.equal (with a residual:
one fp32 add per element, the same one numpy does)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 777.0
# (padded grid (B, Dp, Hp, Wp), box (D, H, W)): one patch block in time, and several blocks
# per axis with two batch items; every box axis short of its padded axis
GRIDS = [((1, 4, 8, 8), (3, 6, 6)), ((2, 12, 12, 12), (9, 10, 9))]
SHIFTS = [(0, 0, 1), (1, 2, 2), (0, 0, 0)]


def _K():
    from dl_cs.models import _ops as K
    return K


def _rows(grid):
    """Blocked row of every voxel: int64 [B, Dp, Hp, Wp]."""
    B, Dp, Hp, Wp = grid
    b, t, y, x = np.meshgrid(np.arange(B), np.arange(Dp), np.arange(Hp), np.arange(Wp), indexing="ij")
    patch = ((b * (Dp // 4) + t // 4) * (Hp // 4) + y // 4) * (Wp // 4) + x // 4
    return patch * 64 + (t % 4) * 16 + (y % 4) * 4 + x % 4


def _ref(src, grid, box, shift, C, transpose, res=None, relu=False):
    """numpy gather: [rows, C] with zeros where there is no source."""
    rows = _rows(grid)
    D, H, W = box
    sd, sh, sw = shift
    out = np.zeros((rows.size, C), np.float32)
    lo = rows[:, :D, :H, :W].reshape(-1)                               # the box
    hi = rows[:, sd:D + sd, sh:H + sh, sw:W + sw].reshape(-1)          # the box moved by the shift
    if transpose:
        out[hi] = src[lo, :C]
    else:
        out[lo] = src[hi, :C]
        if res is not None:
            out[lo] = out[lo] + res[lo, :C]
        if relu:
            out = np.maximum(out, 0.0)
    return out


def _rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("C,ld", [(4, 8), (6, 8), (384, 388)])
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("grid,box", GRIDS)
def test_box_shift_vs_gather(grid, box, shift, C, ld):
    """Both directions, with and without the residual (and the ReLU after it): dst starts as NaN
    in [0, C) and a sentinel in the guard columns [C, ld) -- every row of the padded grid is
    written, the guard columns are not."""
    K = _K()
    assert all(n + s <= p for n, s, p in zip(box, shift, grid[1:]))      # refusals: test_box_shift_refuses
    V = int(np.prod(grid))
    src, res = _rnd((V, ld), 1), _rnd((V, ld), 2)
    sd_, rd_ = src.to(DEV), res.to(DEV)
    fbox = (grid[0],) + box
    for transpose, r, relu in ((False, None, False), (False, rd_, False), (False, rd_, True), (True, None, False)):
        dst = torch.full((V, ld), float("nan"), device=DEV)
        dst[:, C:] = SENT
        K.box_shift(sd_, C, grid, fbox, shift, transpose=transpose, out=dst, res=r, relu=relu)
        want = _ref(src.numpy(), grid, box, shift, C, transpose, None if r is None else res.numpy(), relu)
        got = dst.cpu()
        assert torch.equal(got[:, :C], torch.from_numpy(want)), (transpose, r is not None, relu)
        assert bool((got[:, C:] == SENT).all())
        if r is None:                                  # the zero fill is +0.0 (torch.equal takes -0.0 too)
            assert not bool(torch.signbit(got[:, :C][torch.from_numpy(want) == 0]).any())


@pytest.mark.parametrize("C", [4, 6])
def test_box_shift_scalar_path_on_odd_strides(C):
    """ld = 7 (no multiple of 4) takes the one-float path whatever C is."""
    K = _K()
    grid, box, shift = (2, 12, 12, 12), (9, 10, 9), (1, 2, 2)
    V = int(np.prod(grid))
    src = _rnd((V, 7), 3)
    dst = torch.full((V, 7), float("nan"), device=DEV)
    dst[:, C:] = SENT
    K.box_shift(src.to(DEV), C, grid, (2,) + box, shift, out=dst)
    got = dst.cpu()
    assert torch.equal(got[:, :C], torch.from_numpy(_ref(src.numpy(), grid, box, shift, C, False)))
    assert bool((got[:, C:] == SENT).all())


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("grid,box", GRIDS)
def test_box_shift_adjoint_identity(grid, box, shift):
    """<shift(a), b> = <a, shift^T(b)> over the rows of the padded grid, summed in float64: both
    sides are the same products (a at the moved box times b at the box), so 1e-12 relative."""
    K = _K()
    V, C = int(np.prod(grid)), 8
    a, b = _rnd((V, C), 4).to(DEV), _rnd((V, C), 5).to(DEV)
    fbox = (grid[0],) + box
    sa = K.box_shift(a, C, grid, fbox, shift)
    stb = K.box_shift(b, C, grid, fbox, shift, transpose=True)
    lhs = float((sa.double() * b.double()).sum())
    rhs = float((a.double() * stb.double()).sum())
    assert abs(lhs) > 1.0 and abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)


def test_box_shift_refuses():
    """A shift that leaves the padded grid, a padded axis that is no multiple of 4 and a box
    larger than the grid return DLCS_ERR_UNSUPPORTED_SIZE before any launch: dst keeps its
    fill.  transpose with a residual, and dst = src, are invalid arguments."""
    from dl_cs import _lib
    K = _K()
    grid = (1, 4, 8, 8)
    V = int(np.prod(grid))
    src = _rnd((V, 8), 6).to(DEV)
    for g, box, shift in ((grid, (3, 6, 6), (2, 0, 0)), (grid, (3, 6, 6), (0, 3, 0)), (grid, (3, 6, 6), (0, 0, 3)),
                          ((1, 4, 8, 6), (3, 6, 6), (0, 0, 0)), (grid, (5, 6, 6), (0, 0, 0))):
        for transpose in (False, True):
            dst = torch.full((V, 8), SENT, device=DEV)
            with pytest.raises(_lib.DlcsError, match="unsupported"):
                K.box_shift(src, 8, g, (1,) + box, shift, transpose=transpose, out=dst)
            assert bool((dst == SENT).all())
    dst = torch.full((V, 8), SENT, device=DEV)
    with pytest.raises(_lib.DlcsError, match="invalid argument"):
        K.box_shift(src, 8, grid, (1, 3, 6, 6), (1, 1, 1), transpose=True, out=dst, res=src)
    with pytest.raises(_lib.DlcsError, match="invalid argument"):
        K.box_shift(src, 8, grid, (1, 3, 6, 6), (1, 1, 1), out=src)
    assert bool((dst == SENT).all())
