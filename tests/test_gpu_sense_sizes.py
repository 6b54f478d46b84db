"""2-D FFT and SENSE operator at in-plane lengths that are not 2-3-5-smooth:
Stockham passes of radix 7 / 11 / 13 and Bluestein's algorithm (csrc/sense.hip,
sense_anylen.inc), either kind on either axis.  Same bars as test_gpu_sense.py:
fft2 vs float64 numpy NRMSE < 2e-6, SENSE operators vs the oracle NRMSE < 1e-5.
dlcs_fft_plan says which case a length takes, so each case asserts its path."""
import ctypes

import numpy as np
import pytest
import torch

from goldutil import nrmse
from oracle import dlcs_oracle as O
from oracle import recipe

pytestmark = pytest.mark.gpu
TOL = 1e-5
FFT_TOL = 2e-6
DEV = "cuda"
SMOOTH, MIXED, BLUESTEIN = 0, 1, 2


def _T():
    from dl_cs.mri import transforms as T
    return T


def _kind(n):
    from dl_cs import _lib
    kind = ctypes.c_int(-1)
    _lib.call("dlcs_fft_plan", n, ctypes.byref(kind), None)
    return kind.value


# (Y, X, kind of Y, kind of X); Y != X everywhere, so a swapped plan shows
FFT_CASES = [
    (7, 11, MIXED, MIXED), (13, 7, MIXED, MIXED),                 # one new-radix pass
    (49, 14, MIXED, MIXED),                                       # repeated 7, 7 with 2
    (28, 26, MIXED, MIXED), (77, 91, MIXED, MIXED), (343, 5, MIXED, SMOOTH), (1001, 4, MIXED, SMOOTH),
    (224, 208, MIXED, MIXED),                                     # cine matrix, 7 and 13
    (1, 17, SMOOTH, BLUESTEIN), (31, 37, BLUESTEIN, BLUESTEIN),   # primes
    (34, 62, BLUESTEIN, BLUESTEIN),                               # 2 x a large prime
    (246, 204, BLUESTEIN, BLUESTEIN),                             # cine matrix after crops
    (186, 448, BLUESTEIN, MIXED),                                 # Bluestein columns, radix-7 rows
    (1021, 8, BLUESTEIN, SMOOTH), (8, 1019, SMOOTH, BLUESTEIN),   # padded length 2048: the LDS worst case
]


@pytest.mark.parametrize("Y,X,ky,kx", FFT_CASES)
def test_fft2_vs_numpy(Y, X, ky, kx):
    assert (_kind(Y), _kind(X)) == (ky, kx)
    T = _T()
    x = recipe.crandn(9, (3, Y, X))
    F = T.FFT(2)
    x64 = x.numpy().astype(np.complex128)
    out = F(x.to(DEV)).cpu().numpy()
    err = nrmse(np.fft.fftn(x64, axes=(-1, -2), norm="ortho"), out)
    inv = F(x.to(DEV), adjoint=True).cpu().numpy()
    erri = nrmse(np.fft.ifftn(x64, axes=(-1, -2), norm="ortho"), inv)
    print(f"fft2 {Y}x{X}: forward NRMSE {err:.3e}, inverse {erri:.3e}")
    assert err < FFT_TOL
    assert erri < FFT_TOL


def test_fft2_round_trip():
    T = _T()
    x = recipe.crandn(10, (3, 62, 77))
    F = T.FFT(2)
    back = F(F(x.to(DEV)), adjoint=True).cpu().numpy()
    err = nrmse(x.numpy(), back)
    print(f"fft2 round trip 62x77: NRMSE {err:.3e}")
    assert err < FFT_TOL


def test_fft2_above_1024_still_raises():
    from dl_cs._lib import DlcsError
    T = _T()
    with pytest.raises(DlcsError, match="unsupported size"):
        T.FFT(2)(recipe.crandn(11, (1, 1030, 8)).to(DEV))


def _weights(kind, seed, B, C, Tt, Y, X):
    if kind == "mask":
        return recipe.binary_mask(seed, (B, 1, Tt, Y, X))
    if kind == "coil":
        return recipe.binary_mask(seed, (B, C, Tt, Y, X)) * (1.0 + recipe.crandn(seed + 100, (B, C, Tt, Y, X)).real.abs())
    return None


@pytest.mark.parametrize("shape", [(2, 1, 3, 2, 28, 26), (1, 2, 8, 3, 34, 62)])
@pytest.mark.parametrize("wkind", ["mask", "coil", "none"])
def test_sense_fwd_adj_vs_oracle(shape, wkind):
    T = _T()
    B, E, C, Tt, Y, X = shape
    maps = recipe.sense_maps(1, B, E, C, Y, X)
    w = _weights(wkind, 2, B, C, Tt, Y, X)
    x = recipe.crandn(3, (B, E, Tt, Y, X))
    y = recipe.crandn(4, (B, C, Tt, Y, X))
    A = T.SenseModel(maps.to(DEV), weights=None if w is None else w.to(DEV))
    ef = nrmse(O.sense_forward(x, maps, w).numpy(), A(x.to(DEV)).cpu().numpy())
    ea = nrmse(O.sense_adjoint(y, maps, w).numpy(), A(y.to(DEV), adjoint=True).cpu().numpy())
    print(f"sense {shape} {wkind}: forward NRMSE {ef:.3e}, adjoint {ea:.3e}")
    assert ef < TOL
    assert ea < TOL


def test_adjointness():
    T = _T()
    B, E, C, Tt, Y, X = 1, 2, 4, 3, 62, 77
    maps = recipe.sense_maps(5, B, E, C, Y, X).to(DEV)
    w = recipe.binary_mask(6, (B, 1, Tt, Y, X)).to(DEV)
    A = T.SenseModel(maps, weights=w)
    x = recipe.crandn(7, (B, E, Tt, Y, X)).to(DEV)
    y = recipe.crandn(8, (B, C, Tt, Y, X)).to(DEV)
    lhs = torch.vdot(A(x).reshape(-1).to(torch.complex128), y.reshape(-1).to(torch.complex128))
    rhs = torch.vdot(x.reshape(-1).to(torch.complex128), A(y, adjoint=True).reshape(-1).to(torch.complex128))
    print(f"adjointness 62x77: |lhs - rhs| / |lhs| = {abs(complex(lhs - rhs)) / abs(complex(lhs)):.3e}")
    assert abs(complex(lhs - rhs)) <= 1e-5 * abs(complex(lhs))


@pytest.mark.parametrize("Y,X", [(28, 26), (34, 62)])
def test_normal_dc_and_grad(Y, X):
    T = _T()
    B, E, C, Tt = 1, 2, 3, 4
    maps = recipe.sense_maps(15, B, E, C, Y, X)
    w = recipe.binary_mask(16, (B, 1, Tt, Y, X))
    x = recipe.crandn(17, (B, E, Tt, Y, X))
    aty = recipe.crandn(18, (B, E, Tt, Y, X))
    ref = x + (-2.0) * (O.sense_adjoint(O.sense_forward(x, maps, w), maps, w) - aty)
    A = T.SenseModel(maps.to(DEV), weights=w.to(DEV))
    xg = x.to(DEV).requires_grad_()
    out = A.normal_dc(xg, aty.to(DEV), -2.0)
    ev = nrmse(ref.numpy(), out.detach().cpu().numpy())
    # gradient vs autograd through the oracle
    g = recipe.crandn(19, out.shape)
    (out.real * g.real.to(DEV) + out.imag * g.imag.to(DEV)).sum().backward()
    xo = x.clone().requires_grad_()
    refo = xo + (-2.0) * (O.sense_adjoint(O.sense_forward(xo, maps, w), maps, w) - aty)
    (refo.real * g.real + refo.imag * g.imag).sum().backward()
    eg = nrmse(xo.grad.numpy(), xg.grad.cpu().numpy())
    print(f"normal_dc {Y}x{X}: value NRMSE {ev:.3e}, input gradient {eg:.3e}")
    assert ev < TOL
    assert eg < TOL


def test_normal_and_cg_vs_oracle():
    T = _T()
    B, E, C, Tt, Y, X = 2, 1, 3, 2, 28, 26
    lam = 0.1
    maps = recipe.sense_maps(31, B, E, C, Y, X)
    w = recipe.binary_mask(32, (B, 1, Tt, Y, X))
    x0 = recipe.crandn(33, (B, E, Tt, Y, X))
    b = recipe.crandn(34, (B, E, Tt, Y, X))
    normal = lambda m: O.sense_adjoint(O.sense_forward(m, maps, w), maps, w) + lam * m  # noqa: E731
    A = T.SenseModel(maps.to(DEV), weights=w.to(DEV))
    en = nrmse(normal(x0).numpy(), A.normal(x0.to(DEV), lam).cpu().numpy())
    ec = nrmse(O.conjugate_gradient(normal, x0, b, 10).numpy(), A.cg(x0.to(DEV), b.to(DEV), lam, 10).cpu().numpy())
    print(f"28x26: normal NRMSE {en:.3e}, 10-step CG {ec:.3e}")
    assert en < TOL
    assert ec < TOL


@pytest.fixture
def _fp32():
    from dl_cs.models import swin3D
    old = swin3D.get_compute_dtype()
    swin3D.set_compute_dtype(torch.float32)
    yield
    swin3D.set_compute_dtype(old)


# (28, 26): radix 7 and 13; (22, 31): radix 11 and Bluestein
@pytest.mark.parametrize("Y,X,ky,kx", [(28, 26, MIXED, MIXED), (22, 31, MIXED, BLUESTEIN)])
def test_pgd2_eval_vs_oracle(_fp32, Y, X, ky, kx):
    """The unrolled network end to end (2 unrolls, eval, fp32, 20 frames) on a
    matrix the operator used to refuse; the regularizer takes its
    module-by-module path (token grid inside one window)."""
    assert (_kind(Y), _kind(X)) == (ky, kx)
    from dl_cs.config import get_cfg
    from dl_cs.models import unrolledswin
    T = _T()
    cfg = get_cfg()
    P = cfg.MODEL.PARAMETERS
    P.NUM_UNROLLS, P.NUM_SWINBLOCKS, P.NUM_FEATURES = 2, 1, 160
    P.CONV_BLOCK.COMPLEX, P.FIX_STEP_SIZE = False, True
    model = unrolledswin.ProximalGradientDescent(cfg)
    model.eval()
    recipe.fill_module(model, 41)
    model = model.to(DEV)
    B, E, C, Tt = 1, 2, 8, 20
    maps = recipe.sense_maps(42, B, E, C, Y, X)
    mask = recipe.binary_mask(43, (B, 1, Tt, Y, X))
    y = recipe.crandn(44, (B, C, Tt, Y, X)) * mask
    with torch.no_grad():
        pred = model(y=y.to(DEV), A=T.SenseModel(maps.to(DEV), weights=mask.to(DEV)), x0=None)
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        ref = O.pgd(O.split_unrolls(sd, 2), y, maps, mask)
    err = nrmse(ref.numpy(), pred.cpu().numpy())
    print(f"pgd2 eval {Y}x{X}: NRMSE vs oracle {err:.3e}")
    assert err < TOL
