"""Inputs, float64 references and the shared checks of the block SVD tests
(tests/test_gpu_block_svd.py on the GPU, tests/test_block_svd_host.py for the
preconditions).

Shapes (b, E, T, Y, X, r); two images per shape from oracle.recipe.crandn:
  lowrank  sum over k < r of 0.75^k u_k(e, y, x) v_k(t) + 0.01 noise
  gauss    plain complex Gaussian
The reference is torch.linalg.svd of dslr_oracle.extract in complex128, computed once per
(shape, image) and shared (functools.lru_cache): the tests only read it.
"""
import functools

import torch

import dslr_oracle as D
from oracle import recipe

CASES = {
    "A": (4, 2, 8, 12, 20, 3),
    "B": (4, 2, 5, 9, 13, 3),            # odd T and sizes, a bye, a one-pixel corner block of rank 2 < r
    "C": (4, 1, 3, 11, 14, 2),
    "b8": (8, 2, 6, 16, 24, 4),
    "b16": (16, 2, 20, 32, 48, 8),       # the shipped block
    "t32": (16, 2, 32, 24, 16, 8),       # the LDS maximum
    "full": (4, 1, 3, 8, 8, 3),          # r = T
}
KINDS = ("lowrank", "gauss")
GAP = 0.02                               # a compared vector's sigma is this far (times sigma_1) from its neighbours
MAX_LEFT_OUT = 0.20


def image(name, kind):
    """[E, T, Y, X] complex64."""
    b, E, T, Y, X, r = CASES[name]
    i = list(CASES).index(name)
    if kind == "gauss":
        return recipe.crandn(703 + 10 * i, (E, T, Y, X))
    u = recipe.crandn(700 + 10 * i, (r, E, 1, Y, X)).to(torch.complex128)
    v = recipe.crandn(701 + 10 * i, (r, 1, T, 1, 1)).to(torch.complex128)
    s = (0.75 ** torch.arange(r, dtype=torch.float64)).reshape(r, 1, 1, 1, 1)
    return ((s * u * v).sum(0) + 0.01 * recipe.crandn(702 + 10 * i, (E, T, Y, X))).to(torch.complex64)


def svd64(b, img):
    """(U, S, Vh) in float64 of every block of img [E, T, Y, X]."""
    E, T, Y, X = img.shape
    geo = D.Geo(b, E, T, Y, X)
    return torch.linalg.svd(D.extract(geo, img.to(torch.complex128)), full_matrices=False)


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    return svd64(CASES[name][0], image(name, kind))


def truncation(ref, r):
    U, S, Vh = ref
    return (U[:, :, :r] * S[:, None, :r]) @ Vh[:, :r]


def compared(S, r):
    """[N, r] bool: the components whose vectors are compared -- sigma_k at least GAP sigma_1
    away from sigma_{k-1} and from sigma_{k+1} (sigma_{r+1} included where the block has one).
    A component whose float64 sigma_k is below 2^-20 sigma_1 (null by the kernel's own rule:
    sigma^2 <= 2^-40 of the largest) has no vector to compare -- the reference's is sqrt(1e-17)
    times an arbitrary direction -- and counts as left out; with r = T it has no sigma_{r+1}
    beside it, so the gap rule alone would keep it."""
    s1 = S[:, :1]
    d = (S[:, :-1] - S[:, 1:])                                   # [N, K - 1], d[k] = sigma_k - sigma_{k+1}
    big = torch.full_like(s1, float("inf"))
    below = torch.cat((d, big), dim=1)[:, :r]                    # to the next one (none after the last column)
    above = torch.cat((big, d), dim=1)[:, :r]
    return (below >= GAP * s1) & (above >= GAP * s1) & (S[:, :r] > 2.0 ** -20 * s1)


# ------------------------------------------------------------------ the checks (every tensor on the CPU)
def check_truncation(ref, r, L, R, S, info, label=""):
    """Check 1 of the issue: truncation NRMSE, singular values, balance, finite, sweeps < 30."""
    S64 = ref[1]
    L, R = L.to(torch.complex128), R.to(torch.complex128)
    S = S.to(torch.float64)
    assert all(bool(torch.isfinite(torch.view_as_real(t)).all()) for t in (L, R)) and bool(torch.isfinite(S).all())
    e = D.nrmse(truncation(ref, r).numpy(), torch.bmm(L, D.bt(R)).numpy())
    s1 = S64[:, :1]
    live = s1[:, 0] > 0
    es = float(((S - S64[:, :r]).abs()[live] / s1[live]).max()) if bool(live.any()) else 0.0
    assert bool((S[~live] == 0).all())
    smax = S.max(dim=1, keepdim=True).values
    bl = float((((L.abs() ** 2).sum(1) - S).abs() - 2e-5 * smax).max())
    br = float((((R.abs() ** 2).sum(1) - S).abs() - 2e-5 * smax).max())
    bal = max(float((((L.abs() ** 2).sum(1) - S).abs()[live] / smax[live]).max()),
              float((((R.abs() ** 2).sum(1) - S).abs()[live] / smax[live]).max())) if bool(live.any()) else 0.0
    print(f"{label}: truncation NRMSE {e:.3g}, S error / sigma_1 {es:.3g}, balance / max S {bal:.3g}, "
          f"sweeps {int(info.min())}..{int(info.max())}")
    assert e <= 1e-5
    assert es <= 1e-5
    assert bl <= 0 and br <= 0
    assert int(info.max()) < 30 and int(info.min()) >= 1


def vector_errors(ref, r, L, R):
    """Check 2: ([N, r] relative error of the phase-aligned stacked column [L_k; R_k], the
    [N, r] mask of compared components)."""
    U, S64, Vh = ref
    sq = S64[:, None, :r].sqrt()
    want = torch.cat((U[:, :, :r] * sq, D.bt(Vh)[:, :, :r] * sq), dim=1)          # [N, M + T, r]
    got = torch.cat((L, R), dim=1).to(torch.complex128)
    ip = (want.conj() * got).sum(1, keepdim=True)                                 # <ref, got>
    phase = ip / ip.abs().clamp_min(1e-300)
    err = (got * phase.conj() - want).norm(dim=1) / want.norm(dim=1).clamp_min(1e-300)
    return err, compared(S64, r)


def left_out_share(name, kind="lowrank"):
    r = CASES[name][5]
    return 1.0 - float(compared(reference(name, kind)[1], r).double().mean())
