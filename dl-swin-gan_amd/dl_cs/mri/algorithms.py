"""Conjugate gradient for the HQS / MoDL / DSLR solvers and the power method of the
DSLR step sizes (alg = dl_cs/mri/algorithms.py:11-102).

The normal operator A passed in runs on the HIP SENSE (and low-rank block) kernels; the
CG vector updates are device tensor ops (HQS is SURVEY 8(f) rank 3, not the PGD hot
path).  The power method works on r x r matrices and stays in torch ops.
"""
import torch
from torch import nn


class ConjugateGradient(nn.Module):
    """Solve A x = y for Hermitian positive-definite A with `num_iter` CG steps."""

    def __init__(self, A, num_iter, dbprint=False):
        super().__init__()
        self.A = A
        self.num_iter = num_iter
        self.dbprint = dbprint

    @staticmethod
    def zdot(x1, x2):
        return torch.sum(x1.conj() * x2)

    def zdot_single(self, x):
        return self.zdot(x, x).real

    def forward(self, x, y):
        r = y - self.A(x)
        rsold = self.zdot_single(r)
        p = r
        for i in range(self.num_iter):
            Ap = self.A(p)
            alpha = rsold / self.zdot(p, Ap)
            x = x + alpha * p
            r = r - alpha * Ap
            rsnew = self.zdot_single(r)
            p = (rsnew / rsold) * p + r
            rsold = rsnew
            if self.dbprint:
                print(f"CG Iteration {i}: {float(rsnew)}")
        return x


class PowerMethod(nn.Module):
    """alg:76-102 -- the largest eigenvalue of A^H A for a batch of matrices A [n, m, k],
    by num_iter normalised power iterations.  v0 [n, k, 1] is the start vector; None
    draws it from torch.rand as the reference does."""

    def __init__(self, num_iter, eps=1e-6):
        super().__init__()
        self.num_iter = num_iter
        self.eps = eps

    def forward(self, A, v0=None):
        batch_size, m, n = A.shape
        if v0 is None:
            v0 = torch.rand((batch_size, n, 1), dtype=torch.complex64, device=A.device)
        v = v0.to(device=A.device, dtype=A.dtype)
        AhA = torch.bmm(A.conj().permute(0, 2, 1), A)
        for _ in range(self.num_iter):
            v = torch.bmm(AhA, v)
            eigenvals = (torch.abs(v) ** 2).sum(1).sqrt()
            v = v / (eigenvals.reshape(batch_size, 1, 1) + self.eps)
        return eigenvals.reshape(batch_size)
