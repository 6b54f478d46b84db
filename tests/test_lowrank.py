"""dl_cs.mri.lowrank on CPU tensors (the torch path: preprocessing runs in loader
workers) and dl_cs.mri.algorithms.PowerMethod, against tests/golden/dslr.npz and the
float64 oracle.  fp32 torch ops against fp32 reference outputs: 2e-6 (20 roundings)."""
import numpy as np
import pytest
import torch

import dslr_oracle as D
from oracle import recipe

TOL = 2e-6


@pytest.fixture(scope="module")
def g(golden):
    return golden("dslr")


def _op(tag):
    from dl_cs.mri import lowrank
    b, E, T, Y, X = D.GEO_CASES[tag]
    return lowrank.ArrayToBlocks(b, [1, E, T, Y, X], True)


@pytest.mark.parametrize("tag", list(D.GEO_CASES))
def test_geometry_attributes(g, tag):
    op = _op(tag)
    assert [op.pad_x[0], op.pad_x[1], op.pad_y[0], op.pad_y[1], op.nx_pad, op.ny_pad, op.num_blocks_x,
            op.num_blocks_y, op.num_blocks, op.block_stride] == g[f"geo_{tag}"].tolist()
    b, E, T, Y, X = D.GEO_CASES[tag]
    assert tuple(op.win.shape) == (1, E * b * b, 1) and op.win.dtype == torch.float32
    assert tuple(op.weights.shape) == (1, E, T, Y, X) and op.weights.dtype == torch.complex64
    assert sorted(op.state_dict()) == ["weights", "win"]                   # the reference's buffers, no more
    assert D.nrmse(g[f"w_{tag}"], op.weights[0, 0, 0].real.numpy()) <= TOL
    assert D.nrmse(g[f"w_{tag}"], op.weights2d.numpy()) <= TOL


@pytest.mark.parametrize("tag", list(D.GEO_CASES))
def test_cpu_path(g, tag):
    op = _op(tag)
    x, B = D.geo_inputs(tag)
    ext = op(x[None])
    assert D.sampled_err(g, f"ext_{tag}", ext.numpy()) <= TOL
    comb = op(B, adjoint=True)
    assert tuple(comb.shape) == (1,) + tuple(x.shape)
    assert D.nrmse(g[f"comb_{tag}"], comb[0].numpy()) <= TOL
    # the adjoint pairs: <extract x, B> = <x, combine_0 B>, <combine B, x> = <B, extract_1 x>
    dot = lambda a, b: torch.sum(a.to(torch.complex128).conj() * b.to(torch.complex128))
    l1, r1 = dot(ext, B), dot(x[None], op.extract_adjoint(B))
    l2, r2 = dot(comb, x[None]), dot(B, op.combine_adjoint(x[None]))
    assert float((l1 - r1).abs() / l1.abs()) <= 1e-5 and float((l2 - r2).abs() / l2.abs()) <= 1e-5
    if tag == "C":                                                          # weight 0: 0 / 1e-8 = 0, finite
        assert float(comb[0, :, :, 0].abs().max()) == 0.0 and torch.isfinite(torch.view_as_real(comb)).all()


def test_cpu_autograd_matches_oracle():
    """The four Functions on the torch path: gradients of Re <out, W> against the float64 oracle's."""
    from dl_cs.mri import lowrank as lr
    tag = "B"
    op = _op(tag)
    b, E, T, Y, X = D.GEO_CASES[tag]
    geo = D.Geo(b, E, T, Y, X)
    x, B = D.geo_inputs(tag)
    L, R = recipe.crandn(5, (geo.N, E * b * b, 3)), recipe.crandn(6, (geo.N, T, 3))
    c128 = lambda t: t.to(torch.complex128)

    def grads(fn, args, w):
        args = [a.clone().requires_grad_() for a in args]
        torch.sum((fn(*args) * w.conj()).real).backward()
        return [a.grad for a in args]
    todo = [(lambda v: op.extract(v), lambda v: D.extract(geo, v[0]), [x[None]]),
            (lambda v: op.combine(v), lambda v: D.combine(geo, v)[None], [B]),
            (lambda l, r: lr.compose(l, r, op), lambda l, r: D.compose(geo, l, r)[None], [L, R]),
            (lambda v, r: lr.project_l(v, r, op), lambda v, r: D.project_l(geo, v[0], r), [x[None], R]),
            (lambda v, l: lr.project_r(v, l, op), lambda v, l: D.project_r(geo, v[0], l), [x[None], L])]
    for f, f64, args in todo:
        a64 = [c128(a) for a in args]
        w = recipe.crandn(7, tuple(f64(*a64).shape))
        for got, want in zip(grads(f, args, w), grads(f64, a64, c128(w))):
            assert D.nrmse(want.numpy(), got.numpy()) <= 1e-5


def test_overlapping_false_asserts():
    from dl_cs.mri import lowrank
    with pytest.raises(AssertionError):
        lowrank.ArrayToBlocks(4, [1, 1, 3, 8, 8], False)
    with pytest.raises(AssertionError):
        lowrank.Decompose(4, 2, [1, 1, 3, 8, 8], True, device='cuda')


def test_decompose(g):
    """Gauge-free quantities only: L R^H composed to an image, and ||L_k||^2 = ||R_k||^2 = S_k."""
    from dl_cs.mri import lowrank
    b, E, T, Y, X = D.GEO_CASES["A"]
    dec = lowrank.Decompose(b, D.DEC_RANK, [1, E, T, Y, X], True)
    img = D.lowrank_image()[None]
    L, R = dec(img)
    assert tuple(L.shape) == (dec.block_op.num_blocks, E * b * b, D.DEC_RANK)
    assert tuple(R.shape) == (dec.block_op.num_blocks, T, D.DEC_RANK)
    assert D.nrmse(g["dec_S"], (L.abs() ** 2).sum(1).numpy()) <= 1e-5
    assert D.nrmse(g["dec_S"], (R.abs() ** 2).sum(1).numpy()) <= 1e-5
    out = dec((L, R), adjoint=True)
    assert D.nrmse(g["dec_img"], out[0].numpy()) <= 1e-5
    # rank-2 plus 1 % noise: the truncation is the image up to the noise
    assert D.nrmse(img.numpy(), out.numpy()) < 0.05


def test_power_method():
    """sigma_1 = 2 sigma_2: ten iterations leave (1/4)^10 = 1e-6 of the second eigenvector,
    a relative eigenvalue error around 1e-12 -- far below fp32; 1e-4 relative."""
    from dl_cs.mri.algorithms import PowerMethod
    gen = torch.Generator().manual_seed(11)
    A = torch.complex(torch.randn(7, 12, 4, generator=gen), torch.randn(7, 12, 4, generator=gen))
    U, S, Vh = torch.linalg.svd(A, full_matrices=False)
    S = S[:, :1] * torch.tensor([1.0, 0.5, 0.3, 0.1])
    A = (U * S[:, None, :]) @ Vh
    pm = PowerMethod(num_iter=10)
    v0 = torch.ones(7, 4, 1, dtype=torch.complex64)
    ev = pm(A, v0=v0)
    assert tuple(ev.shape) == (7,)
    assert float(((ev - S[:, 0] ** 2).abs() / S[:, 0] ** 2).max()) <= 1e-4
    torch.manual_seed(0)
    ev2 = pm(A)                                                             # the reference's random start
    assert float(((ev2 - S[:, 0] ** 2).abs() / S[:, 0] ** 2).max()) <= 1e-4
    assert torch.equal(pm(A, v0=v0), ev)


def test_preprocess_lr_decom_cpu():
    """CinePreprocess(lr_decom=True) on CPU tensors: the reference's 8-tuple, with L R^H
    composing back to the rank-r truncation of init_image's blocks."""
    import types
    from dl_cs.data.preprocess import CinePreprocess
    from dl_cs.mri import lowrank
    N = types.SimpleNamespace
    cfg = N(AUG_TRAIN=N(UNDERSAMPLE=N(ACCELERATIONS=(4, 6), PARTIAL_KX=0.25, PARTIAL_KY=0.25), CROP_READOUT=0, ZPAD_PE=0),
            MODEL=N(PARAMETERS=N(SLWIN_INIT=True, DSLR=N(BLOCK_SIZE=4, NUM_BASIS=2, OVERLAPPING=True))))
    C, T, Y, X, E = 3, 6, 12, 10, 2
    k = recipe.crandn(1, (C, T, Y, X)).numpy()
    maps = recipe.sense_maps(2, 1, E, C, Y, X)[0].numpy()
    target = recipe.crandn(3, (E, T, Y, X)).numpy()
    six = CinePreprocess(cfg, use_seed=True)(k, maps, target, "slice.h5")
    eight = CinePreprocess(cfg, lr_decom=True, use_seed=True)(k, maps, target, "slice.h5")
    assert len(six) == 6 and len(eight) == 8
    masked, mask, mp, L, R, init, scale, tgt = eight
    for a, b in zip(six, (masked, mask, mp, init, scale, tgt)):            # the other six items are unchanged
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))
    op = lowrank.ArrayToBlocks(4, [1, E, T, Y, X], True)
    assert tuple(L.shape) == (op.num_blocks, E * 16, 2) and tuple(R.shape) == (op.num_blocks, T, 2)
    U, S, Vh = torch.linalg.svd(op(init[None]).to(torch.complex128), full_matrices=False)
    trunc = (U[:, :, :2] * S[:, None, :2]) @ Vh[:, :2]
    assert D.nrmse(trunc.numpy(), torch.bmm(L, R.conj().transpose(1, 2)).numpy()) <= 1e-5
