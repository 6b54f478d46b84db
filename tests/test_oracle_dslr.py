"""Pins the float64 DSLR oracle (tests/dslr_oracle.py) to the reference's outputs in
tests/golden/dslr.npz (CPU).  The reference ran in fp32 for the operator cases, and its
float64 network runs still carry an fp32 window and fp32 weights, so the oracle sits
about 1e-7 from the fixtures; the bound is 2e-6 throughout (20 fp32 roundings)."""
import numpy as np
import pytest
import torch

import dslr_oracle as D

TOL = 2e-6


@pytest.fixture(scope="module")
def g(golden):
    return golden("dslr")


@pytest.mark.parametrize("tag", list(D.GEO_CASES))
def test_operators(g, tag):
    b, E, T, Y, X = D.GEO_CASES[tag]
    geo = D.Geo(b, E, T, Y, X)
    assert [geo.px[0], geo.px[1], geo.py[0], geo.py[1], geo.Xp, geo.Yp, geo.nbx, geo.nby, geo.N, geo.s] == \
        g[f"geo_{tag}"].tolist()
    assert D.nrmse(g[f"w_{tag}"], geo.weights.numpy()) <= TOL
    x, B = D.geo_inputs(tag)
    assert D.sampled_err(g, f"ext_{tag}", D.extract(geo, x.to(torch.complex128)).numpy()) <= TOL
    assert D.nrmse(g[f"comb_{tag}"], D.combine(geo, B.to(torch.complex128)).numpy()) <= TOL
    if tag == "C":
        assert float(geo.weights[0].abs().max()) == 0.0 and float(np.abs(g["comb_C"][:, :, 0]).max()) == 0.0


def test_decompose(g):
    b, E, T, Y, X = D.GEO_CASES["A"]
    geo = D.Geo(b, E, T, Y, X)
    L, R, S = D.decompose(geo, D.lowrank_image().to(torch.complex128), D.DEC_RANK)
    assert D.nrmse(g["dec_S"], S[:, :D.DEC_RANK].numpy()) <= TOL
    assert D.nrmse(g["dec_S"], (L.abs() ** 2).sum(1).numpy()) <= TOL            # ||L_k||^2 = S_k
    assert D.nrmse(g["dec_img"], D.compose(geo, L, R).numpy()) <= 1e-5         # fp32 SVD in the reference


@pytest.mark.parametrize("arch", D.ARCHS)
def test_networks(g, arch):
    pred, loss, grads = D.oracle_run(g, arch)
    e = D.nrmse(g[f"{arch}_pred"], pred.numpy())
    names = [str(n) for n in g[f"{arch}_grad_names"]]
    assert sorted(grads) == names
    cat = np.concatenate([grads[n].numpy().reshape(-1) for n in names])
    eg = D.nrmse(g[f"{arch}_grad_sample"], cat[D.sample_index(cat.size)])
    norms = np.array([float(grads[n].norm()) for n in names])
    en = float(np.max(np.abs(norms - g[f"{arch}_grad_norms"]) / np.linalg.norm(g[f"{arch}_grad_norms"])))
    print(f"{arch}: oracle vs reference: output {e:.3g}, gradient sample {eg:.3g}, norms {en:.3g}")
    assert abs(loss - float(g[f"{arch}_loss"])) <= TOL * abs(loss)
    assert e <= TOL and eg <= TOL and en <= TOL
    fl = g[f"{arch}_floor"]
    assert fl.shape == (2,) and float(fl.max()) < 2.5e-6
