"""LatteNet on grids the (4, 4) patch, or the 4-frame block of the layout, does not divide
(latte_engine "Any grid size": the reference's F frames of ceil(Y/4) x ceil(X/4) patches as
tokens, zeros where the reference pads, unpatchify2's centre crop as dlcs_box_shift) vs the
reference's own outputs (tests/golden/dit_anygrid.npz) and the fp32 / float64 oracle
(oracle/dit_oracle.py latte_*).

Tolerances, those of tests/test_gpu_latte.py: outputs and input gradients vs the reference
NRMSE < 1e-5; input and parameter gradients at the float64 floor (goldutil.assert_f64_floor:
max(1e-5, 4 x the fp32 oracle's own NRMSE vs float64); LatteNet has no ReLU); fp8 inference
within its 5e-2 budget."""
import pytest
import torch

import dit_anygrid_cases as AC
from goldutil import assert_f64_floor, golden_err, nrmse, oracle_grads
from oracle import dit_oracle as DO
from oracle import dlcs_oracle as O
from oracle import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAG = "latte"
ODD = (2, 5, 10, 9)                       # 9 frames in 12, pads (2, 3), shifts (1, 2), two items
_ids = lambda c: "x".join(map(str, c))    # noqa: E731


@pytest.fixture(scope="module")
def net():
    return AC.build(TAG).to(DEV)


@pytest.fixture(scope="module")
def tabs():
    return AC.tables(TAG)


def _cast_tabs(tabs, dt):
    return {k: v.to(dt) for k, v in tabs.items()}


def _run(net, case):
    net.zero_grad(set_to_none=True)
    x, t, lab, gr = AC.inputs(TAG, case)
    xg = x.to(DEV).requires_grad_()
    y = net(xg, t.to(DEV), lab.to(DEV))
    (y.real * gr.real.to(DEV) + y.imag * gr.imag.to(DEV)).sum().backward()
    return y, xg


@pytest.mark.parametrize("case", AC.CASES, ids=_ids)
def test_vs_reference(golden, net, tabs, case):
    """Output and dx vs the reference's; input and parameter gradients at the float64 floor."""
    g = golden("dit_anygrid")
    y, xg = _run(net, case)
    ey, edx = golden_err(g, AC.key(TAG, case) + "y", y), golden_err(g, AC.key(TAG, case) + "dx", xg.grad)
    print(f"latte {case}: y {ey:.3g}, dx {edx:.3g} vs the reference")
    assert ey < 1e-5
    assert edx < 1e-5
    x, t, lab, gr = AC.inputs(TAG, case)
    xkey = "__x__"
    sd = dict(net.state_dict())
    sd[xkey] = x

    def lf(P, c):
        yo = AC.oracle(TAG, P, P[xkey], t, lab, _cast_tabs(tabs, P["Latte.t_embedder.mlp.0.weight"].dtype))
        gc = c(gr)
        return (yo.real * gc.real + yo.imag * gc.imag).sum()
    hip = {n: p.grad for n, p in net.named_parameters() if p.grad is not None and AC.trainable(n)}
    hip[xkey] = xg.grad
    o32, o64 = (oracle_grads(lf, sd, dt, AC.trainable) for dt in (torch.float32, torch.float64))
    assert_f64_floor(hip, o32, o64, f"latte {_ids(case)}")


def test_two_items_that_differ(net, tabs):
    """B = 2 at (5, 10, 9) with different items and timesteps, each item against the oracle's
    single-item call: an error in the batch strides of the padded grid, or a slack frame that
    became a token (temporal attention would mix it in), shows in one item or the other."""
    x, t, lab, _ = AC.inputs(TAG, ODD)
    with torch.no_grad():
        y = net(x.to(DEV), t.to(DEV), lab.to(DEV)).cpu()
        P = {k: v.detach().cpu() for k, v in net.state_dict().items()}
        for b in range(2):
            ref = AC.oracle(TAG, P, x[b:b + 1], t[b:b + 1], lab[b:b + 1], tabs)
            assert nrmse(ref.numpy(), y[b:b + 1].numpy()) < 1e-5, b
    assert nrmse(y[0].numpy(), y[1].numpy()) > 0.1


def test_identical_calls_identical_bits(net):
    y1, x1 = _run(net, ODD)
    y2, x2 = _run(net, ODD)
    assert torch.equal(torch.view_as_real(y1), torch.view_as_real(y2))
    assert torch.equal(torch.view_as_real(x1.grad), torch.view_as_real(x2.grad))


def test_no_slack_launches_no_box_kernel(net, monkeypatch):
    """(4, 8, 8) (8 frames): forward and backward with every box wrapper of _ops replaced by one
    that raises -- without slack the launches are those of the dlcs_swin_* path."""
    from dl_cs.models import _ops as K

    def refuse(*a, **k):
        raise AssertionError("a box kernel was called on a grid without slack")
    for name in ("box_shift", "box_zero", "box_pre", "box_pre_bwd", "box_post", "box_post_bwd"):
        monkeypatch.setattr(K, name, refuse)
    y, xg = _run(net, AC.CASES[0])
    assert bool(torch.isfinite(torch.view_as_real(xg.grad)).all())


def test_shift_launched_only_when_nonzero(net, monkeypatch):
    """(6, 8, 8): 10 frames in 12 (two slack frames that are no tokens) but Y and X unpadded,
    so no shift: box_shift is not launched."""
    from dl_cs.models import _ops as K
    monkeypatch.setattr(K, "box_shift", lambda *a, **k: pytest.fail("box_shift without a shift"))
    _run(net, (1, 6, 8, 8))


def test_pgd2_training_step(tabs):
    """unrolledLatte.ProximalGradientDescent, 2 unrolls, at (5, 10, 9): prediction vs
    DO.latte_pgd in float64, gradients at the float64 floor."""
    from dl_cs.models import unrolledLatte
    from dl_cs.mri import transforms as T
    from test_oracle_latte import latte_config
    B, E, C, Tt, Y, X = 1, 2, 4, 5, 10, 9
    model = unrolledLatte.ProximalGradientDescent(latte_config(2))
    model.eval()
    recipe.fill_module(model, 511)
    model = model.to(DEV)
    maps = recipe.sense_maps(512, B, E, C, Y, X)
    mask = recipe.binary_mask(513, (B, 1, Tt, Y, X))
    yk = recipe.crandn(514, (B, C, Tt, Y, X)) * mask
    target = recipe.crandn(515, (B, E, Tt, Y, X))
    t, lab = torch.tensor([37]), torch.tensor([1])
    A = T.SenseModel(maps.to(DEV), weights=mask.to(DEV))
    x0 = A(yk.to(DEV), adjoint=True)
    pred = model(x0, t.to(DEV), A, lab.to(DEV))
    torch.mean(torch.abs(target.to(DEV) - pred)).backward()

    def predict(P, c):
        dt = P["step_size"].dtype
        xo = O.sense_adjoint(c(yk), c(maps), c(mask))
        return DO.latte_pgd(DO.split_unrolls(P, 2), xo, t, c(maps), c(mask), 2, 6, **_cast_tabs(tabs, dt))
    with torch.no_grad():
        P64 = {k: (v.detach().cpu().double() if torch.is_floating_point(v) else v.detach().cpu())
               for k, v in model.state_dict().items()}
        ref = predict(P64, lambda v: v.to(torch.complex128) if v.is_complex() else v.double())
    err = nrmse(ref.numpy(), pred.detach().cpu().numpy())
    print(f"latte pgd2 (5, 10, 9): prediction vs the float64 oracle {err:.3g}")
    assert err < 1e-5
    lf = lambda P, c: torch.mean(torch.abs(c(target) - predict(P, c)))              # noqa: E731
    o32, o64 = (oracle_grads(lf, model.state_dict(), dt, AC.trainable) for dt in (torch.float32, torch.float64))
    named = dict(model.named_parameters())
    assert_f64_floor({n: p.grad for n, p in named.items() if p.grad is not None and AC.trainable(n)}, o32, o64,
                     "latte pgd2 (5, 10, 9)")


def test_fp8_inference(net, tabs):
    """set_fp8(True) at (5, 10, 9): NRMSE vs the fp32 oracle within the 5e-2 budget of
    test_gpu_latte.test_latte_full_slice_forward."""
    from dl_cs.models import dit_engine
    x, t, lab, _ = AC.inputs(TAG, ODD)
    P = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    with torch.no_grad():
        ref = AC.oracle(TAG, P, x, t, lab, tabs)
        dit_engine.set_fp8(True)
        try:
            y8 = net(x.to(DEV), t.to(DEV), lab.to(DEV)).cpu()
        finally:
            dit_engine.set_fp8(False)
    err8 = nrmse(ref.numpy(), y8.numpy())
    print(f"LatteNet (5, 10, 9) x 2 fp8 inference NRMSE vs the fp32 oracle {err8:.3g}")
    assert err8 < 5e-2
