"""DiTResNet / DiTNet on grids the (2, 4, 4) patch does not divide (dit_engine "Any grid
size": tokens of the reference's token grid only, zeros where the reference pads, unpatchify2's
centre crop as dlcs_box_shift) vs the reference's own outputs (tests/golden/dit_anygrid.npz)
and the fp32 / float64 oracle (oracle/dit_oracle.py).

Tolerances, those of tests/test_gpu_dit.py: outputs and input gradients vs the reference
NRMSE < 1e-5; input and parameter gradients at the float64 floor (goldutil: max(1e-5, 4 x the
fp32 oracle's own NRMSE vs float64), DiTResNet with the HIP forward's final-ReLU decisions);
fp8 inference within its 5e-2 budget."""
import pytest
import torch

import dit_anygrid_cases as AC
from goldutil import assert_f64_floor, assert_masked_f64, golden_err, nrmse, oracle_grads
from oracle import dit_oracle as DO
from oracle import dlcs_oracle as O
from oracle import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAGS = ["ditres", "ditnet"]
ODD = (2, 5, 10, 9)                       # Tp = 9: all three axes padded, shifts (1, 1, 2), two items
_ids = lambda c: "x".join(map(str, c))    # noqa: E731


@pytest.fixture(scope="module")
def nets():
    return {tag: AC.build(tag).to(DEV) for tag in TAGS}


@pytest.fixture(scope="module")
def tabs():
    return AC.tables("ditres")


def _cast_tabs(tabs, dt):
    return {k: v.to(dt) for k, v in tabs.items()}


def _run(net, tag, case):
    """One forward + backward of the fixture's loss: (y, x with its grad, captures)."""
    net.zero_grad(set_to_none=True)
    x, t, lab, gr = AC.inputs(tag, case)
    xg = x.to(DEV).requires_grad_()
    y, caps = AC.captured(lambda: net(xg, t.to(DEV), lab.to(DEV)))
    (y.real * gr.real.to(DEV) + y.imag * gr.imag.to(DEV)).sum().backward()
    return y, xg, caps


@pytest.mark.parametrize("case", AC.CASES, ids=_ids)
@pytest.mark.parametrize("tag", TAGS)
def test_vs_reference(golden, nets, tabs, tag, case):
    """Output and dx vs the reference's; input and parameter gradients at the float64 floor."""
    g = golden("dit_anygrid")
    net = nets[tag]
    y, xg, caps = _run(net, tag, case)
    ey, edx = golden_err(g, AC.key(tag, case) + "y", y), golden_err(g, AC.key(tag, case) + "dx", xg.grad)
    print(f"{tag} {case}: y {ey:.3g}, dx {edx:.3g} vs the reference")
    assert ey < 1e-5
    assert edx < 1e-5
    x, t, lab, gr = AC.inputs(tag, case)
    xkey = "__x__"
    sd = dict(net.state_dict())
    sd[xkey] = x
    tr = lambda k: k == xkey or AC.trainable(k)                          # noqa: E731

    def lf(P, c, mk):
        yo = AC.oracle(tag, P, P[xkey], t, lab, _cast_tabs(tabs, P["DiT.t_embedder.mlp.0.weight"].dtype),
                       relu=mk.relu() if mk is not None else None)
        gc = c(gr)
        return (yo.real * gc.real + yo.imag * gc.imag).sum()
    hip = {n: p.grad for n, p in net.named_parameters() if p.grad is not None and AC.trainable(n)}
    hip[xkey] = xg.grad
    label = f"{tag} {_ids(case)}"
    if tag == "ditres":
        assert len(caps) == 1 and ("box" in caps[0]) == (case != AC.CASES[0])
        assert_masked_f64(hip, lf, sd, tr, AC.hip_masks(caps), label)
    else:
        o32, o64 = (oracle_grads(lambda P, c: lf(P, c, None), sd, dt, tr) for dt in (torch.float32, torch.float64))
        assert_f64_floor(hip, o32, o64, label)


@pytest.mark.parametrize("tag", TAGS)
def test_two_items_that_differ(nets, tabs, tag):
    """B = 2 at (5, 10, 9) with different items and timesteps, each item against the oracle's
    single-item call: an error in the batch strides of the padded grid, or a slack subpatch
    that became a token (attention would mix it in), shows in one item or the other."""
    net = nets[tag]
    x, t, lab, _ = AC.inputs(tag, ODD)
    with torch.no_grad():
        y = net(x.to(DEV), t.to(DEV), lab.to(DEV)).cpu()
        P = {k: v.detach().cpu() for k, v in net.state_dict().items()}
        for b in range(2):
            ref = AC.oracle(tag, P, x[b:b + 1], t[b:b + 1], lab[b:b + 1], tabs)
            assert nrmse(ref.numpy(), y[b:b + 1].numpy()) < 1e-5, b
    assert nrmse(y[0].numpy(), y[1].numpy()) > 0.1


@pytest.mark.parametrize("tag", TAGS)
def test_identical_calls_identical_bits(nets, tag):
    net = nets[tag]
    y1, x1, _ = _run(net, tag, ODD)
    y2, x2, _ = _run(net, tag, ODD)
    assert torch.equal(torch.view_as_real(y1), torch.view_as_real(y2))
    assert torch.equal(torch.view_as_real(x1.grad), torch.view_as_real(x2.grad))


@pytest.mark.parametrize("tag", TAGS)
def test_no_slack_launches_no_box_kernel(nets, tag, monkeypatch):
    """(4, 8, 8) (Tp = 8): forward and backward with every box wrapper of _ops replaced by one
    that raises -- without slack the launches are those of the dlcs_swin_* path."""
    from dl_cs.models import _ops as K

    def refuse(*a, **k):
        raise AssertionError("a box kernel was called on a grid without slack")
    for name in ("box_shift", "box_zero", "box_pre", "box_pre_bwd", "box_post", "box_post_bwd"):
        monkeypatch.setattr(K, name, refuse)
    y, xg, _ = _run(nets[tag], tag, AC.CASES[0])
    assert bool(torch.isfinite(torch.view_as_real(xg.grad)).all())


def test_shift_launched_only_when_nonzero(nets, monkeypatch):
    """(6, 8, 8): Tp = 10 has slack (a half block of the padded grid is no token) but the
    reference pads nothing, so no shift: box_zero runs, box_shift does not."""
    from dl_cs.models import _ops as K
    calls = []
    zero = K.box_zero
    monkeypatch.setattr(K, "box_zero", lambda *a, **k: (calls.append(1), zero(*a, **k))[1])
    monkeypatch.setattr(K, "box_shift", lambda *a, **k: pytest.fail("box_shift without a shift"))
    _run(nets["ditres"], "ditres", (1, 6, 8, 8))
    assert calls


def test_pgd2_training_step(tabs):
    """unrolledDiT.ProximalGradientDescent, 2 unrolls, at (5, 10, 9): prediction vs DO.pgd in
    float64, gradients at the masked float64 floor (as test_gpu_dit.test_dit_pgd2_training_step)."""
    from dl_cs.models import unrolledDiT
    from dl_cs.mri import transforms as T
    from test_oracle_dit import dit_config
    B, E, C, Tt, Y, X = 1, 2, 4, 5, 10, 9
    model = unrolledDiT.ProximalGradientDescent(dit_config(2))
    model.eval()
    recipe.fill_module(model, 311)
    model = model.to(DEV)
    maps = recipe.sense_maps(312, B, E, C, Y, X)
    mask = recipe.binary_mask(313, (B, 1, Tt, Y, X))
    yk = recipe.crandn(314, (B, C, Tt, Y, X)) * mask
    target = recipe.crandn(315, (B, E, Tt, Y, X))
    t, lab = torch.tensor([37]), torch.tensor([1])
    A = T.SenseModel(maps.to(DEV), weights=mask.to(DEV))
    x0 = A(yk.to(DEV), adjoint=True)
    pred, caps = AC.captured(lambda: model(x0, t.to(DEV), A, lab.to(DEV)))
    torch.mean(torch.abs(target.to(DEV) - pred)).backward()
    assert len(caps) == 2 and all(c["box"] == (1, 9, 10, 9) for c in caps)
    masks = AC.hip_masks(caps)

    def predict(P, c, mk):
        xo = O.sense_adjoint(c(yk), c(maps), c(mask))
        return DO.pgd(DO.split_unrolls(P, 2), xo, t, lab, c(maps), c(mask), 2, 16,
                      pos_table=tabs["pos_table"].to(P["step_size"].dtype), relus=mk.relu)
    with torch.no_grad():
        P64 = {k: (v.detach().cpu().double() if torch.is_floating_point(v) else v.detach().cpu())
               for k, v in model.state_dict().items()}
        c64 = lambda v: v.to(torch.complex128) if v.is_complex() else v.double()    # noqa: E731
        ref = predict(P64, c64, masks)
    err = nrmse(ref.numpy(), pred.detach().cpu().numpy())
    print(f"dit pgd2 (5, 10, 9): prediction vs the float64 oracle {err:.3g}")
    assert err < 1e-5
    named = dict(model.named_parameters())
    assert_masked_f64({n: p.grad for n, p in named.items() if p.grad is not None and AC.trainable(n)},
                      lambda P, c, mk: torch.mean(torch.abs(c(target) - predict(P, c, mk))),
                      model.state_dict(), AC.trainable, masks, "dit pgd2 (5, 10, 9)")


def test_fp8_inference(nets, tabs):
    """set_fp8(True) at (5, 10, 9): the blocks' token Linears on fp8 MFMAs, NRMSE vs the fp32
    oracle within the 5e-2 budget of test_gpu_dit.test_dit_fp8_inference; nothing in the fp8
    path looks at the grid."""
    from dl_cs.models import _ops as K
    from dl_cs.models import dit_engine
    net = nets["ditres"]
    x, t, lab, _ = AC.inputs("ditres", ODD)
    P = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    with torch.no_grad():
        ref = AC.oracle("ditres", P, x, t, lab, tabs)
    calls = []
    orig = K.linear_f8r
    dit_engine.set_fp8(True)
    try:
        K.linear_f8r = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        with torch.no_grad():
            y8 = net(x.to(DEV), t.to(DEV), lab.to(DEV)).cpu()
    finally:
        K.linear_f8r = orig
        dit_engine.set_fp8(False)
    err8 = nrmse(ref.numpy(), y8.numpy())
    print(f"DiTResNet (5, 10, 9) x 2 fp8 inference NRMSE vs the fp32 oracle {err8:.3g} ({len(calls)} fp8 GEMMs)")
    assert len(calls) > 0 and err8 < 5e-2
