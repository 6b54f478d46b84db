"""HIP unrolled SE-ResNet (MODEL_TYPE 'SE'; dl_cs/models/unrolledSE.py, se3d.py) vs the
reference's own outputs (tests/golden/se.npz) and the CPU restatement
tests/se_oracle.py: test_gpu_resnet.py transposed to the SE family.  Outputs
NRMSE <= 1e-5; gradients held to the float64 floor with the HIP forward's ReLU
decisions (goldutil.assert_masked_f64: max(1e-5, 4 x the fp32 oracle's own floor))."""
import importlib.util
import os

import pytest
import torch

import se_oracle
from goldutil import HipMasks, assert_masked_f64, golden_err, grad_keys
from oracle import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(n, feats=64, rr=16):
    from dl_cs.config import get_cfg
    cfg = get_cfg()
    cfg.MODEL.MODEL_TYPE = "SE"
    P = cfg.MODEL.PARAMETERS
    P.NUM_UNROLLS, P.NUM_RESBLOCKS, P.NUM_FEATURES, P.NUM_EMAPS, P.RR = n, 2, feats, 1, rr
    P.CONV_BLOCK.COMPLEX, P.FIX_STEP_SIZE = False, True
    return cfg


def _model(n, seed, hqs=False):
    from dl_cs.models import unrolledSE
    m = (unrolledSE.HalfQuadraticSplitting if hqs else unrolledSE.ProximalGradientDescent)(_cfg(n))
    m.eval()
    recipe.fill_module(m, seed)
    assert se_oracle.scale_fc_weights(m) == 4 * n                # the fixtures' x8 on the SE FC weights
    return m.to(DEV)


_STEP = {}


def _golden_step():
    """One 2-unroll training step at the fixture's sizes and seeds (fill 81, data 82-85):
    computed once, shared by the golden and the determinism tests, left unchanged."""
    if _STEP:
        return _STEP
    from dl_cs.models import engine, swin3D
    from dl_cs.mri import transforms as T
    swin3D.set_compute_dtype(torch.float32)
    B, E, C, Tt, Y, X = 1, 1, 8, 20, 32, 32
    model = _model(2, 81)
    maps = recipe.sense_maps(82, B, E, C, Y, X).to(DEV)
    mask = recipe.binary_mask(83, (B, 1, Tt, Y, X))
    y = (recipe.crandn(84, (B, C, Tt, Y, X)) * mask).to(DEV)
    target = recipe.crandn(85, (B, E, Tt, Y, X)).to(DEV)

    def step(capture):
        model.zero_grad(set_to_none=True)
        engine.CAPTURE = [] if capture else None
        try:
            pred = model(y=y, A=T.SenseModel(maps, weights=mask.to(DEV)), x0=None)
        finally:
            caps, engine.CAPTURE = engine.CAPTURE, None
        loss = torch.mean(torch.abs(target - pred))
        loss.backward()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        return pred.detach().clone(), loss.detach().clone(), grads, caps

    _STEP.update(model=model, maps=maps, mask=mask, y=y, target=target, first=step(True), step=step)
    return _STEP


def test_se_pgd2_training_step(golden):
    from oracle import dlcs_oracle as O
    g = golden("se")
    st = _golden_step()
    model, mask = st["model"], st["mask"]
    pred, loss, grads, caps = st["first"]
    named = dict(model.named_parameters())
    keys = grad_keys(g, "se2_")
    assert set(keys) <= set(named), "state_dict schema differs from the reference"
    fc = [k for k in keys if ".layers2." in k]
    assert len(fc) == 16 and set(fc) <= set(grads), "the SE FC gradients are not among the checked keys"
    e = golden_err(g, "se2_pred", pred)
    print(f"se pgd2: prediction NRMSE vs the reference {e:.3g}; loss {float(loss):.8g} vs {float(g['se2_loss']):.8g}")
    assert e < 1e-5
    assert abs(float(loss) - float(g["se2_loss"])) < 1e-5 * float(g["se2_loss"])
    mc, yc, tc = st["maps"].cpu(), st["y"].cpu(), st["target"].cpu()

    def lf(P, c, mk):
        reg = lambda Pu, xu: se_oracle.seresnet(Pu, xu, relu=mk.relu())       # noqa: E731
        pred_o = O.pgd(O.split_unrolls(P, 2), c(yc), c(mc), c(mask), reg=reg)
        return torch.mean(torch.abs(c(tc) - pred_o))
    assert_masked_f64(grads, lf, model.state_dict(), lambda k: "step_size" not in k, HipMasks(caps), "se pgd2")


def test_se_determinism():
    """The same step twice: bit-identical predictions and SE FC gradients (the gate's two
    reductions use no float atomics, and the gate multiplies every voxel of a block)."""
    st = _golden_step()
    pred1, _, grads1, _ = st["first"]
    pred2, _, grads2, _ = st["step"](False)
    assert torch.equal(pred1, pred2)
    fc = [k for k in grads1 if ".layers2." in k]
    assert len(fc) == 16
    for k in fc:
        assert torch.equal(grads1[k], grads2[k]), k


def test_seresnet_batch_independence():
    """SeResNet alone at B = 2 with the items scaled x1 and x3 (Tp = 20): gates, dm / N and
    the pooled means stay per batch item, and N counts the time pad."""
    from dl_cs.models import engine, se3d, swin3D
    swin3D.set_compute_dtype(torch.float32)
    B, E, T, Y, X = 2, 1, 8, 8, 12
    net = se3d.SeResNet(num_resblocks=2, in_chans=2 * E, chans=32, kernel_size=3, rr=4)
    assert T + 2 * net.pad_size == 20
    recipe.fill_module(net, 111)
    assert se_oracle.scale_fc_weights(net) == 4
    net = net.to(DEV)
    x = recipe.crandn(112, (B, E, T, Y, X)) * torch.tensor([1.0, 3.0]).view(B, 1, 1, 1, 1)
    dy = recipe.crandn(113, (B, E, T, Y, X))
    xg = x.to(DEV).requires_grad_()
    engine.CAPTURE = []
    try:
        out = net(xg)
    finally:
        caps, engine.CAPTURE = engine.CAPTURE, None
    (out * dy.to(DEV).conj()).real.sum().backward()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    stats = []
    ref = se_oracle.seresnet({k: v.double() for k, v in sd.items()}, x.to(torch.complex128), stats=stats)
    gates = torch.cat([s.reshape(-1) for s, _ in stats])
    zs = torch.cat([z.reshape(-1) for _, z in stats])
    rel = float(zs.abs().min() / zs.pow(2).mean().sqrt())
    print(f"batch independence: gates {float(gates.min()):.3g} .. {float(gates.max()):.3g}, "
          f"min |FC1 pre-activation| / rms {rel:.3g}")
    assert float((stats[0][0][0] - stats[0][0][1]).abs().max()) > 0.05, "the two items' gates do not differ"
    assert rel >= 1e-3, "a hidden unit of the gate sits at its ReLU threshold"
    from oracle import dlcs_oracle as O
    e = O.nrmse(ref, out.detach().cpu())
    print(f"batch independence: output NRMSE vs float64 {e:.3g}")
    assert e < 1e-5

    def lf(P, c, mk):
        o = se_oracle.seresnet({k: v for k, v in P.items() if k != "x"}, P["x"], relu=mk.relu())
        return (o * c(dy).conj()).real.sum()
    hip = {n: p.grad for n, p in net.named_parameters()}
    hip["x"] = xg.grad
    assert_masked_f64(hip, lf, dict(sd, x=x), None, HipMasks(caps), "seresnet B=2")


def test_se_hqs_runs_and_matches_oracle():
    """HQS with the SE-ResNet regularizer through the device CG vs the oracle's loop, at the
    ResNet HQS test's shape (no reference golden for this combination)."""
    from oracle import dlcs_oracle as O
    from dl_cs.mri import transforms as T
    from dl_cs.models import swin3D
    swin3D.set_compute_dtype(torch.float32)
    B, E, C, Tt, Y, X = 1, 1, 8, 20, 32, 32
    model = _model(2, 91, hqs=True)
    maps = recipe.sense_maps(92, B, E, C, Y, X)
    mask = recipe.binary_mask(93, (B, 1, Tt, Y, X))
    y = recipe.crandn(94, (B, C, Tt, Y, X)) * mask
    with torch.no_grad():
        pred = model(y=y.to(DEV), A=T.SenseModel(maps.to(DEV), weights=mask.to(DEV)), x0=None).cpu()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    Ps = O.split_unrolls(sd, 2)
    ATy = O.sense_adjoint(y, maps, mask)
    x = ATy
    normal = lambda m: O.sense_adjoint(O.sense_forward(m, maps, mask), maps, mask) + 0.1 * m   # noqa: E731
    for P in Ps:
        x = O.conjugate_gradient(normal, x, ATy + 0.1 * se_oracle.seresnet(P, x), 10)
    e = O.nrmse(x, pred)
    print(f"se hqs: NRMSE vs the oracle loop {e:.3g}")
    assert e < 1e-5


def test_reconstruct_build_model_se(tmp_path):
    """scripts/reconstruct.py::build_model with MODEL_TYPE 'SE': loads a state dict saved from a
    fresh unrolledSE model (strict) and reconstructs one 32 x 32 slice."""
    from dl_cs.models import swin3D, unrolledSE
    from dl_cs.mri import transforms as T
    from oracle import dlcs_oracle as O
    swin3D.set_compute_dtype(torch.float32)
    spec = importlib.util.spec_from_file_location("reconstruct", os.path.join(REPO, "scripts", "reconstruct.py"))
    rc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rc)
    cfg = _cfg(1)
    fresh = unrolledSE.ProximalGradientDescent(cfg)
    recipe.fill_module(fresh, 121)
    se_oracle.scale_fc_weights(fresh)
    ck = tmp_path / "se.ckpt"
    torch.save(fresh.state_dict(), ck)
    model = rc.build_model(cfg)
    assert type(model) is unrolledSE.ProximalGradientDescent
    model.load_state_dict(torch.load(ck, weights_only=True), strict=True)
    model = model.to(DEV).eval()
    B, E, C, Tt, Y, X = 1, 1, 4, 8, 32, 32
    maps = recipe.sense_maps(122, B, E, C, Y, X)
    mask = recipe.binary_mask(123, (B, 1, Tt, Y, X))
    y = recipe.crandn(124, (B, C, Tt, Y, X)) * mask
    with torch.no_grad():
        pred = model(y=y.to(DEV), A=T.SenseModel(maps.to(DEV), weights=mask.to(DEV)), x0=None).cpu()
    assert pred.shape == (B, E, Tt, Y, X) and bool(torch.isfinite(torch.view_as_real(pred)).all())
    ref = O.pgd(O.split_unrolls(fresh.state_dict(), 1), y, maps, mask, reg=se_oracle.seresnet)
    assert O.nrmse(ref.detach(), pred) < 1e-5
