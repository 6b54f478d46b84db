"""HIP unrolled CBAM-ResNet (MODEL_TYPE 'CBAM'; dl_cs/models/unrolledCBAM.py, CBAM.py) vs the
reference's own outputs (tests/golden/cbam.npz) and the CPU restatement
tests/cbam_oracle.py: test_gpu_se.py transposed to the CBAM family.  Outputs
NRMSE <= 1e-5; gradients held to the float64 floor with the HIP forward's ReLU
decisions (goldutil.assert_masked_f64: max(1e-5, 4 x the fp32 oracle's own floor))."""
import importlib.util
import os

import pytest
import torch

import cbam_oracle
from goldutil import HipMasks, assert_masked_f64, golden_err, grad_keys
from oracle import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(n, feats=64, rr=16):
    from dl_cs.config import get_cfg
    cfg = get_cfg()
    cfg.MODEL.MODEL_TYPE = "CBAM"
    P = cfg.MODEL.PARAMETERS
    P.NUM_UNROLLS, P.NUM_RESBLOCKS, P.NUM_FEATURES, P.NUM_EMAPS, P.RR = n, 2, feats, 1, rr
    P.CONV_BLOCK.COMPLEX, P.FIX_STEP_SIZE = False, True
    return cfg


def _model(n, seed, hqs=False):
    from dl_cs.models import unrolledCBAM
    m = (unrolledCBAM.HalfQuadraticSplitting if hqs else unrolledCBAM.ProximalGradientDescent)(_cfg(n))
    m.eval()
    recipe.fill_module(m, seed)
    assert cbam_oracle.spread_gates(m) == 8 * n                  # the fixtures' CA x8, SA x32, SA bias + 1
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


def test_cbam_pgd2_training_step(golden):
    from oracle import dlcs_oracle as O
    g = golden("cbam")
    st = _golden_step()
    model, mask = st["model"], st["mask"]
    pred, loss, grads, caps = st["first"]
    named = dict(model.named_parameters())
    keys = grad_keys(g, "cbam2_")
    assert set(keys) <= set(named), "state_dict schema differs from the reference"
    gate = [k for k in keys if ".CAmodule." in k or ".SAmodule." in k]
    assert len(gate) == 24 and set(gate) <= set(grads), "the gates' gradients are not among the checked keys"
    e = golden_err(g, "cbam2_pred", pred)
    print(f"cbam pgd2: prediction NRMSE vs the reference {e:.3g}; loss {float(loss):.8g} vs {float(g['cbam2_loss']):.8g}")
    assert e < 1e-5
    assert abs(float(loss) - float(g["cbam2_loss"])) < 1e-5 * float(g["cbam2_loss"])
    mc, yc, tc = st["maps"].cpu(), st["y"].cpu(), st["target"].cpu()

    def lf(P, c, mk):
        reg = lambda Pu, xu: cbam_oracle.cbamresnet(Pu, xu, relu=mk.relu())       # noqa: E731
        pred_o = O.pgd(O.split_unrolls(P, 2), c(yc), c(mc), c(mask), reg=reg)
        return torch.mean(torch.abs(c(tc) - pred_o))
    assert_masked_f64(grads, lf, model.state_dict(), lambda k: "step_size" not in k, HipMasks(caps), "cbam pgd2")


def test_cbam_determinism():
    """The same step twice: bit-identical predictions and gradients of every parameter of the two
    gates, the 125-tap weight and its bias included (their reductions use no float atomics).  The conv
    trunk's weight gradients come from the conv wgrad kernels, which accumulate with fp32 atomics, as in
    test_se_determinism."""
    st = _golden_step()
    pred1, _, grads1, _ = st["first"]
    pred2, _, grads2, _ = st["step"](False)
    assert torch.equal(pred1, pred2)
    gate = [k for k in grads1 if ".CAmodule." in k or ".SAmodule." in k]
    assert len(gate) == 24
    for k in gate:
        assert torch.equal(grads1[k], grads2[k]), k


def test_cbamresnet_batch_independence():
    """CBAMResNet alone at B = 2 with the items scaled x1 and x3 (Tp = 20): gates, maps, dm / N and
    the pooled means stay per batch item, the stencil does not cross items, and N counts the time pad.

    The SA bias is one number, the sum over all voxels of dL/dq, and the bar below is relative to it.
    Each dL/dq element carries at least one fp32 rounding (u = 2^-24 = 6e-8 relative), so any fp32
    evaluation of that sum is off by about K u of its value, K = sum |dL/dq| / |sum dL/dq|: the 1e-5
    bar can be met only for K < 1e-5 / u = 168.  The float64 oracle gives K = 45 and 28 for the two
    blocks with the data below (fill 211, x 212, dy 213) and 575 for block 0 with the SE test's seeds
    111-113, where the bar would measure that cancellation, not the kernels; K < 100 is asserted."""
    from dl_cs.models import CBAM, engine, swin3D
    swin3D.set_compute_dtype(torch.float32)
    B, E, T, Y, X = 2, 1, 8, 8, 12
    net = CBAM.CBAMResNet(num_resblocks=2, in_chans=2 * E, chans=32, kernel_size=3, rr=4)
    assert T + 2 * net.pad_size == 20
    recipe.fill_module(net, 211)
    assert cbam_oracle.spread_gates(net) == 8
    net = net.to(DEV)
    x = recipe.crandn(212, (B, E, T, Y, X)) * torch.tensor([1.0, 3.0]).view(B, 1, 1, 1, 1)
    dy = recipe.crandn(213, (B, E, T, Y, X))
    xg = x.to(DEV).requires_grad_()
    engine.CAPTURE = []
    try:
        out = net(xg)
    finally:
        caps, engine.CAPTURE = engine.CAPTURE, None
    (out * dy.to(DEV).conj()).real.sum().backward()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    stats = []
    qmaps = []
    ref = cbam_oracle.cbamresnet({k: v.double().requires_grad_() for k, v in sd.items()}, x.to(torch.complex128),
                                 stats=stats, maps=qmaps)
    (ref * dy.to(torch.complex128).conj()).real.sum().backward()
    cond = [float(q.grad.abs().sum() / q.grad.sum().abs()) for q in qmaps]
    print("batch independence: sum |dL/dq| / |sum dL/dq| per block " + ", ".join(f"{k:.3g}" for k in cond))
    assert max(cond) < 100, "the SA-bias gradient of this data cancels too far for an fp32 bar of 1e-5"
    ref = ref.detach()
    gates = torch.cat([s.reshape(-1) for s, _, _ in stats])
    zs = torch.cat([z.reshape(-1) for _, z, _ in stats])
    qs = torch.cat([q.reshape(-1) for _, _, q in stats])
    rel = float(zs.abs().min() / zs.pow(2).mean().sqrt())
    print(f"batch independence: gates {float(gates.min()):.3g} .. {float(gates.max()):.3g}, "
          f"maps {float(qs.min()):.3g} .. {float(qs.max()):.3g}, min |FC1 pre-activation| / rms {rel:.3g}")
    assert float((stats[0][0][0] - stats[0][0][1]).abs().max()) > 0.05, "the two items' gates do not differ"
    assert rel >= 1e-3, "a hidden unit of the gate sits at its ReLU threshold"
    from oracle import dlcs_oracle as O
    e = O.nrmse(ref, out.detach().cpu())
    print(f"batch independence: output NRMSE vs float64 {e:.3g}")
    assert e < 1e-5

    def lf(P, c, mk):
        o = cbam_oracle.cbamresnet({k: v for k, v in P.items() if k != "x"}, P["x"], relu=mk.relu())
        return (o * c(dy).conj()).real.sum()
    hip = {n: p.grad for n, p in net.named_parameters()}
    hip["x"] = xg.grad
    assert_masked_f64(hip, lf, dict(sd, x=x), None, HipMasks(caps), "cbamresnet B=2")


def test_cbam_hqs_runs_and_matches_oracle():
    """HQS with the CBAM-ResNet regularizer through the device CG vs the oracle's loop, at the
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
        x = O.conjugate_gradient(normal, x, ATy + 0.1 * cbam_oracle.cbamresnet(P, x), 10)
    e = O.nrmse(x, pred)
    print(f"cbam hqs: NRMSE vs the oracle loop {e:.3g}")
    assert e < 1e-5


# _cfg(1) as a file, for the command line
CFG = """
MODEL:
  MODEL_TYPE: "CBAM"
  META_ARCHITECTURE: "dlespirit"
  PARAMETERS:
    NUM_UNROLLS: 1
    NUM_RESBLOCKS: 2
    NUM_FEATURES: 64
    RR: 16
    NUM_EMAPS: 1
    FIX_STEP_SIZE: True
    SLWIN_INIT: True
    CONV_BLOCK:
      COMPLEX: False
AUG_TRAIN:
  CROP_READOUT: 16
OUTPUT_DIR: "{out}"
"""


def test_reconstruct_cbam_builds_and_runs(tmp_path):
    """scripts/reconstruct_cbam.py: its build_model loads a state dict saved from a fresh
    unrolledCBAM model (strict), and its main reconstructs one 32 x 32 slice from CFL files."""
    import numpy as np
    from dl_cs.fileio import cfl
    from dl_cs.models import swin3D, unrolledCBAM
    from dl_cs.mri import transforms as T
    from oracle import dlcs_oracle as O
    swin3D.set_compute_dtype(torch.float32)
    spec = importlib.util.spec_from_file_location("reconstruct_cbam", os.path.join(REPO, "scripts", "reconstruct_cbam.py"))
    rc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rc)
    cfg = _cfg(1)
    fresh = unrolledCBAM.ProximalGradientDescent(cfg)
    recipe.fill_module(fresh, 121)
    cbam_oracle.spread_gates(fresh)
    ck = tmp_path / "cbam.ckpt"
    torch.save(fresh.state_dict(), ck)
    model = rc.build_model(cfg)
    assert type(model) is unrolledCBAM.ProximalGradientDescent
    model.load_state_dict(torch.load(ck, weights_only=True), strict=True)
    model = model.to(DEV).eval()
    B, E, C, Tt, Y, X = 1, 1, 4, 8, 32, 32
    maps = recipe.sense_maps(122, B, E, C, Y, X)
    mask = recipe.binary_mask(123, (B, 1, Tt, Y, X))
    y = recipe.crandn(124, (B, C, Tt, Y, X)) * mask
    with torch.no_grad():
        pred = model(y=y.to(DEV), A=T.SenseModel(maps.to(DEV), weights=mask.to(DEV)), x0=None).cpu()
    assert pred.shape == (B, E, Tt, Y, X) and bool(torch.isfinite(torch.view_as_real(pred)).all())
    ref = O.pgd(O.split_unrolls(fresh.state_dict(), 1), y, maps, mask, reg=cbam_oracle.cbamresnet)
    assert O.nrmse(ref.detach(), pred) < 1e-5
    # the command line: CFL k-space [x, y, sl, coil, 1, echo, 1, phase] and maps [x, y, sl, coil, emap] in, images out
    from dl_cs.data.dataset import SyntheticCineDataset
    ds = SyntheticCineDataset(1, lambda k, m, t, f: (k, m), coils=C, emaps=E, frames=Tt, ny=Y, nx=X, seed=5)
    ks = np.stack([ds[0][0]])                                    # [sl, C, T, Y, X]
    mp = np.stack([ds[0][1]])                                    # [sl, E, C, 1, Y, X]
    ks[:, :, :, ::3] = 0                                         # undersample ky
    cfl.write(str(tmp_path / "ks"), ks.transpose(4, 3, 0, 1, 2).reshape(X, Y, 1, C, 1, 1, 1, Tt), order='F')
    cfl.write(str(tmp_path / "maps"), mp[:, :, :, 0].transpose(4, 3, 0, 2, 1), order='F')
    cfg_file = tmp_path / "cbam.yaml"
    cfg_file.write_text(CFG.format(out=str(tmp_path / "out")))
    args = rc.create_arg_parser().parse_args(["--directory", str(tmp_path), "--ckpt", str(ck),
                                              "--config-file", str(cfg_file), "--device", "0"])
    rc.main(args)
    im = cfl.read(str(tmp_path / "im.dl"), order='F')
    assert im.shape == (X, Y, 1, 1, E, 1, 1, Tt)
    assert np.isfinite(im).all() and np.abs(im).max() > 0
