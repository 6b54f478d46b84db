"""The ResNet, SE and CBAM regularisers on grids that are no multiples of 4 (the padded path
of dl_cs/models/resnet3d.py: box_pre / box_post, box_zero on the slack rows, means over the
box's voxels) vs the reference's own outputs (tests/golden/anygrid.npz) and the CPU oracles
oracle.dlcs_oracle.resnet, tests/se_oracle.seresnet and tests/cbam_oracle.cbamresnet.

Tolerances are those of test_gpu_resnet.py / test_gpu_se.py / test_gpu_cbam.py: outputs
NRMSE < 1e-5, loss 1e-5 relative, gradients held to the float64 floor with the HIP forward's
ReLU decisions (goldutil.assert_masked_f64: max(1e-5, 4 x the fp32 oracle's own floor)).  The
decisions are captured in the padded grid's rows and cropped to the box here
(goldutil.captured_masks assumes a grid without slack)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import cbam_oracle
import se_oracle
from goldutil import HipMasks, assert_masked_f64, captured_masks, golden_err
from oracle import dlcs_oracle as O
from oracle import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRIDS = [(7, 10, 13), (9, 11, 14), (10, 13, 9)]       # T + 12 = 19, 21, 22: every axis sees 1, 2, 3 mod 4
FAMILIES = ["res", "se", "cbam"]
FILL = {"res": 81, "se": 181, "cbam": 281}            # the fixture's fill seeds (make_golden_anygrid.py)
MODEL_TYPE = {"res": "RES", "se": "SE", "cbam": "CBAM"}
_fam = pytest.mark.parametrize("fam", FAMILIES)


def _oracle(fam):
    return {"res": O.resnet, "se": se_oracle.seresnet, "cbam": cbam_oracle.cbamresnet}[fam]


def _spread(fam, m):
    """The fixtures' spreading of the gates (nothing for the plain ResNet)."""
    if fam == "se":
        return se_oracle.scale_fc_weights(m)
    if fam == "cbam":
        return cbam_oracle.spread_gates(m)
    return 0


def _cfg(fam, n):
    from dl_cs.config import get_cfg
    cfg = get_cfg()
    cfg.MODEL.MODEL_TYPE = MODEL_TYPE[fam]
    P = cfg.MODEL.PARAMETERS
    P.NUM_UNROLLS, P.NUM_RESBLOCKS, P.NUM_FEATURES, P.NUM_EMAPS, P.RR = n, 2, 64, 1, 16
    P.CONV_BLOCK.COMPLEX, P.FIX_STEP_SIZE = False, True
    return cfg


def _unrolled(fam):
    from dl_cs.models import unrolled, unrolledCBAM, unrolledSE
    return {"res": unrolled, "se": unrolledSE, "cbam": unrolledCBAM}[fam]


def _model(fam, n, seed, hqs=False):
    mod = _unrolled(fam)
    m = (mod.HalfQuadraticSplitting if hqs else mod.ProximalGradientDescent)(_cfg(fam, n))
    m.eval()
    recipe.fill_module(m, seed)
    assert _spread(fam, m) == {"res": 0, "se": 4 * n, "cbam": 8 * n}[fam]
    return m.to(DEV)


def _net(fam, blocks, feats, rr, seed):
    """The regulariser alone."""
    from dl_cs.models import CBAM, resnet3d, se3d
    if fam == "res":
        net = resnet3d.ResNet(num_resblocks=blocks, in_chans=2, chans=feats, kernel_size=3)
    else:
        cls = se3d.SeResNet if fam == "se" else CBAM.CBAMResNet
        net = cls(num_resblocks=blocks, in_chans=2, chans=feats, kernel_size=3, rr=rr)
    recipe.fill_module(net, seed)
    _spread(fam, net)
    return net.to(DEV)


def _crop(cap):
    """captured_masks of a CAPTURE entry of the padded path, cropped to its box."""
    B, D, H, W = cap["box"]
    assert cap["grid"] == (B,) + tuple((n + 3) // 4 * 4 for n in (D, H, W)) and cap["grid"] != cap["box"]
    for t in cap["relu_inputs"]:                       # the invariant: post-ReLU tensors are zero outside the box
        m = captured_masks(dict(cap, relu_inputs=[t]))[0]
        m[:, :, :D, :H, :W] = False
        assert not bool(m.any()), "a stored activation is non-zero on a slack row"
    return [m[:, :, :D, :H, :W].contiguous() for m in captured_masks(cap)]


class BoxMasks(HipMasks):
    def __init__(self, caps):
        super().__init__([])
        self.calls = [_crop(c) for c in caps]


def _capture(fn):
    from dl_cs.models import engine
    engine.CAPTURE = []
    try:
        out = fn()
    finally:
        caps, engine.CAPTURE = engine.CAPTURE, None
    return out, caps


def _fp32():
    from dl_cs.models import swin3D
    swin3D.set_compute_dtype(torch.float32)


_STEPS = {}


def _step(fam, grid):
    """One 2-unroll training step at the fixture's sizes and seeds: computed once per
    (family, grid), shared by the golden and the repeatability tests, left unchanged."""
    key = (fam, grid)
    if key in _STEPS:
        return _STEPS[key]
    from dl_cs.mri import transforms as T
    _fp32()
    B, E, C = 1, 1, 4
    Tt, Y, X = grid
    model = _model(fam, 2, FILL[fam])
    maps = recipe.sense_maps(82, B, E, C, Y, X).to(DEV)
    mask = recipe.binary_mask(83, (B, 1, Tt, Y, X))
    y = (recipe.crandn(84, (B, C, Tt, Y, X)) * mask).to(DEV)
    target = recipe.crandn(85, (B, E, Tt, Y, X)).to(DEV)

    def step():
        model.zero_grad(set_to_none=True)
        pred, caps = _capture(lambda: model(y=y, A=T.SenseModel(maps, weights=mask.to(DEV)), x0=None))
        loss = torch.mean(torch.abs(target - pred))
        loss.backward()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        return pred.detach().clone(), loss.detach().clone(), grads, caps

    _STEPS[key] = dict(model=model, maps=maps, mask=mask, y=y, target=target, first=step(), step=step)
    return _STEPS[key]


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
@_fam
def test_anygrid_pgd2_training_step(golden, fam, grid):
    g = golden("anygrid")
    tag = f"{fam}_{grid[0]}x{grid[1]}x{grid[2]}_"
    st = _step(fam, grid)
    model, mask = st["model"], st["mask"]
    pred, loss, grads, caps = st["first"]
    keys = sorted(k[len(tag + "norm::"):] for k in g if k.startswith(tag + "norm::"))
    assert keys and set(keys) <= set(grads), "state_dict schema differs from the reference"
    e = golden_err(g, tag + "pred", pred)
    print(f"{tag}: prediction NRMSE vs the reference {e:.3g}; loss {float(loss):.8g} vs {float(g[tag + 'loss']):.8g}")
    assert e < 1e-5
    assert abs(float(loss) - float(g[tag + "loss"])) < 1e-5 * float(g[tag + "loss"])
    assert len(caps) == 2 and all(c["box"] == (1, grid[0] + 12, grid[1], grid[2]) for c in caps)
    mc, yc, tc = st["maps"].cpu(), st["y"].cpu(), st["target"].cpu()
    oracle = _oracle(fam)

    def lf(P, c, mk):
        reg = lambda Pu, xu: oracle(Pu, xu, relu=mk.relu())                   # noqa: E731
        pred_o = O.pgd(O.split_unrolls(P, 2), c(yc), c(mc), c(mask), reg=reg)
        return torch.mean(torch.abs(c(tc) - pred_o))
    assert_masked_f64(grads, lf, model.state_dict(), lambda k: "step_size" not in k, BoxMasks(caps), tag)


@_fam
def test_anygrid_hqs_matches_oracle(fam):
    """HQS through the device CG vs the oracle's conjugate_gradient restatement on (9, 11, 14),
    as test_resnet_hqs_runs_and_matches_oracle."""
    from dl_cs.mri import transforms as T
    _fp32()
    B, E, C, Tt, Y, X = 1, 1, 4, 9, 11, 14
    model = _model(fam, 2, 91, hqs=True)
    maps = recipe.sense_maps(92, B, E, C, Y, X)
    mask = recipe.binary_mask(93, (B, 1, Tt, Y, X))
    y = recipe.crandn(94, (B, C, Tt, Y, X)) * mask
    with torch.no_grad():
        pred = model(y=y.to(DEV), A=T.SenseModel(maps.to(DEV), weights=mask.to(DEV)), x0=None).cpu()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ATy = O.sense_adjoint(y, maps, mask)
    x = ATy
    normal = lambda m: O.sense_adjoint(O.sense_forward(m, maps, mask), maps, mask) + 0.1 * m   # noqa: E731
    for P in O.split_unrolls(sd, 2):
        x = O.conjugate_gradient(normal, x, ATy + 0.1 * _oracle(fam)(P, x), 10)
    e = O.nrmse(x, pred)
    print(f"{fam} hqs 9x11x14: NRMSE vs the oracle loop {e:.3g}")
    assert e < 1e-5


@_fam
def test_anygrid_batch_of_two(fam):
    """The regulariser alone on (7, 10, 13) at B = 2 with two different items: each item's output
    and input gradient carry the bits of its single-item run (the per-item row ranges of the
    padded grid: box_pre / box_post, box_zero's slabs, the gates' per-item means over the box)."""
    _fp32()
    E, T, Y, X = 1, 7, 10, 13
    net = _net(fam, 2, 64, 16, 131)
    x = recipe.crandn(132, (2, E, T, Y, X)) * torch.tensor([1.0, 3.0]).view(2, 1, 1, 1, 1)
    dy = recipe.crandn(133, (2, E, T, Y, X))

    def run(xi, dyi):
        xg = xi.to(DEV).requires_grad_()
        out = net(xg)
        (out * dyi.to(DEV).conj()).real.sum().backward()
        return out.detach().cpu(), xg.grad.cpu()
    both, gboth = run(x, dy)
    assert not torch.equal(both[0], both[1])
    for b in range(2):
        one, gone = run(x[b:b + 1], dy[b:b + 1])
        assert torch.equal(torch.view_as_real(both[b:b + 1]), torch.view_as_real(one)), f"item {b}: output"
        assert torch.equal(torch.view_as_real(gboth[b:b + 1]), torch.view_as_real(gone)), f"item {b}: input gradient"


@_fam
def test_anygrid_axes_shorter_than_a_patch(fam):
    """(T, Y, X) = (6, 3, 5) with 1 block (pad 4), 8 features, RR 4: the box 14 x 3 x 5 in
    16 x 4 x 8, Y inside one patch.  The regulariser alone vs its oracle: forward output, and
    the input gradient with the HIP forward's ReLU decisions (float64)."""
    _fp32()
    B, E, T, Y, X = 1, 1, 6, 3, 5
    net = _net(fam, 1, 8, 4, 141)
    assert net.pad_size == 4
    x = recipe.crandn(142, (B, E, T, Y, X))
    dy = recipe.crandn(143, (B, E, T, Y, X))
    xg = x.to(DEV).requires_grad_()
    out, caps = _capture(lambda: net(xg))
    (out * dy.to(DEV).conj()).real.sum().backward()
    assert caps[0]["grid"] == (1, 16, 4, 8) and caps[0]["box"] == (1, 14, 3, 5)
    P = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    kw = {}
    if fam != "res":
        kw["stats"] = stats = []
    ref = _oracle(fam)(P, x.to(torch.complex128), num_resblocks=1, **kw)
    if fam != "res":
        z = torch.cat([s[1].reshape(-1) for s in stats])
        rel = float(z.abs().min() / z.pow(2).mean().sqrt())
        assert rel >= 1e-3, "a hidden unit of the gate sits at its ReLU threshold"
    e = O.nrmse(ref, out.detach().cpu())
    x64 = x.to(torch.complex128).requires_grad_()
    o64 = _oracle(fam)(P, x64, num_resblocks=1, relu=BoxMasks(caps).relu())
    (o64 * dy.to(torch.complex128).conj()).real.sum().backward()
    eg = O.nrmse(x64.grad, xg.grad.cpu())
    print(f"{fam} 6x3x5: output NRMSE {e:.3g}, input gradient NRMSE {eg:.3g}")
    assert e < 1e-5
    assert eg < 1e-5


@pytest.mark.parametrize("fam", ["se", "cbam"])
def test_anygrid_repeatability(fam):
    """Two identical training steps on (10, 13, 9): bit-identical predictions and gate-parameter
    gradients, as test_se_determinism / test_cbam_determinism on a grid without slack (the gate's
    reductions use no float atomics; the conv weight and bias gradients accumulate with float
    atomics on either path and are held to the oracle by the training-step test)."""
    st = _step(fam, (10, 13, 9))
    pred1, _, grads1, _ = st["first"]
    pred2, _, grads2, _ = st["step"]()
    assert torch.equal(pred1, pred2)
    gate = [k for k in grads1 if any(s in k for s in (".layers2.", ".CAmodule.", ".SAmodule."))]
    assert len(gate) == {"se": 16, "cbam": 24}[fam]
    for k in gate:
        assert torch.equal(grads1[k], grads2[k]), k


@_fam
def test_unpadded_path_launches_no_box_kernel(fam, monkeypatch):
    """A grid of multiples of 4 (20 x 32 x 32) runs forward and backward with every box wrapper
    of _ops replaced by one that raises: the launches of the unpadded path are unchanged."""
    from dl_cs.models import _ops as K
    _fp32()

    def refuse(*a, **k):
        raise AssertionError("a box kernel was called on a grid without slack")
    for name in ("box_zero", "box_pre", "box_pre_bwd", "box_post", "box_post_bwd"):
        monkeypatch.setattr(K, name, refuse)
    net = _net(fam, 2, 32, 4, 151)
    xg = recipe.crandn(152, (1, 1, 8, 32, 32)).to(DEV).requires_grad_()
    out, caps = _capture(lambda: net(xg))
    out.abs().sum().backward()
    assert caps[0]["grid"] == (1, 20, 32, 32) and "box" not in caps[0]
    assert bool(torch.isfinite(torch.view_as_real(xg.grad)).all())


# ---------------------------------------------------------------------------- end to end
CFG = """
MODEL:
  MODEL_TYPE: "{model_type}"
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


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@_fam
def test_reconstruct_scan_of_odd_size(fam, tmp_path):
    """scripts/reconstruct.py (RES, SE) and scripts/reconstruct_cbam.py (CBAM) on a 2-slice CFL
    scan of 9 phases, 11 x 14, 4 coils, with a freshly filled 1-unroll checkpoint: the output CFL
    has the scan's shape, is finite and matches the oracle's PGD on the same preprocessed inputs."""
    from dl_cs.config import load_cfg
    from dl_cs.data.dataset import SyntheticCineDataset
    from dl_cs.data.preprocess import DataTransform
    from dl_cs.fileio import cfl
    _fp32()
    S, E, C, Tt, Y, X = 2, 1, 4, 9, 11, 14
    rc = _script("reconstruct_cbam" if fam == "cbam" else "reconstruct")
    cfg_file = tmp_path / "c.yaml"
    cfg_file.write_text(CFG.format(model_type=MODEL_TYPE[fam], out=str(tmp_path / "out")))
    config = load_cfg(str(cfg_file))
    fresh = rc.build_model(config)
    recipe.fill_module(fresh, 161)
    _spread(fam, fresh)
    ck = tmp_path / "m.ckpt"
    torch.save(fresh.state_dict(), ck)
    ds = SyntheticCineDataset(S, lambda k, m, t, f: (k, m), coils=C, emaps=E, frames=Tt, ny=Y, nx=X, seed=5)
    ks = np.stack([ds[i][0] for i in range(S)]).astype(np.complex64)         # [sl, C, T, Y, X]
    mp = np.stack([ds[i][1] for i in range(S)]).astype(np.complex64)         # [sl, E, C, 1, Y, X]
    ks[:, :, :, ::3] = 0                                                     # undersample ky
    cfl.write(str(tmp_path / "ks"), ks.transpose(4, 3, 0, 1, 2).reshape(X, Y, S, C, 1, 1, 1, Tt), order='F')
    cfl.write(str(tmp_path / "maps"), mp[:, :, :, 0].transpose(4, 3, 0, 2, 1), order='F')
    args = rc.create_arg_parser().parse_args(["--directory", str(tmp_path), "--ckpt", str(ck),
                                              "--config-file", str(cfg_file), "--device", "0"])
    rc.main(args)
    im = cfl.read(str(tmp_path / "im.dl"), order='F')
    assert im.shape == (X, Y, S, 1, E, 1, 1, Tt)
    assert np.isfinite(im).all() and np.abs(im).max() > 0
    got = np.transpose(im[:, :, :, 0, :, 0, 0, :], (2, 3, 4, 1, 0))          # [sl, E, T, Y, X]
    tf = DataTransform(config, device="cuda")
    sd = {k: v.detach().cpu() for k, v in fresh.state_dict().items()}
    data = _script("reconstruct").CflDataset(str(tmp_path / "ks"), str(tmp_path / "maps"))
    for sl in range(S):
        k_, mp_, mask_, init_, scale_ = (t.cpu() for t in tf(*data[sl]))
        ref = O.pgd(O.split_unrolls(sd, 1), k_[None], mp_[None], mask_[None], x0=init_[None], reg=_oracle(fam))
        e = O.nrmse(scale_ * ref[0], torch.from_numpy(np.ascontiguousarray(got[sl])))
        print(f"{fam} reconstruct 9x11x14 slice {sl}: NRMSE vs the oracle's PGD {e:.3g}")
        assert e < 1e-5
