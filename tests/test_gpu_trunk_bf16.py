"""The ResNet, SE and CBAM regularisers with compute dtype bf16 (swin3D.set_compute_dtype):
activations stored in bf16, weights / gradients / the complex boundary in fp32.

  1 prediction vs the reference's own fixtures at the bf16 budget NRMSE < 1e-2
  2 gradients vs an autocast oracle (the rule of test_bf16_swinnet_two_swinblocks, factor 1.5)
  3 slack rows of the padded path stay zero        4 batch of two = single items, bitwise
  5 repeatability of the gated families            6 HQS eval within 1e-2 of the oracle loop
  7 the training and reconstruction entry points with --dtype bf16
  8 the fp32 path calls none of the bf16 wrappers

Models, oracles, fixtures' gate spreading and the CFL scan are those of test_gpu_anygrid.py."""
import json
import math

import numpy as np
import pytest
import torch

import test_gpu_anygrid as A
from goldutil import golden_err
from oracle import dlcs_oracle as O
from oracle import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
_fam = pytest.mark.parametrize("fam", A.FAMILIES)


@pytest.fixture(autouse=True)
def _fp32_after():
    yield
    from dl_cs.models import swin3D
    swin3D.set_compute_dtype(torch.float32)


def _bf16():
    from dl_cs.models import swin3D
    swin3D.set_compute_dtype(BF16)


_STEPS = {}


def _step(fam, grid, coils, fill):
    """One 2-unroll PGD training step in bf16 at the fixtures' seeds (data 82-85): computed once
    per (family, grid), shared by the tests below, left unchanged."""
    key = (fam, grid)
    if key in _STEPS:
        return _STEPS[key]
    from dl_cs.mri import transforms as T
    _bf16()
    B, E = 1, 1
    Tt, Y, X = grid
    model = A._model(fam, 2, fill)
    maps = recipe.sense_maps(82, B, E, coils, Y, X).to(DEV)
    mask = recipe.binary_mask(83, (B, 1, Tt, Y, X))
    y = (recipe.crandn(84, (B, coils, Tt, Y, X)) * mask).to(DEV)
    target = recipe.crandn(85, (B, E, Tt, Y, X)).to(DEV)

    def step():
        _bf16()
        model.zero_grad(set_to_none=True)
        pred, caps = A._capture(lambda: model(y=y, A=T.SenseModel(maps, weights=mask.to(DEV)), x0=None))
        torch.mean(torch.abs(target - pred)).backward()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        return pred.detach().clone(), grads, caps

    _STEPS[key] = dict(first=step(), step=step)
    return _STEPS[key]


# ---------------------------------------------------------------------------- 1
@_fam
def test_bf16_prediction_vs_reference_20x32x32(golden, fam):
    """The 2-unroll PGD step of test_gpu_resnet.py / test_gpu_se.py / test_gpu_cbam.py (fill 81, 8 coils)."""
    name, tag = {"res": ("resnet", "res2_"), "se": ("se", "se2_"), "cbam": ("cbam", "cbam2_")}[fam]
    pred, grads, caps = _step(fam, (20, 32, 32), 8, 81)["first"]
    e = golden_err(golden(name), tag + "pred", pred)
    print(f"{fam} bf16 pgd2 20x32x32: prediction NRMSE vs the reference {e:.3g}")
    assert e < 1e-2
    assert all(c["relu_inputs"][0].dtype == BF16 and "box" not in c for c in caps)
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())


@pytest.mark.parametrize("grid", [(7, 10, 13), (10, 13, 9)], ids=lambda g: "x".join(map(str, g)))
@_fam
def test_bf16_prediction_vs_reference_odd_grids(golden, fam, grid):
    pred, grads, caps = _step(fam, grid, 4, A.FILL[fam])["first"]
    e = golden_err(golden("anygrid"), f"{fam}_{grid[0]}x{grid[1]}x{grid[2]}_pred", pred)
    print(f"{fam} bf16 pgd2 {grid}: prediction NRMSE vs the reference {e:.3g}")
    assert e < 1e-2
    assert len(caps) == 2 and all(c["box"] == (1, grid[0] + 12, grid[1], grid[2]) for c in caps)
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())


# ---------------------------------------------------------------------------- 2
def _rel(a, b):
    return float((a - b).abs().pow(2).sum().sqrt() / b.abs().pow(2).sum().sqrt())


@pytest.mark.parametrize("shape", [(1, 1, 8, 16, 16), (1, 1, 7, 10, 13)], ids=lambda s: "x".join(map(str, s[2:])))
@_fam
def test_bf16_gradients_vs_autocast_oracle(fam, shape):
    """The regulariser alone.  The CPU oracle under torch.autocast(bfloat16) on the same weights,
    input and cotangent gives the error that a bf16-operand evaluation of this network carries
    against the fp32 oracle; the HIP bf16 path stays within 1.5 x of it per class: the
    correction net(x) - x, dx, and the median and the max over the parameter tensors."""
    net = A._net(fam, 2, 64, 16, 171)
    x = recipe.crandn(172, shape).to(torch.complex64)
    gr = recipe.crandn(173, shape).to(torch.complex64)
    _bf16()
    xx = x.to(DEV).requires_grad_()
    y = net(xx)
    (y.real * gr.real.to(DEV) + y.imag * gr.imag.to(DEV)).sum().backward()
    hip = (y.detach().cpu(), xx.grad.cpu(), {k: p.grad.cpu() for k, p in net.named_parameters()})
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}

    def oracle(amp):
        P = {k: v.clone().requires_grad_(torch.is_floating_point(v)) for k, v in sd.items()}
        xo = x.clone().requires_grad_()
        if amp:
            with torch.autocast("cpu", dtype=BF16):
                yo = A._oracle(fam)(P, xo)
        else:
            yo = A._oracle(fam)(P, xo)
        yo = yo.to(torch.complex64)
        (yo.real * gr.real + yo.imag * gr.imag).sum().backward()
        return yo.detach(), xo.grad, {k: v.grad for k, v in P.items() if v.grad is not None}

    ref = oracle(False)

    def classes(y_, dx_, gp):
        y32, dx32, g32 = ref
        pr = sorted(_rel(gp[k], g32[k]) for k in g32 if g32[k].abs().sum() > 0)
        return _rel(y_ - x, y32 - x), _rel(dx_, dx32), pr[len(pr) // 2], pr[-1], _rel(y_, y32)

    h, a = classes(*hip), classes(*oracle(True))
    for name, hv, av in zip(("correction", "dx", "median param", "max param"), h, a):
        print(f"{fam} {shape[2:]} {name}: HIP bf16 {hv:.3g}  autocast oracle {av:.3g}")
    print(f"{fam} {shape[2:]} rel(y): HIP bf16 {h[4]:.3g}  autocast oracle {a[4]:.3g}")
    assert h[4] < 1e-2
    for hv, av in zip(h[:4], a[:4]):
        assert hv <= 1.5 * av, (h, a)


# ---------------------------------------------------------------------------- 3
@_fam
def test_bf16_slack_rows_stay_zero(fam):
    """Every captured post-ReLU tensor of the padded path is zero outside the box (A._crop asserts it)."""
    _, _, caps = _step(fam, (7, 10, 13), 4, A.FILL[fam])["first"]
    for c in caps:
        assert all(t.dtype == BF16 for t in c["relu_inputs"])
        assert len(A._crop(c)) == 5


# ---------------------------------------------------------------------------- 4
@_fam
def test_bf16_batch_of_two(fam):
    _bf16()
    E, T, Y, X = 1, 7, 10, 13
    net = A._net(fam, 2, 64, 16, 131)
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


# ---------------------------------------------------------------------------- 5
@pytest.mark.parametrize("fam", ["se", "cbam"])
def test_bf16_repeatability(fam):
    """Two identical steps on (10, 13, 9): the same bits in the predictions and the gate-parameter
    gradients (the conv weight gradients flush with float atomics and are left out, as in fp32)."""
    st = _step(fam, (10, 13, 9), 4, A.FILL[fam])
    pred1, grads1, _ = st["first"]
    pred2, grads2, _ = st["step"]()
    assert torch.equal(torch.view_as_real(pred1), torch.view_as_real(pred2))
    gate = [k for k in grads1 if any(s in k for s in (".layers2.", ".CAmodule.", ".SAmodule."))]
    assert len(gate) == {"se": 16, "cbam": 24}[fam]
    for k in gate:
        assert torch.equal(grads1[k], grads2[k]), k


# ---------------------------------------------------------------------------- 6
@_fam
def test_bf16_hqs_matches_oracle(fam):
    from dl_cs.mri import transforms as T
    B, E, C, Tt, Y, X = 1, 1, 4, 9, 11, 14
    model = A._model(fam, 2, 91, hqs=True)
    maps = recipe.sense_maps(92, B, E, C, Y, X)
    mask = recipe.binary_mask(93, (B, 1, Tt, Y, X))
    y = recipe.crandn(94, (B, C, Tt, Y, X)) * mask
    _bf16()
    with torch.no_grad():
        pred = model(y=y.to(DEV), A=T.SenseModel(maps.to(DEV), weights=mask.to(DEV)), x0=None).cpu()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ATy = O.sense_adjoint(y, maps, mask)
    x = ATy
    normal = lambda m: O.sense_adjoint(O.sense_forward(m, maps, mask), maps, mask) + 0.1 * m   # noqa: E731
    for P in O.split_unrolls(sd, 2):
        x = O.conjugate_gradient(normal, x, ATy + 0.1 * A._oracle(fam)(P, x), 10)
    e = O.nrmse(x, pred)
    print(f"{fam} bf16 hqs 9x11x14: NRMSE vs the oracle loop {e:.3g}")
    assert e < 1e-2


# ---------------------------------------------------------------------------- 7
TRAIN_CFG = """MODEL:
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
  RECON_LOSS:
    NAME: "complex_l1"
    RENORMALIZE_DATA: False
AUG_TRAIN:
  CROP_READOUT: 16
  UNDERSAMPLE:
    ACCELERATIONS: (4, 6)
    PARTIAL_KX: 0.25
    PARTIAL_KY: 0.25
OPTIMIZER:
  MAX_EPOCHS: 1
EVAL:
  RUN_EVERY_N_EPOCHS: 1
LOGGER:
  LOG_METRICS_EVERY_N_STEPS: 1
SEED: 1000
OUTPUT_DIR: "{out}"
"""


@_fam
def test_bf16_training_script(fam, tmp_path):
    """train_swin.py (RES), train_se.py, train_cbam.py with --dtype bf16: one unroll, two steps."""
    out = tmp_path / "out"
    cfg = tmp_path / "c.yaml"
    cfg.write_text(TRAIN_CFG.format(model_type=A.MODEL_TYPE[fam], out=str(out)))
    tr = A._script({"res": "train_swin", "se": "train_se", "cbam": "train_cbam"}[fam])
    tr.main(["--config-file", str(cfg), "--data", "synthetic", "--synthetic-slices", "2",
             "--synthetic-shape", "4", "1", "8", "16", "24", "--dtype", "bf16"])
    from dl_cs.models import swin3D
    assert swin3D.get_compute_dtype() == BF16
    recs = [json.loads(line) for line in (out / "exp" / "metrics.jsonl").read_text().splitlines()]
    train = [r for r in recs if "Train/complex_l1" in r]
    assert len(train) == 2 and all(math.isfinite(r["Train/complex_l1"]) for r in train)
    ck = torch.load(out / "last.ckpt", weights_only=True)
    assert ck["global_step"] == 2


@_fam
def test_bf16_reconstruct_scan_of_odd_size(fam, tmp_path):
    """reconstruct.py / reconstruct_cbam.py with --dtype bf16 on the 9 x 11 x 14 CFL scan of
    test_reconstruct_scan_of_odd_size: within 1e-2 of the same script's fp32 output."""
    from dl_cs.config import load_cfg
    from dl_cs.data.dataset import SyntheticCineDataset
    from dl_cs.fileio import cfl
    S, E, C, Tt, Y, X = 2, 1, 4, 9, 11, 14
    rc = A._script("reconstruct_cbam" if fam == "cbam" else "reconstruct")
    cfg_file = tmp_path / "c.yaml"
    cfg_file.write_text(A.CFG.format(model_type=A.MODEL_TYPE[fam], out=str(tmp_path / "out")))
    fresh = rc.build_model(load_cfg(str(cfg_file)))
    recipe.fill_module(fresh, 161)
    A._spread(fam, fresh)
    ck = tmp_path / "m.ckpt"
    torch.save(fresh.state_dict(), ck)
    ds = SyntheticCineDataset(S, lambda k, m, t, f: (k, m), coils=C, emaps=E, frames=Tt, ny=Y, nx=X, seed=5)
    ks = np.stack([ds[i][0] for i in range(S)]).astype(np.complex64)
    mp = np.stack([ds[i][1] for i in range(S)]).astype(np.complex64)
    ks[:, :, :, ::3] = 0
    cfl.write(str(tmp_path / "ks"), ks.transpose(4, 3, 0, 1, 2).reshape(X, Y, S, C, 1, 1, 1, Tt), order='F')
    cfl.write(str(tmp_path / "maps"), mp[:, :, :, 0].transpose(4, 3, 0, 2, 1), order='F')
    ims = {}
    for dt in ("fp32", "bf16"):
        args = rc.create_arg_parser().parse_args(["--directory", str(tmp_path), "--ckpt", str(ck), "--config-file",
                                                  str(cfg_file), "--device", "0", "--dtype", dt])
        rc.main(args)
        ims[dt] = cfl.read(str(tmp_path / "im.dl"), order='F').copy()
    assert ims["bf16"].shape == (X, Y, S, 1, E, 1, 1, Tt) and np.isfinite(ims["bf16"]).all()
    e = float(np.linalg.norm(ims["bf16"] - ims["fp32"]) / np.linalg.norm(ims["fp32"]))
    print(f"{fam} reconstruct 9x11x14 --dtype bf16 vs fp32: NRMSE {e:.3g}")
    assert 0 < e < 1e-2


# ---------------------------------------------------------------------------- 8
@pytest.mark.parametrize("shape", [(1, 1, 8, 16, 16), (1, 1, 7, 10, 13)], ids=lambda s: "x".join(map(str, s[2:])))
@_fam
def test_fp32_calls_no_bf16_wrapper(fam, shape, monkeypatch):
    """fp32 forward + backward with every bf16 wrapper of _ops replaced by one that raises."""
    from dl_cs.models import _ops as K

    def refuse(*a, **k):
        raise AssertionError("a bf16 wrapper was called on the fp32 path")
    for name in ("box_pre_bf16", "box_post_bwd_bf16", "box_zero_bf16", "bf16_rows_call"):
        monkeypatch.setattr(K, name, refuse)
    A._fp32()
    net = A._net(fam, 2, 64, 16, 151)
    xg = recipe.crandn(152, shape).to(DEV).requires_grad_()
    out, caps = A._capture(lambda: net(xg))
    out.abs().sum().backward()
    assert caps[0]["relu_inputs"][0].dtype == torch.float32
    assert bool(torch.isfinite(torch.view_as_real(xg.grad)).all())
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
