"""The DSLR family on the GPU (dl_cs.models.dslr, resnet2d, resnet1d over mri/lowrank's
block kernels) against tests/golden/dslr.npz and the float64 oracle tests/dslr_oracle.py
at the fixture's case A: E, C, T, Y, X = 2, 4, 8, 12, 20; b = 4, r = 3; 8 features,
1 resblock, 2 unrolls, 3 CG steps.

Bars: outputs NRMSE <= 1e-5; gradients per tensor <= max(1e-5, 4 x the fp32 oracle's own
distance from float64) (goldutil.assert_f64_floor).  The reference's fp32 run sits
<= 6e-7 (output) and <= 7e-7 (gradients) from its float64 run at this case; those two
distances are stored in the fixture and test_oracle_dslr.py asserts them < 2.5e-6.  That no
ReLU decision flips between the two runs is asserted by the generator when it writes the
fixture; it is not stored.
"""
import importlib.util
import json
import math
import os

import pytest
import torch

import dslr_oracle as D
import goldutil
from oracle import recipe

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = {"pgd": "AltMinPGD", "cg-v1": "AltMinCGv1", "cg-v2": "AltMinCGv2", "modl-v1": "AltMinMoDLv1",
           "modl-v2": "AltMinMoDLv2"}
_ORACLE = {}


def _cfg(**over):
    from dl_cs.config import get_cfg
    cfg = get_cfg()
    P, m = cfg.MODEL.PARAMETERS, D.MODEL
    P.NUM_UNROLLS, P.NUM_RESBLOCKS, P.NUM_FEATURES, P.NUM_EMAPS = m["unrolls"], m["resblocks"], m["features"], m["E"]
    P.CONV_BLOCK.COMPLEX, P.CONV_BLOCK.CIRCULAR_PAD, P.FIX_STEP_SIZE = False, True, False
    P.SHARE_WEIGHTS, P.GRAD_CHECKPOINT = False, False
    P.DSLR.BLOCK_SIZE, P.DSLR.NUM_BASIS, P.DSLR.OVERLAPPING, P.DSLR.NUM_CG_STEPS = m["b"], m["r"], True, m["cg"]
    for k, v in over.items():
        setattr(P, k, v)
    return cfg


def _model(arch, **over):
    from dl_cs.models import dslr, swin3D
    swin3D.set_compute_dtype(torch.float32)
    model = getattr(dslr, CLASSES[arch])(_cfg(**over))
    model.eval()
    return D.fill(model, D.MODEL["seed"]).cuda()


def _run(model, g, arch):
    """One forward + backward of the complex-L1 loss on the fixture inputs."""
    from dl_cs.mri import lowrank, transforms as T
    m = D.MODEL
    maps, mask, y, target = (t.cuda() for t in D.model_inputs())
    op = lowrank.ArrayToBlocks(m["b"], [1, m["E"], m["T"], m["Y"], m["X"]], True).cuda()
    kw = {}
    if arch == "pgd":
        v = torch.from_numpy(g["pgd_v0"]).cuda()
        kw["v0"] = [(v[2 * i], v[2 * i + 1]) for i in range(m["unrolls"])]
    model.zero_grad()
    pred = model(y=y, A=T.SenseModel(maps, weights=mask), BlockOp=op, L0=torch.from_numpy(g["L0"]).cuda(),
                 R0=torch.from_numpy(g["R0"]).cuda(), **kw)
    loss = torch.mean(torch.abs(target - pred))
    loss.backward()
    grads = {n: p.grad.detach().cpu() for n, p in model.named_parameters() if p.grad is not None}
    return pred.detach().cpu(), float(loss.detach()), grads


def _oracle(g, arch, share=False):
    """The fp32 and float64 oracle runs of a network, computed once."""
    key = (arch, share)
    if key not in _ORACLE:
        _ORACLE[key] = (D.oracle_run(g, arch, torch.float32, share), D.oracle_run(g, arch, torch.float64, share))
    return _ORACLE[key]


@pytest.mark.parametrize("arch", D.ARCHS)
def test_network_fwd_bwd(golden, arch):
    g = golden("dslr")
    model = _model(arch)
    assert sorted(model.state_dict().keys()) == [str(k) for k in g[f"{arch}_state_keys"]]
    pred, loss, grads = _run(model, g, arch)
    e = D.nrmse(g[f"{arch}_pred"], pred[0].numpy())
    print(f"{arch}: output NRMSE vs the reference {e:.3g}, loss {loss:.6g} (reference {float(g[arch + '_loss']):.6g})")
    assert tuple(pred.shape) == (1,) + tuple(g[f"{arch}_pred"].shape)
    assert e <= 1e-5
    assert abs(loss - float(g[f"{arch}_loss"])) <= 1e-5 * abs(loss)
    (_, _, o32), (_, _, o64) = _oracle(g, arch)
    assert sorted(grads) == [str(k) for k in g[f"{arch}_grad_names"]]
    goldutil.assert_f64_floor(grads, {k: v.numpy() for k, v in o32.items()}, {k: v.numpy() for k, v in o64.items()},
                              f"dslr {arch}")


def test_share_weights_aliasing(golden):
    g = golden("dslr")
    model = _model("cg-v2", SHARE_WEIGHTS=True)
    assert model.spatial_cnn_update[0] is model.spatial_cnn_update[1]
    assert model.temporal_cnn_update[0] is model.temporal_cnn_update[1]
    assert len(list(model.parameters())) == len(list(_model("cg-v2").parameters())) // 2
    assert len(model.state_dict()) == len(g["cg-v2_state_keys"])         # both aliases are listed, as in the reference
    pred, _, grads = _run(model, g, "cg-v2")
    (_, _, o32), (p64, _, o64) = _oracle(g, "cg-v2", share=True)
    assert D.nrmse(p64.numpy(), pred[0].numpy()) <= 1e-5
    pick = lambda o: {k: v.numpy() for k, v in o.items()}             # the oracle used (and differentiated) net 0 only
    assert sorted(grads) == sorted(o64) and all(".0." in k for k in grads)
    goldutil.assert_f64_floor(grads, pick(o32), pick(o64), "dslr cg-v2 shared")


@pytest.mark.parametrize("arch", ["cg-v1", "modl-v2"])
def test_grad_checkpoint_same_gradients(golden, arch):
    g = golden("dslr")
    res = []
    for ck in (False, True):
        model = _model(arch, GRAD_CHECKPOINT=ck)
        model.train()
        assert model.do_checkpoint is ck
        res.append(_run(model, g, arch))
    (p0, _, g0), (p1, _, g1) = res
    assert D.nrmse(p0.numpy(), p1.numpy()) <= 1e-6
    assert sorted(g0) == sorted(g1)
    for k in g0:
        assert D.nrmse(g0[k].numpy(), g1[k].numpy()) <= 1e-6, k


def test_state_dict_round_trip(golden):
    g = golden("dslr")
    a = _model("modl-v1")
    b = _model("modl-v1")
    with torch.no_grad():
        for p in b.parameters():
            p.add_(0.01)
    missing = b.load_state_dict({k: v.cpu() for k, v in a.state_dict().items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    pa, _, _ = _run(a, g, "modl-v1")
    pb, _, _ = _run(b, g, "modl-v1")
    assert torch.equal(torch.view_as_real(pa), torch.view_as_real(pb))


def _net_case(kind):
    from dl_cs.models import resnet1d, resnet2d, swin3D
    swin3D.set_compute_dtype(torch.float32)
    if kind == "2d":                              # 77 blocks: not a multiple of 4, the grid pads to 80
        net = resnet2d.ResNet(num_resblocks=2, in_chans=12, chans=8, kernel_size=3)
        x = recipe.crandn(31, (77, 6, 4, 4))
        f = lambda P, v, acts=None: D.resnet2d(P, "", v, 2, acts=acts)
    else:                                         # 77 sequences (80 grid positions), T = 12 + 2 * 6 = 24
        net = resnet1d.ResNet(num_resblocks=2, in_chans=6, chans=8, kernel_size=3, circular_pad=True)
        x = recipe.crandn(32, (77, 3, 12))
        f = lambda P, v, acts=None: D.resnet1d(P, "", v, 2, acts=acts)
    recipe.fill_module(net, 33)
    return net, x, f


@pytest.mark.parametrize("kind", ["2d", "1d"])
def test_resnet_alone(kind):
    """ResNet2D / ResNet1D forward, input gradient and parameter gradients against the oracle."""
    net, x, f = _net_case(kind)
    w = recipe.crandn(34, tuple(x.shape))
    net = net.cuda()
    xg = x.cuda().requires_grad_()
    out = net(xg)
    torch.sum((out * w.cuda().conj()).real).backward()
    hip = {n: p.grad.detach().cpu() for n, p in net.named_parameters()}
    hip["input"] = xg.grad.detach().cpu()
    res = {}
    for dt, cd in ((torch.float32, torch.complex64), (torch.float64, torch.complex128)):
        P = {k: v.detach().cpu().to(dt).clone().requires_grad_() for k, v in net.state_dict().items()}
        xi = x.to(cd).clone().requires_grad_()
        acts = []
        o = f(P, xi, acts)
        torch.sum((o * w.to(cd).conj()).real).backward()
        gr = {k: p.grad.numpy() for k, p in P.items()}
        gr["input"] = xi.grad.numpy()
        res[dt] = (o.detach(), gr, acts)
    flips = sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(res[torch.float32][2], res[torch.float64][2]))
    e = D.nrmse(res[torch.float64][0].numpy(), out.detach().cpu().numpy())
    print(f"resnet{kind}: output NRMSE {e:.3g}; fp32 / float64 oracle ReLU flips {flips}")
    assert tuple(out.shape) == tuple(x.shape) and e <= 1e-5
    goldutil.assert_f64_floor(hip, res[torch.float32][1], res[torch.float64][1], f"resnet{kind}")


def test_unsupported_raise():
    from dl_cs.models import dslr, resnet1d, resnet2d
    with pytest.raises(NotImplementedError):
        resnet2d.ResNet(num_resblocks=1, in_chans=4, chans=8, kernel_size=3, use_complex_layers=True)
    with pytest.raises(NotImplementedError):
        resnet1d.ResNet(num_resblocks=1, in_chans=4, chans=8, kernel_size=5)
    net = resnet1d.ResNet(num_resblocks=1, in_chans=4, chans=8, kernel_size=3, circular_pad=True).cuda()
    with pytest.raises(NotImplementedError):                      # 6 + 2 * 4 = 14: not a multiple of 4
        net(torch.zeros((5, 2, 6), dtype=torch.complex64, device="cuda"))
    cfg = _cfg()
    cfg.MODEL.PARAMETERS.CONV_BLOCK.COMPLEX = True
    with pytest.raises(NotImplementedError):
        dslr.AltMinCGv1(cfg)
    with pytest.raises(NotImplementedError):
        dslr.AltMinCGv1(_cfg()).init_recurrent_nets()


LR_CFG = """MODEL:
  META_ARCHITECTURE: "{arch}"
  PARAMETERS:
    NUM_UNROLLS: 2
    NUM_RESBLOCKS: 1
    NUM_FEATURES: 8
    NUM_EMAPS: 2
    FIX_STEP_SIZE: False
    SLWIN_INIT: True
    GRAD_CHECKPOINT: True
    DSLR:
      NUM_BASIS: 3
      BLOCK_SIZE: 4
      OVERLAPPING: True
      NUM_CG_STEPS: 3
    CONV_BLOCK:
      COMPLEX: False
      CIRCULAR_PAD: True
  RECON_LOSS:
    NAME: "complex_l1"
    RENORMALIZE_DATA: False
AUG_TRAIN:
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


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_lr_script(tmp_path):
    """scripts/train_lr.py: two optimiser steps of the MoDL v1 network on synthetic slices
    (GPU preprocessing with the host SVD, checkpointed unrolls), validation, checkpoints."""
    out = tmp_path / "out"
    cfg = tmp_path / "dslr.yaml"
    cfg.write_text(LR_CFG.format(out=str(out), arch="modslr-v1"))
    tr = _script("train_lr")
    tr.main(["--config-file", str(cfg), "--data", "synthetic", "--synthetic-slices", "2",
             "--synthetic-shape", "4", "2", "8", "16", "24"])
    recs = [json.loads(line) for line in (out / "exp" / "metrics.jsonl").read_text().splitlines()]
    train = [r for r in recs if "Train/complex_l1" in r]
    val = [r for r in recs if "Validate/complex_l1" in r]
    assert len(train) == 2 and len(val) == 1
    assert all(math.isfinite(r["Train/complex_l1"]) for r in train) and math.isfinite(val[0]["Validate/complex_l1"])
    ck = torch.load(out / "last.ckpt", weights_only=True)
    assert ck["global_step"] == 2
    keys = list(ck["state_dict"])
    assert any(k.endswith("spatial_cnn_update.1.final_layer.layers.2.conv.weight") for k in keys)
    assert any(k.endswith("lambda_l") for k in keys)


def test_preprocess_lr_decom_gpu():
    """CinePreprocess(lr_decom=True, device='cuda'): eight items; the fused compose of
    (L_init, R_init) is the combine of the rank-r truncation of init_image's blocks."""
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
    res = CinePreprocess(cfg, lr_decom=True, use_seed=True, device="cuda")(k, maps, target, "slice.h5")
    assert len(res) == 8
    masked, mask, mp, L, R, init, scale, tgt = res
    assert all(t.is_cuda for t in (masked, mask, mp, L, R, init, tgt))
    op = lowrank.ArrayToBlocks(4, [1, E, T, Y, X], True)
    assert tuple(L.shape) == (op.num_blocks, E * 16, 2) and tuple(R.shape) == (op.num_blocks, T, 2)
    geo = D.Geo(4, E, T, Y, X)
    U, S, Vh = torch.linalg.svd(D.extract(geo, init.cpu().to(torch.complex128)), full_matrices=False)
    trunc = D.combine(geo, (U[:, :, :2] * S[:, None, :2]) @ Vh[:, :2])
    got = lowrank.compose(L, R, op.cuda())
    assert D.nrmse(trunc.numpy(), got[0].cpu().numpy()) <= 1e-5
