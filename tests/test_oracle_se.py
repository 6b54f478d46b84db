"""The SE-ResNet family (MODEL_TYPE 'SE') on the CPU: tests/se_oracle.py vs goldens the
reference's unrolledSE network produced (tests/golden/make_golden_se.py), the HIP
module's state_dict schema, and the entry points' model dispatch.  Tolerances as
test_oracle_float.py::test_resnet_pgd2_loss_and_grads."""
import importlib.util
import os

import pytest
import torch

import se_oracle
from goldutil import golden_err, grad_keys
from oracle import dlcs_oracle as O
from oracle import recipe

TOL = 1e-5
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cfg(model_type, n=2, arch="dlespirit"):
    from dl_cs.config import get_cfg
    cfg = get_cfg()
    cfg.MODEL.MODEL_TYPE, cfg.MODEL.META_ARCHITECTURE = model_type, arch
    P = cfg.MODEL.PARAMETERS
    P.NUM_UNROLLS, P.NUM_RESBLOCKS, P.NUM_SWINBLOCKS, P.NUM_FEATURES, P.NUM_EMAPS, P.RR = n, 2, 1, 64, 1, 16
    P.CONV_BLOCK.COMPLEX, P.FIX_STEP_SIZE = False, True
    if model_type == "SWIN":
        P.NUM_FEATURES = 160
    return cfg


def test_se_pgd2_loss_and_grads(golden):
    """The restatement vs the reference: prediction, loss, parameter gradients (SE FC
    weights x8 after the recipe fill, as the generator applies)."""
    g = golden("se")
    torch.set_num_threads(8)
    B, E, C, T, Y, X = 1, 1, 8, 20, 32, 32
    names = grad_keys(g, "se2_")
    assert any(".layers2.layers.1.fc.weight" in n for n in names) and any(".layers2.layers.3.fc.bias" in n for n in names)
    Ps = []
    for i in range(2):
        pre = f"cnn_update.{i}."
        shapes = {n[len(pre):]: tuple(g[f"se2_grad::{n}"].shape) if f"se2_grad::{n}" in g
                  else tuple(g[f"se2_grad::{n}@shape"]) for n in names if n.startswith(pre)}
        P = {k: recipe.param_value(81, pre + k, s) for k, s in shapes.items()}
        assert se_oracle.scale_fc_weights(P) == 4
        Ps.append({k: v.clone().requires_grad_() for k, v in P.items()})
    maps = recipe.sense_maps(82, B, E, C, Y, X)
    mask = recipe.binary_mask(83, (B, 1, T, Y, X))
    y = recipe.crandn(84, (B, C, T, Y, X)) * mask
    target = recipe.crandn(85, (B, E, T, Y, X))
    stats = []
    pred = O.pgd(Ps, y, maps, mask, reg=lambda P, x: se_oracle.seresnet(P, x, stats=stats))
    loss = O.l1(target, pred)
    loss.backward()
    gates = torch.cat([s.reshape(-1) for s, _ in stats])
    print("oracle gates", float(gates.min()), float(gates.max()), "reference", g["se2_gate_range"])
    assert float(gates.min()) < 0.25 and float(gates.max()) > 0.75
    assert golden_err(g, "se2_pred", pred.detach()) < TOL
    assert abs(float(loss.detach()) - float(g["se2_loss"])) < 1e-5 * float(g["se2_loss"])
    grads = {f"cnn_update.{i}.{k}": v.grad for i, P in enumerate(Ps) for k, v in P.items() if v.grad is not None}
    for name in names:
        assert name in grads, name
        assert golden_err(g, f"se2_grad::{name}", grads[name]) < 1e-3, name


def test_se_state_dict_schema(golden):
    """The HIP module's parameters cover the reference's (constructed on the CPU, no forward)."""
    from dl_cs.models import unrolledSE
    g = golden("se")
    model = unrolledSE.ProximalGradientDescent(_cfg("SE"))
    named = dict(model.named_parameters())
    keys = grad_keys(g, "se2_")
    assert set(keys) <= set(named), sorted(set(keys) - set(named))
    for k in keys:
        shape = tuple(g[f"se2_grad::{k}"].shape) if f"se2_grad::{k}" in g else tuple(g[f"se2_grad::{k}@shape"])
        assert tuple(named[k].shape) == shape, k
    assert named["cnn_update.0.se_res_blocks.1.layers2.layers.1.fc.weight"].shape == (16, 64)
    assert named["cnn_update.1.se_res_blocks.0.layers2.layers.3.fc.weight"].shape == (64, 16)
    hqs = unrolledSE.HalfQuadraticSplitting(_cfg("SE", arch="modl"))
    assert set(hqs.state_dict()) - {"lamda"} == set(model.state_dict()) - {"step_size"}


def test_se_restrictions():
    from dl_cs.models import se3d
    ok = dict(num_resblocks=1, in_chans=2, chans=8, kernel_size=3, rr=4)
    se3d.SeResNet(**ok)
    for bad in (dict(kernel_size=5), dict(act_type="leaky_relu"), dict(circular_pad=False),
                dict(use_complex_layers=True), dict(chans=1025), dict(rr=257)):
        with pytest.raises(NotImplementedError):
            se3d.SeResNet(**{**ok, **bad})


@pytest.mark.parametrize("script", ["reconstruct", "train_swin", "train_se", "reconstruct_h5"])
def test_build_model_dispatch(script):
    from dl_cs.models import unrolled, unrolledSE, unrolledswin
    mod = _script(script)
    build = (lambda cfg: mod.build_model(cfg, cfg.MODEL.MODEL_TYPE)) if script == "reconstruct_h5" else mod.build_model
    for mt, m in (("SE", unrolledSE), ("RES", unrolled), ("SWIN", unrolledswin)):
        assert type(build(_cfg(mt, n=1))) is m.ProximalGradientDescent, mt
        assert type(build(_cfg(mt, n=1, arch="modl"))) is m.HalfQuadraticSplitting, mt
    with pytest.raises(NotImplementedError):
        build(_cfg("CBAM", n=1))


def test_config_se_yaml():
    from dl_cs.config import load_cfg
    cfg = load_cfg(os.path.join(REPO, "configs", "config_se.yaml"))
    assert cfg.MODEL.MODEL_TYPE == "SE" and cfg.MODEL.PARAMETERS.RR == 16
    model = _script("train_se").build_model(cfg)
    assert type(model).__module__ == "dl_cs.models.unrolledSE"
    assert len(model.cnn_update) == 5 and len(model.cnn_update[0].se_res_blocks) == 2
