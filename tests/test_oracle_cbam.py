"""The CBAM-ResNet family (MODEL_TYPE 'CBAM') on the CPU: tests/cbam_oracle.py vs goldens
the reference's unrolledCBAM network produced (tests/golden/make_golden_cbam.py), the
HIP module's state_dict key set, the restrictions, and the entry points' model
dispatch.  Tolerances as test_oracle_se.py::test_se_pgd2_loss_and_grads."""
import importlib.util
import os

import pytest
import torch

import cbam_oracle
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


def _shape(g, name):
    return tuple(g[f"cbam2_grad::{name}"].shape) if f"cbam2_grad::{name}" in g else tuple(g[f"cbam2_grad::{name}@shape"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "f64"])
def test_cbam_pgd2_loss_and_grads(golden, dtype):
    """The restatement vs the reference: prediction, loss, parameter gradients (after the
    recipe fill: CA FC weights x8, SA conv weights x32, SA biases + 1, as the generator applies)."""
    g = golden("cbam")
    torch.set_num_threads(8)
    B, E, C, T, Y, X = 1, 1, 8, 20, 32, 32
    names = grad_keys(g, "cbam2_")
    assert any(".CAmodule.0.layers.0.fc.weight" in n for n in names) and any(".SAmodule.0.layers.0.conv.bias" in n for n in names)
    cdt = torch.complex64 if dtype == torch.float32 else torch.complex128
    Ps = []
    for i in range(2):
        pre = f"cnn_update.{i}."
        P = {n[len(pre):]: recipe.param_value(81, n, _shape(g, n)) for n in names if n.startswith(pre)}
        assert cbam_oracle.spread_gates(P) == 8
        Ps.append({k: v.to(dtype).requires_grad_() for k, v in P.items()})
    maps = recipe.sense_maps(82, B, E, C, Y, X).to(cdt)
    mask = recipe.binary_mask(83, (B, 1, T, Y, X))
    y = (recipe.crandn(84, (B, C, T, Y, X)) * mask).to(cdt)
    target = recipe.crandn(85, (B, E, T, Y, X)).to(cdt)
    stats = []
    pred = O.pgd(Ps, y, maps, mask.to(dtype), reg=lambda P, x: cbam_oracle.cbamresnet(P, x, stats=stats))
    loss = O.l1(target, pred)
    loss.backward()
    gates = torch.cat([s.reshape(-1) for s, _, _ in stats])
    zs = torch.cat([z.reshape(-1) for _, z, _ in stats])
    qs = torch.cat([q.reshape(-1) for _, _, q in stats])
    rel = float(zs.abs().min() / zs.pow(2).mean().sqrt())
    print(f"oracle gates {float(gates.min()):.4g} .. {float(gates.max()):.4g}, maps {float(qs.min()):.4g} .. "
          f"{float(qs.max()):.4g}, FC1 margin {rel:.3g}; reference {g['cbam2_gate_range']} {g['cbam2_map_range']}")
    assert float(gates.min()) < 0.25 and float(gates.max()) > 0.75
    assert float(qs.min()) < 0.7 and float(qs.max()) > 1.3
    assert rel >= 1e-3
    assert golden_err(g, "cbam2_pred", pred.detach()) < TOL
    assert abs(float(loss.detach()) - float(g["cbam2_loss"])) < 1e-5 * float(g["cbam2_loss"])
    grads = {f"cnn_update.{i}.{k}": v.grad for i, P in enumerate(Ps) for k, v in P.items() if v.grad is not None}
    for name in names:
        assert name in grads, name
        assert golden_err(g, f"cbam2_grad::{name}", grads[name]) < 1e-3, name


def test_cbam_state_dict_keys(golden):
    """The HIP modules' key set is the reference's, for PGD and HQS (constructed on the CPU, no forward)."""
    from dl_cs.models import unrolledCBAM
    g = golden("cbam")
    ref_keys = {str(k) for k in g["cbam2_state_keys"]}
    assert len(ref_keys) == 1 + 2 * (4 + 2 * 10)
    model = unrolledCBAM.ProximalGradientDescent(_cfg("CBAM"))
    assert set(model.state_dict()) == ref_keys
    named = dict(model.named_parameters())
    for k in grad_keys(g, "cbam2_"):
        assert tuple(named[k].shape) == _shape(g, k), k
    assert named["cnn_update.0.se_res_blocks.1.CAmodule.0.layers.0.fc.weight"].shape == (16, 64)
    assert named["cnn_update.1.se_res_blocks.0.CAmodule.0.layers.2.fc.weight"].shape == (64, 16)
    assert named["cnn_update.1.se_res_blocks.1.SAmodule.0.layers.0.conv.weight"].shape == (1, 1, 5, 5, 5)
    hqs = unrolledCBAM.HalfQuadraticSplitting(_cfg("CBAM", arch="modl"))
    assert set(hqs.state_dict()) - {"lamda"} == ref_keys - {"step_size"}
    assert "lamda" in hqs.state_dict()


def test_cbam_restrictions():
    from dl_cs.models import CBAM
    ok = dict(num_resblocks=1, in_chans=2, chans=8, kernel_size=3, rr=4)
    CBAM.CBAMResNet(**ok)
    for bad in (dict(kernel_size=5), dict(act_type="leaky_relu"), dict(circular_pad=False),
                dict(use_complex_layers=True), dict(chans=1025), dict(rr=257)):
        with pytest.raises(NotImplementedError):
            CBAM.CBAMResNet(**{**ok, **bad})
    with pytest.raises(ValueError):
        CBAM.GlobalAvgPool("voxel")
    with pytest.raises(NotImplementedError):
        CBAM.GlobalMaxPool("spatial")(torch.zeros(1, 2, 4, 4, 4))
    net = CBAM.CBAMResNet(**ok)
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 1, 4, 4, 4, dtype=torch.complex64))       # no CPU fallback in the product path


@pytest.mark.parametrize("script", ["train_cbam", "reconstruct_cbam"])
def test_cbam_build_model_dispatch(script):
    from dl_cs.models import unrolledCBAM
    mod = _script(script)
    assert type(mod.build_model(_cfg("CBAM", n=1))) is unrolledCBAM.ProximalGradientDescent
    assert type(mod.build_model(_cfg("CBAM", n=1, arch="modl"))) is unrolledCBAM.HalfQuadraticSplitting
    for mt in ("SE", "RES", "SWIN", "DIT"):
        with pytest.raises(NotImplementedError):
            mod.build_model(_cfg(mt, n=1))
    with pytest.raises(ValueError):
        mod.build_model(_cfg("CBAM", n=1, arch="other"))


def test_builder_argument_defaults():
    """The shared mains take the builder as an optional argument that defaults to their own build_model."""
    import inspect
    for name in ("train_swin", "reconstruct"):
        mod = _script(name)
        assert inspect.signature(mod.main).parameters["builder"].default is None


def test_config_cbam_yaml():
    from dl_cs.config import load_cfg
    cfg = load_cfg(os.path.join(REPO, "configs", "config_cbam.yaml"))
    assert cfg.MODEL.MODEL_TYPE == "CBAM" and cfg.MODEL.PARAMETERS.RR == 16
    body = lambda name: [ln for ln in open(os.path.join(REPO, "configs", name)).read().splitlines()     # noqa: E731
                         if not ln.startswith("#")]
    se = [ln.replace('MODEL_TYPE: "SE"', 'MODEL_TYPE: "CBAM"').replace('"runs/se"', '"runs/cbam"')
          for ln in body("config_se.yaml")]
    assert body("config_cbam.yaml") == se, "config_cbam.yaml is config_se.yaml with the model type (and output directory) changed"
    model = _script("train_cbam").build_model(cfg)
    assert type(model).__module__ == "dl_cs.models.unrolledCBAM"
    assert len(model.cnn_update) == 5 and len(model.cnn_update[0].se_res_blocks) == 2
