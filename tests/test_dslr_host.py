"""Host-side checks of the DSLR family: the script's architecture table, the shipped
config, the state_dict schema against the reference's key lists, weight sharing."""
import importlib.util
import os

import pytest
import torch

import dslr_oracle as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cfg(arch="dslr-cg-v1", **over):
    from dl_cs.config import get_cfg
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE = arch
    P, m = cfg.MODEL.PARAMETERS, D.MODEL
    P.NUM_UNROLLS, P.NUM_RESBLOCKS, P.NUM_FEATURES, P.NUM_EMAPS = m["unrolls"], m["resblocks"], m["features"], m["E"]
    P.CONV_BLOCK.COMPLEX, P.CONV_BLOCK.CIRCULAR_PAD, P.FIX_STEP_SIZE = False, True, False
    P.DSLR.BLOCK_SIZE, P.DSLR.NUM_BASIS, P.DSLR.OVERLAPPING, P.DSLR.NUM_CG_STEPS = m["b"], m["r"], True, m["cg"]
    for k, v in over.items():
        setattr(P, k, v)
    return cfg


def test_train_lr_architecture_table():
    """train_lr.py:39-50, including 'dslr-cg-v2' -> AltMinCGv1 as the reference has it."""
    from dl_cs.models import dslr
    mod = _script("train_lr")
    want = {"dslr-pgd": dslr.AltMinPGD, "dslr-cg-v1": dslr.AltMinCGv1, "dslr-cg-v2": dslr.AltMinCGv1,
            "modslr-v1": dslr.AltMinMoDLv1, "modslr-v2": dslr.AltMinMoDLv2}
    for arch, cls in want.items():
        assert type(mod.build_model(_cfg(arch))) is cls, arch
    with pytest.raises(ValueError):
        mod.build_model(_cfg("dslr"))


def test_config_dslr_yaml():
    from dl_cs.config import load_cfg
    from dl_cs.models import dslr
    cfg = load_cfg(os.path.join(REPO, "configs", "config_dslr.yaml"))
    P = cfg.MODEL.PARAMETERS
    assert cfg.MODEL.META_ARCHITECTURE == "dslr-cg-v1"
    assert (P.NUM_UNROLLS, P.NUM_RESBLOCKS, P.NUM_FEATURES, P.NUM_EMAPS) == (10, 2, 128, 2)
    assert (P.DSLR.NUM_BASIS, P.DSLR.BLOCK_SIZE, P.DSLR.OVERLAPPING, P.DSLR.NUM_CG_STEPS) == (8, 16, True, 10)
    model = _script("train_lr").build_model(cfg)
    assert type(model) is dslr.AltMinCGv1 and model.num_cg_iter == 10
    assert len(model.spatial_cnn_update) == 10 and len(model.temporal_cnn_update[0].res_blocks) == 2
    w = model.spatial_cnn_update[0].init_layer.layers[2].conv.weight
    assert tuple(w.shape) == (128, 2 * 2 * 8, 3, 3)
    assert tuple(model.temporal_cnn_update[0].init_layer.layers[2].conv.weight.shape) == (128, 16, 3)
    assert model.temporal_cnn_update[0].pad_size == 6               # T = 20: 20 + 12 = 32, a multiple of 4


@pytest.mark.parametrize("arch", D.ARCHS)
def test_state_dict_schema(golden, arch):
    from dl_cs.models import dslr
    g = golden("dslr")
    cls = {"pgd": dslr.AltMinPGD, "cg-v1": dslr.AltMinCGv1, "cg-v2": dslr.AltMinCGv2, "modl-v1": dslr.AltMinMoDLv1,
           "modl-v2": dslr.AltMinMoDLv2}[arch]
    model = cls(_cfg())
    assert sorted(model.state_dict().keys()) == [str(k) for k in g[f"{arch}_state_keys"]]
    shapes = D.param_shapes(arch)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == shapes
    if arch.startswith("modl"):
        lam = D.LAMBDA_INIT[arch]
        assert model.lambda_l.item() == pytest.approx(lam[0]) and model.lambda_r.item() == pytest.approx(lam[1])
        assert model.lambda_l.requires_grad
        fixed = cls(_cfg(FIX_STEP_SIZE=True))
        assert not fixed.lambda_l.requires_grad and not fixed.lambda_r.requires_grad


def test_share_weights_aliases_one_network():
    from dl_cs.models import dslr
    model = dslr.AltMinCGv2(_cfg(SHARE_WEIGHTS=True))
    assert model.spatial_cnn_update[0] is model.spatial_cnn_update[1]
    sd = model.state_dict()
    a = sd["spatial_cnn_update.0.init_layer.layers.2.conv.weight"]
    b = sd["spatial_cnn_update.1.init_layer.layers.2.conv.weight"]
    assert a.data_ptr() == b.data_ptr()


def test_cpu_tensors_are_refused():
    """No silent eager fallback: the networks need GPU tensors."""
    from dl_cs.models import resnet2d
    net = resnet2d.ResNet(num_resblocks=1, in_chans=4, chans=8, kernel_size=3)
    with pytest.raises(RuntimeError):
        net(torch.zeros((3, 2, 4, 4), dtype=torch.complex64))
