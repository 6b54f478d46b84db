"""Generate tests/golden/se.npz by importing the REFERENCE's unrolledSE network.

Runs only where the reference is present (see make_golden.py):

    python tests/golden/make_golden_se.py

The reference model is dl_cs/models/unrolledSE.py ProximalGradientDescent with
se3d.SeResNet: 2 unrolls, 2 blocks, 64 features, 1 emap, RR 16 at B, E, C, T, Y, X =
1, 1, 8, 20, 32, 32 -- the sizes and seeds of the `resnet` fixture (fill seed 81, data
seeds 82-85), fwd + bwd of the complex-L1 loss.  After recipe.fill_module the four
SE FC weights (keys with '.layers2.') are multiplied by 8: with the plain fill the
gates sit in 0.475-0.520 and a wrong gate path would hide.  The generator asserts
the spread it relies on (gate min < 0.25, max > 0.75) and that the FC1
pre-activations stay >= 1e-3 of their RMS away from 0 (the hidden ReLU is not one
of the captured decisions).  Nothing of the reference is copied: inputs are
regenerated from recipe seeds, expected outputs are stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
from make_golden import recipe  # noqa: E402
import se_oracle  # noqa: E402


def gen_se():
    T = MG._import_ref()[0]
    import dl_cs.models.unrolledSE as use
    out = {}
    torch.manual_seed(0)
    B, E, C, Tt, Y, X = 1, 1, 8, 20, 32, 32
    cfg = MG._pgd_cfg(2)
    P = cfg.MODEL.PARAMETERS
    P.NUM_RESBLOCKS, P.NUM_FEATURES, P.NUM_EMAPS, P.RR = 2, 64, 1, 16
    model = use.ProximalGradientDescent(cfg)
    model.eval()
    recipe.fill_module(model, 81)
    assert se_oracle.scale_fc_weights(model) == 8          # 2 unrolls x 2 blocks x 2 FCs
    maps = recipe.sense_maps(82, B, E, C, Y, X)
    mask = recipe.binary_mask(83, (B, 1, Tt, Y, X))
    y = recipe.crandn(84, (B, C, Tt, Y, X)) * mask
    target = recipe.crandn(85, (B, E, Tt, Y, X))
    # the reference's own gates and FC1 pre-activations, through forward hooks
    gates, pre1 = [], []
    hooks = []
    for net in model.cnn_update:
        for blk in net.se_res_blocks:
            hooks.append(blk.layers2.register_forward_hook(lambda m, i, o: gates.append(o.detach().clone())))
            hooks.append(blk.layers2.layers[1].register_forward_hook(lambda m, i, o: pre1.append(o.detach().clone())))
    pred = model(y=y, A=T.SenseModel(maps, weights=mask), x0=None)
    for h in hooks:
        h.remove()
    loss = torch.mean(torch.abs(target - pred))
    loss.backward()
    g = torch.cat([t.reshape(-1) for t in gates])
    z = torch.cat([t.reshape(-1) for t in pre1])
    rel = float(z.abs().min() / z.pow(2).mean().sqrt())
    print(f"gates {float(g.min()):.3f} .. {float(g.max()):.3f}; min |FC1 pre-activation| / rms {rel:.3g}")
    assert float(g.min()) < 0.25 and float(g.max()) > 0.75, "the x8 FC weights no longer spread the gates"
    assert rel >= 1e-3, "an FC1 pre-activation sits within 1e-3 rms of 0: the hidden ReLU would be a coin flip"
    MG._put(out, "se2_pred", MG._c(pred))
    out["se2_loss"] = np.array(float(loss))
    out["se2_gate_range"] = np.array([float(g.min()), float(g.max()), rel])
    MG._grad_summary("se2_", model.named_parameters(), out)
    MG._save("se", **out)


if __name__ == "__main__":
    gen_se()
