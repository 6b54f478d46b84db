"""Generate tests/golden/cbam.npz by importing the REFERENCE's unrolledCBAM network.

Runs only where the reference is present (see make_golden.py):

    python tests/golden/make_golden_cbam.py

The reference model is dl_cs/models/unrolledCBAM.py ProximalGradientDescent with
CBAM.CBAMResNet: 2 unrolls, 2 blocks, 64 features, 1 emap, RR 16 at B, E, C, T, Y, X =
1, 1, 8, 20, 32, 32 -- the sizes and seeds of the `se` fixture (fill seed 81, data
seeds 82-85), fwd + bwd of the complex-L1 loss.  After recipe.fill_module the CA
fc.weights are multiplied by 8, the SA conv weights by 32 and 1.0 is added to the SA
biases (cbam_oracle.spread_gates): with the plain fill the channel gates sit in
0.48-0.53 and the spatial map near 0.007 +- 0.003, which kills the branch and would
hide any error in it.  An SA factor of 8 leaves an FC1 pre-activation 8e-4 of its RMS
from 0, too close to a coin flip on the hidden ReLU; hence 32.  The generator asserts
what it relies on: gate min < 0.25 and max > 0.75, spatial-map min < 0.7 and
max > 1.3, min |FC1 pre-activation| / rms >= 1e-3.  Nothing of the reference is
copied: inputs are regenerated from recipe seeds, expected outputs and the list of
state_dict keys are stored.
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
import cbam_oracle  # noqa: E402


def gen_cbam():
    T = MG._import_ref()[0]
    import dl_cs.models.unrolledCBAM as ucb
    out = {}
    torch.manual_seed(0)
    B, E, C, Tt, Y, X = 1, 1, 8, 20, 32, 32
    cfg = MG._pgd_cfg(2)
    P = cfg.MODEL.PARAMETERS
    P.NUM_RESBLOCKS, P.NUM_FEATURES, P.NUM_EMAPS, P.RR = 2, 64, 1, 16
    model = ucb.ProximalGradientDescent(cfg)
    model.eval()
    recipe.fill_module(model, 81)
    assert cbam_oracle.spread_gates(model) == 16           # 2 unrolls x 2 blocks x (2 FC weights, 5^3 weight, its bias)
    maps = recipe.sense_maps(82, B, E, C, Y, X)
    mask = recipe.binary_mask(83, (B, 1, Tt, Y, X))
    y = recipe.crandn(84, (B, C, Tt, Y, X)) * mask
    target = recipe.crandn(85, (B, E, Tt, Y, X))
    # the reference's own gates, FC1 pre-activations and spatial maps, through forward hooks
    gates, pre1, smaps = [], [], []
    hooks = []
    for net in model.cnn_update:
        for blk in net.se_res_blocks:
            hooks.append(blk.CAmodule.register_forward_hook(lambda m, i, o: gates.append(o.detach().clone())))
            hooks.append(blk.CAmodule[0].layers[0].register_forward_hook(lambda m, i, o: pre1.append(o.detach().clone())))
            hooks.append(blk.SAmodule.register_forward_hook(lambda m, i, o: smaps.append(o.detach().clone())))
    pred = model(y=y, A=T.SenseModel(maps, weights=mask), x0=None)
    for h in hooks:
        h.remove()
    loss = torch.mean(torch.abs(target - pred))
    loss.backward()
    g = torch.cat([t.reshape(-1) for t in gates])
    z = torch.cat([t.reshape(-1) for t in pre1])
    q = torch.cat([t.reshape(-1) for t in smaps])
    rel = float(z.abs().min() / z.pow(2).mean().sqrt())
    stds = ", ".join(f"{float(t.std()):.3f}" for t in smaps)
    print(f"gates {float(g.min()):.3f} .. {float(g.max()):.3f}; spatial maps {float(q.min()):.3f} .. {float(q.max()):.3f} "
          f"(mean {float(q.mean()):.3f}, per-block std {stds}); min |FC1 pre-activation| / rms {rel:.3g}; "
          f"loss {float(loss):.6g}")
    assert float(g.min()) < 0.25 and float(g.max()) > 0.75, "the x8 FC weights no longer spread the gates"
    assert float(q.min()) < 0.7 and float(q.max()) > 1.3, "the x32 SA weights no longer spread the spatial map"
    assert rel >= 1e-3, "an FC1 pre-activation sits within 1e-3 rms of 0: the hidden ReLU would be a coin flip"
    MG._put(out, "cbam2_pred", MG._c(pred))
    out["cbam2_loss"] = np.array(float(loss))
    out["cbam2_gate_range"] = np.array([float(g.min()), float(g.max()), rel])
    out["cbam2_map_range"] = np.array([float(q.min()), float(q.max())])
    out["cbam2_state_keys"] = np.array(sorted(model.state_dict().keys()))
    MG._grad_summary("cbam2_", model.named_parameters(), out)
    MG._save("cbam", **out)


if __name__ == "__main__":
    gen_cbam()
