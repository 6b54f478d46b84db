"""Generate tests/golden/anygrid.npz by importing the REFERENCE's unrolled ResNet, SE and
CBAM networks at grids that are no multiples of 4.

Runs only where the reference is present (see make_golden.py):

    python tests/golden/make_golden_anygrid.py

The reference models are dl_cs/models/unrolled.py, unrolledSE.py and unrolledCBAM.py
ProximalGradientDescent: 2 unrolls, 2 blocks, 64 features, 1 emap, RR 16 (pad_size 6, so
T >= 6 for torch's circular pad) at B, E, C = 1, 1, 4 and the three grids (T, Y, X) below.
They give T + 12 = 19, 21, 22, and between them every axis sees the remainders 1, 2 and 3
modulo 4.  Data seeds 82-85 as in the `resnet` fixture, fwd + bwd of the complex-L1 loss;
keys {res,se,cbam}_{T}x{Y}x{X}_{pred,loss,norm::*,grad::*} (norm:: for every parameter,
grad:: for those stored whole).

Fill seeds: 81 for the ResNet, 181 for SE (then se_oracle.scale_fc_weights) and 281 for
CBAM (then cbam_oracle.spread_gates).  With seed 81 the SE and the CBAM net each put an FC1
pre-activation within 1e-3 rms of 0 on one of the grids; with 181 / 281 all three grids
pass the asserts of make_golden_se.py / make_golden_cbam.py, kept here: gate min < 0.25
and max > 0.75, for CBAM the spatial map below 0.7 and above 1.3, min |FC1
pre-activation| / rms >= 1e-3.  Nothing of the reference is copied: inputs are
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
import cbam_oracle  # noqa: E402
import se_oracle  # noqa: E402

GRIDS = [(7, 10, 13), (9, 11, 14), (10, 13, 9)]
FILL = {"res": 81, "se": 181, "cbam": 281}


def _hooks(fam, model, gates, pre1, smaps):
    hooks = []
    keep = lambda dst: (lambda m, i, o: dst.append(o.detach().clone()))   # noqa: E731
    for net in model.cnn_update:
        for blk in getattr(net, "se_res_blocks", []):
            if fam == "se":
                hooks.append(blk.layers2.register_forward_hook(keep(gates)))
                hooks.append(blk.layers2.layers[1].register_forward_hook(keep(pre1)))
            else:
                hooks.append(blk.CAmodule.register_forward_hook(keep(gates)))
                hooks.append(blk.CAmodule[0].layers[0].register_forward_hook(keep(pre1)))
                hooks.append(blk.SAmodule.register_forward_hook(keep(smaps)))
    return hooks


def gen_anygrid():
    T = MG._import_ref()[0]
    import dl_cs.models.unrolled as ur
    import dl_cs.models.unrolledCBAM as ucb
    import dl_cs.models.unrolledSE as use
    mods = {"res": ur, "se": use, "cbam": ucb}
    out = {}
    B, E, C = 1, 1, 4
    for fam in ("res", "se", "cbam"):
        for (Tt, Y, X) in GRIDS:
            torch.manual_seed(0)
            cfg = MG._pgd_cfg(2)
            P = cfg.MODEL.PARAMETERS
            P.NUM_RESBLOCKS, P.NUM_FEATURES, P.NUM_EMAPS, P.RR = 2, 64, 1, 16
            model = mods[fam].ProximalGradientDescent(cfg)
            model.eval()
            recipe.fill_module(model, FILL[fam])
            if fam == "se":
                assert se_oracle.scale_fc_weights(model) == 8
            if fam == "cbam":
                assert cbam_oracle.spread_gates(model) == 16
            maps = recipe.sense_maps(82, B, E, C, Y, X)
            mask = recipe.binary_mask(83, (B, 1, Tt, Y, X))
            y = recipe.crandn(84, (B, C, Tt, Y, X)) * mask
            target = recipe.crandn(85, (B, E, Tt, Y, X))
            gates, pre1, smaps = [], [], []
            hooks = _hooks(fam, model, gates, pre1, smaps)
            pred = model(y=y, A=T.SenseModel(maps, weights=mask), x0=None)
            for h in hooks:
                h.remove()
            loss = torch.mean(torch.abs(target - pred))
            loss.backward()
            loss = loss.detach()
            tag = f"{fam}_{Tt}x{Y}x{X}_"
            msg = f"{tag}: loss {float(loss):.6g}"
            if fam != "res":
                g = torch.cat([t.reshape(-1) for t in gates])
                z = torch.cat([t.reshape(-1) for t in pre1])
                rel = float(z.abs().min() / z.pow(2).mean().sqrt())
                msg += f"; gates {float(g.min()):.3f} .. {float(g.max()):.3f}; min |FC1 pre-activation| / rms {rel:.3g}"
                assert float(g.min()) < 0.25 and float(g.max()) > 0.75, "the x8 FC weights no longer spread the gates"
                assert rel >= 1e-3, "an FC1 pre-activation sits within 1e-3 rms of 0: the hidden ReLU would be a coin flip"
                out[tag + "gate_range"] = np.array([float(g.min()), float(g.max()), rel])
            if fam == "cbam":
                q = torch.cat([t.reshape(-1) for t in smaps])
                msg += f"; spatial maps {float(q.min()):.3f} .. {float(q.max()):.3f}"
                assert float(q.min()) < 0.7 and float(q.max()) > 1.3, "the x32 SA weights no longer spread the spatial map"
                out[tag + "map_range"] = np.array([float(q.min()), float(q.max())])
            print(msg)
            MG._put(out, tag + "pred", MG._c(pred))
            out[tag + "loss"] = np.array(float(loss))
            MG._grad_summary(tag, model.named_parameters(), out)
    # nine cases in one file of at most 1 MiB: a gradient above GRAD_FULL_MAX elements (the
    # 64 -> 64 convs) keeps its norm:: entry only, not the 4096-element sample
    out = {k: v for k, v in out.items() if "grad::" not in k or "@" not in k}
    MG._save("anygrid", **out)


if __name__ == "__main__":
    gen_anygrid()
