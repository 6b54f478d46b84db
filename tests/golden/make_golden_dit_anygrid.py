"""Generate tests/golden/dit_anygrid.npz by importing the REFERENCE's DiTResNet, DiTNet and
LatteNet at grids whose T + 2 pad, Y or X is no multiple of the patch.

Runs only where the reference is present (see make_golden.py):

    python tests/golden/make_golden_dit_anygrid.py

The networks are those of the `dit` and `latte` fixtures (make_golden.py gen_dit / gen_latte):
2 layers, num_blocks = 0 (pad_size 2, Tp = T + 4), DiTResNet / DiTNet at 384 features and 16
heads filled from seed 301, LatteNet at 192 features and 6 heads filled from seed 501; the
output cotangent from seed 303 (DiT) / 503 (Latte), LatteNet's input from seed 502 and the DiT
networks' from the per-case seed of tests/dit_anygrid_cases.py XSEED (the first of 302, 1302,
... that keeps every input of DiTResNet's final ReLU at least RELU_MARGIN rms away from 0,
asserted here), timesteps (37, 613)[:B], label 1.  The reference's patch embeds zero-pad the
end of each axis up to the patch (dit:30-53, :117-122; lat:126-129, :193-214) and unpatchify2
takes a centre crop (dit:539-541, lat:450-475).  Cases (B, T, Y, X):

    (1, 4, 8, 8)    nothing padded: control
    (1, 6, 8, 8)    Tp = 10: nothing padded, but no multiple of 4 frames
    (1, 5, 8, 8)    Tp = 9: DiT pads one frame (crop offset 1); an odd frame count for Latte
    (1, 4, 6, 7)    pads (2, 1), crop offsets (1, 1)
    (1, 4, 5, 8)    Y pad 3: crop offset 2, one row dropped at the end
    (2, 5, 10, 9)   all three axes, crop offsets (1, 1, 2), two batch items that differ

Keys {ditres,ditnet,latte}_{B}x{T}x{Y}x{X}_{y,dx}, stored whole.  Parameter gradients are
not stored: the tests hold them to the float64 oracle.  Nothing of the reference is copied:
inputs are regenerated from recipe seeds, expected outputs are stored.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (puts the repository root on sys.path)
from make_golden import recipe  # noqa: E402
import dit_anygrid_cases as AC  # noqa: E402  (the cases, seeds and inputs the tests use)


def gen_dit_anygrid():
    MG._import_ref()
    import dl_cs.models.DiT as dit
    import dl_cs.models.Latte as lat
    out = {}
    for tag, (mod, cls, feats, heads, fill, _, _) in AC.NETS.items():
        torch.manual_seed(0)
        net = getattr(lat if mod == "Latte" else dit, cls)(num_blocks=0, in_chans=2 * AC.E, chans=feats, kernel_size=3,
                                                           num_heads=heads, num_layers=2)
        net.eval()
        recipe.fill_module(net, fill)
        pre = []
        if tag == "ditres":                  # the inputs of the final ConvBlock's ReLU (dit:1344)
            relus = [m for m in net.final_layer.modules() if isinstance(m, torch.nn.ReLU)]
            assert len(relus) == 1
            relus[0].register_forward_pre_hook(lambda m, i: pre.append(i[0].detach().clone()))
        for case in AC.CASES:
            x, t, lab, g = AC.inputs(tag, case)
            x.requires_grad_()
            y = net(x, t, lab)
            assert y.shape == x.shape, (tag, case, y.shape)
            (y.real * g.real + y.imag * g.imag).sum().backward()
            msg = ""
            if tag == "ditres":
                v = pre.pop()
                rel = float(v.abs().min() / v.pow(2).mean().sqrt())
                assert not pre and rel >= AC.RELU_MARGIN, (case, rel, "a ReLU input within rounding of 0: pick the next seed")
                msg = f": min |ReLU input| / rms {rel:.3g} over {v.numel()}"
            out[AC.key(tag, case) + "y"] = y.detach().numpy()
            out[AC.key(tag, case) + "dx"] = x.grad.detach().numpy()
            print(AC.key(tag, case), "done" + msg)
    MG._save("dit_anygrid", **out)


if __name__ == "__main__":
    torch.set_num_threads(os.cpu_count())
    gen_dit_anygrid()
