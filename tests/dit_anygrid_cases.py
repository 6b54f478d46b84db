"""The cases of tests/golden/dit_anygrid.npz (made by tests/golden/make_golden_dit_anygrid.py)
and how each network is built, filled and evaluated by the oracle: shared by the CPU
oracle test and the GPU tests."""
import torch

from oracle import dit_oracle as DO
from oracle import recipe

E = 2
# (B, T, Y, X); num_blocks = 0 -> pad 2, Tp = T + 4
CASES = [(1, 4, 8, 8), (1, 6, 8, 8), (1, 5, 8, 8), (1, 4, 6, 7), (1, 4, 5, 8), (2, 5, 10, 9)]
# tag -> (module, class, features, heads, fill seed, input seed, cotangent seed)
NETS = {"ditres": ("DiT", "DiTResNet", 384, 16, 301, 302, 303), "ditnet": ("DiT", "DiTNet", 384, 16, 301, 302, 303),
        "latte": ("Latte", "LatteNet", 192, 6, 501, 502, 503)}
TSTEPS = (37, 613)
# Input seed of the two DiT networks per case.  DiTResNet's final ConvBlock takes a ReLU of
# DiT(res) + res, B Tp Y X 384 values (up to 622,080 here); with the `dit` fixture's seed 302 the
# smallest |pre-activation| / rms of a case lies between 2e-7 and 2e-5, and below about 1e-6 --
# fp32 rounding of that sum -- the decision is a coin flip between two correct fp32 evaluations,
# which moves dx by 1e-3 to 1e-2 (the reason tests/test_gpu_dit.py compares DiTResNet's dx at
# fixed decisions only).  So each case takes the first seed of 302, 1302, 2302, ... whose smallest
# |pre-activation| / rms in the reference is >= 5e-6, ten times the HIP path's output error
# (5e-7); make_golden_dit_anygrid.py asserts that margin.
XSEED = {(1, 4, 8, 8): 2302, (1, 6, 8, 8): 1302, (1, 5, 8, 8): 1302, (1, 4, 6, 7): 1302, (1, 4, 5, 8): 302,
         (2, 5, 10, 9): 29302}
RELU_MARGIN = 5e-6
FROZEN = ("pos_embed_table", "temp_embed_table", "step_size", "x_unembedder")


def trainable(k):
    return not any(f in k for f in FROZEN)


def key(tag, case):
    return f"{tag}_" + "x".join(str(n) for n in case) + "_"


def build(tag):
    """The product model of one fixture network, filled from its recipe seed (CPU, eval)."""
    import importlib
    mod, cls, feats, heads, fill = NETS[tag][:5]
    net = getattr(importlib.import_module("dl_cs.models." + mod), cls)(
        num_blocks=0, in_chans=2 * E, chans=feats, kernel_size=3, num_heads=heads, num_layers=2)
    net.eval()
    recipe.fill_module(net, fill)
    return net


def inputs(tag, case):
    """x, t, labels and the output cotangent of one case."""
    B, T, Y, X = case
    x = recipe.crandn(NETS[tag][5] if tag == "latte" else XSEED[case], (B, E, T, Y, X))
    return x, torch.tensor(TSTEPS[:B]), torch.tensor([1] * B), recipe.crandn(NETS[tag][6], (B, E, T, Y, X))


def tables(tag):
    if tag == "latte":
        return dict(pos_table=DO.latte_pos_table(192), temp_table=DO.latte_temp_table(192))
    return dict(pos_table=DO.pos_embed_table(384))


def oracle(tag, P, x, t, lab, tabs, relu=None):
    """The oracle's forward of one fixture network on parameters P (tabs: tables(tag) cast
    to P's dtype)."""
    heads = NETS[tag][3]
    if tag == "latte":
        return DO.latte_net(P, x, t, 2, heads, **tabs)
    if tag == "ditnet":
        return DO.dit_net(P, x, t, lab, 2, heads, **tabs)
    kw = {} if relu is None else dict(relu=relu)
    return DO.dit_resnet(P, x, t, lab, 2, heads, **tabs, **kw)


def hip_masks(caps):
    """goldutil.HipMasks of CAPTURE entries; an entry of a grid with slack holds the padded
    grid's rows with the box beside it and is cropped to the box (goldutil.captured_masks
    assumes a grid without slack), after checking that nothing outside the box is positive."""
    from goldutil import HipMasks, captured_masks
    masks = HipMasks([])
    for cap in caps:
        ms = captured_masks(cap)
        if "box" in cap:
            B, D, H, W = cap["box"]
            assert cap["grid"] == (B,) + tuple((n + 3) // 4 * 4 for n in (D, H, W)) != cap["box"]
            for m in ms:
                out = m.clone()
                out[:, :, :D, :H, :W] = False
                assert not bool(out.any()), "a stored post-ReLU activation is non-zero on a slack row"
            ms = [m[:, :, :D, :H, :W].contiguous() for m in ms]
        masks.calls.append(ms)
    return masks


def captured(fn):
    from dl_cs.models import engine
    engine.CAPTURE = []
    try:
        out = fn()
    finally:
        caps, engine.CAPTURE = engine.CAPTURE, None
    return out, caps
