"""Time one regulariser call, forward plus backward, of the ResNet, SE and CBAM families
(the shipped configs: 2 blocks, 64 features, RR 16, 1 emap, so pad_size 6) at two grids:

  odd   x [1, 1, 8, 190, 158]: the box 20 x 190 x 158 runs on the padded path in 20 x 192 x 160
  mult4 x [1, 1, 8, 192, 160]: 20 x 192 x 160 itself, the unpadded path

Both execute the same convs, gates and reductions on 614,400 rows; the odd grid adds the box_zero
launches on the slack rows (14,000 of them) and takes box_pre / box_post (+ _bwd) for the
swin_* calls.  What is expected is a few launches' worth; no threshold is set.

One process, the six variants alternate inside every round, each sample is HIP events around
`reps` calls after a warm-up; the median and the minimum over the rounds are printed, and one
JSON line per family with the two medians and their ratio.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from se_bench import DEV, emit, interleaved  # noqa: E402

GRIDS = {"odd": (8, 190, 158), "mult4": (8, 192, 160)}


def nets():
    from oracle import recipe
    from dl_cs.models import CBAM, resnet3d, se3d
    kw = dict(num_resblocks=2, in_chans=2, chans=64, kernel_size=3)
    out = {"res": resnet3d.ResNet(**kw), "se": se3d.SeResNet(rr=16, **kw), "cbam": CBAM.CBAMResNet(rr=16, **kw)}
    for k, n in out.items():
        recipe.fill_module(n, 7)
        out[k] = n.to(DEV)
    return out


def call(net, x, dy):
    def run():
        net.zero_grad(set_to_none=True)
        x.grad = None
        (net(x) * dy).real.sum().backward()
    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="", help="append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("anygrid_bench needs a GPU")
    from oracle import recipe
    from dl_cs.models import swin3D
    swin3D.set_compute_dtype(torch.float32)
    variants = {}
    for fam, net in nets().items():
        for tag, (T, Y, X) in GRIDS.items():
            x = recipe.crandn(11, (1, 1, T, Y, X)).to(DEV).requires_grad_()
            dy = recipe.crandn(12, (1, 1, T, Y, X)).to(DEV)
            variants[f"{fam}_{tag}"] = call(net, x, dy)
    res = interleaved(variants, args.rounds, args.reps)
    for k, (med, mn) in res.items():
        print(f"{k:11s} fwd + bwd: median {med / 1e3:8.3f} ms  min {mn / 1e3:8.3f} ms")
    for fam in ("res", "se", "cbam"):
        odd, m4 = res[f"{fam}_odd"], res[f"{fam}_mult4"]
        print(f"{fam:5s} odd / mult4 {odd[0] / m4[0]:.4f} ({odd[0] - m4[0]:+.0f} us)")
        emit(dict(what="anygrid", family=fam, device=torch.cuda.get_device_name(0), odd_grid=[20, 190, 158],
                  mult4_grid=[20, 192, 160], odd_ms=odd[0] / 1e3, mult4_ms=m4[0] / 1e3, odd_min_ms=odd[1] / 1e3,
                  mult4_min_ms=m4[1] / 1e3, odd_over_mult4=odd[0] / m4[0], rounds=args.rounds, reps=args.reps), args.out)


if __name__ == "__main__":
    main()
