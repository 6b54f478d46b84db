"""Time one DiTResNet and one LatteNet call, forward plus backward, (config widths: 384
features / 16 heads and 192 / 6, 2 layers, num_blocks 0 so pad_size 2) at two grids:

  odd   x [1, 2, 19, 190, 158]: the box 23 x 190 x 158 in the layout grid 24 x 192 x 160, the
        reference's token grid (DiT 12 x 48 x 40, Latte 23 frames of 48 x 40), crop shift (1, 1, 1)
  mult4 x [1, 2, 20, 192, 160]: 24 x 192 x 160 itself, no slack

and dlcs_box_shift on the [737,280, 384] fp32 rows of that layout grid (both directions, and
with the residual and ReLU of DiTResNet) beside a dlcs_axpby copy of the same bytes.

One process, the variants alternate inside every round, each sample is HIP events around
`reps` calls after a warm-up; the median and the minimum over the rounds are printed, and one
JSON line per network / kernel.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from se_bench import DEV, emit, interleaved  # noqa: E402

GRIDS = {"odd": (19, 190, 158), "mult4": (20, 192, 160)}


def nets():
    from oracle import recipe
    from dl_cs.models import DiT, Latte
    out = {"ditres": DiT.DiTResNet(num_blocks=0, in_chans=4, chans=384, kernel_size=3, num_heads=16, num_layers=2),
           "latte": Latte.LatteNet(num_blocks=0, in_chans=4, chans=192, kernel_size=3, num_heads=6, num_layers=2)}
    for k, n in out.items():
        n.eval()
        recipe.fill_module(n, 7)
        out[k] = n.to(DEV)
    return out


def call(net, x, dy, t, lab):
    def run():
        net.zero_grad(set_to_none=True)
        x.grad = None
        (net(x, t, lab) * dy).real.sum().backward()
    return run


def networks(args):
    from oracle import recipe
    t, lab = torch.tensor([500], device=DEV), torch.tensor([1], device=DEV)
    variants = {}
    for fam, net in nets().items():
        for tag, (T, Y, X) in GRIDS.items():
            x = recipe.crandn(11, (1, 2, T, Y, X)).to(DEV).requires_grad_()
            dy = recipe.crandn(12, (1, 2, T, Y, X)).to(DEV)
            variants[f"{fam}_{tag}"] = call(net, x, dy, t, lab)
    res = interleaved(variants, args.rounds, args.reps)
    for k, (med, mn) in res.items():
        print(f"{k:13s} fwd + bwd: median {med / 1e3:8.3f} ms  min {mn / 1e3:8.3f} ms")
    for fam in ("ditres", "latte"):
        odd, m4 = res[f"{fam}_odd"], res[f"{fam}_mult4"]
        print(f"{fam:7s} odd / mult4 {odd[0] / m4[0]:.4f} ({odd[0] - m4[0]:+.0f} us)")
        emit(dict(what="dit_anygrid", family=fam, device=torch.cuda.get_device_name(0), odd_box=[23, 190, 158],
                  mult4_grid=[24, 192, 160], odd_ms=odd[0] / 1e3, mult4_ms=m4[0] / 1e3, odd_min_ms=odd[1] / 1e3,
                  mult4_min_ms=m4[1] / 1e3, odd_over_mult4=odd[0] / m4[0], rounds=args.rounds, reps=args.reps), args.out)


def kernels(args):
    from dl_cs.models import _ops as K
    grid, box, shift, C = (1, 24, 192, 160), (1, 23, 190, 158), (1, 1, 1), 384
    V = grid[1] * grid[2] * grid[3]
    src, res, dst = (torch.randn((V, C), device=DEV) for _ in range(3))
    variants = {
        "axpby_copy": lambda: K.axpby(src, dst, 1.0, 0.0),
        "box_shift": lambda: K.box_shift(src, C, grid, box, shift, out=dst),
        "box_shift_T": lambda: K.box_shift(src, C, grid, box, shift, transpose=True, out=dst),
        "box_shift_res_relu": lambda: K.box_shift(src, C, grid, box, shift, out=dst, res=res, relu=True),
    }
    rd = {"axpby_copy": V, "box_shift": box[1] * box[2] * box[3], "box_shift_T": box[1] * box[2] * box[3],
          "box_shift_res_relu": 2 * box[1] * box[2] * box[3]}
    out = interleaved(variants, args.rounds, 10)
    for k, (med, mn) in out.items():
        nbytes = 4 * C * (rd[k] + V)                   # rows read + every row of the layout grid written
        print(f"{k:19s} median {med:8.1f} us  min {mn:8.1f} us  {nbytes / med / 1e6:6.2f} TB/s")
        emit(dict(what="box_shift", kernel=k, device=torch.cuda.get_device_name(0), rows=V, C=C, us=med, min_us=mn,
                  bytes=nbytes, tb_per_s=nbytes / med / 1e6), args.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only", choices=("networks", "kernels"), default=None)
    ap.add_argument("--out", default="", help="append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dit_anygrid_bench needs a GPU")
    from dl_cs.models import swin3D
    swin3D.set_compute_dtype(torch.float32)
    if args.only != "networks":
        kernels(args)
    if args.only != "kernels":
        networks(args)


if __name__ == "__main__":
    main()
