"""Time one regulariser call, forward plus backward, of the ResNet, SE and CBAM families (the
shipped configs: 2 blocks, 64 features, RR 16, 1 emap, pad_size 6) in fp32 and in bf16
(swin3D.set_compute_dtype) at two grids:

  mult4 x [1, 1, 8, 192, 160]: 20 x 192 x 160, the unpadded path
  odd   x [1, 1, 8, 190, 158]: the box 20 x 190 x 158 on the padded path in 20 x 192 x 160

and the 64 x 64 weight gradient alone on (1, 20, 192, 160): the bf16 tap-row kernel
(conv3d_wgrad_row.inc) beside the fp32 generic kernel, both at the voxel range the trunks pass.

The yardstick of a bf16 time is the fp32 time of the same call in the same process: one process,
the variants alternate inside every round, each sample is HIP events around `reps` calls after a
warm-up; the median and the minimum over the rounds and the bf16 / fp32 ratio are printed, one
JSON line per pair.  No threshold is set.  For the weight gradient the achieved TFLOP/s
(2 x 27 x 64 x 64 x voxels per call) is given against the dense bf16 peak that bench.py uses.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from se_bench import DEV, emit, interleaved  # noqa: E402
from anygrid_bench import GRIDS, nets  # noqa: E402

BF16_DENSE_TFLOPS = 2500.0             # bench.py: MI355X_BF16_DENSE_TFLOPS
WG_GRID = (1, 20, 192, 160)
F = 64


def call(net, x, dy, dtype):
    from dl_cs.models import swin3D

    def run():
        swin3D.set_compute_dtype(dtype)
        net.zero_grad(set_to_none=True)
        x.grad = None
        (net(x) * dy).real.sum().backward()
    return run


def wgrad_variants():
    from dl_cs.models import _ops as K
    from dl_cs.models import resnet3d
    rows = WG_GRID[0] * WG_GRID[1] * WG_GRID[2] * WG_GRID[3]
    g = torch.Generator(device="cpu").manual_seed(5)
    x32 = torch.randn((rows, F), generator=g).to(DEV)
    g32 = torch.randn((rows, F), generator=g).to(DEV)
    dwp = torch.zeros((27, F, F), device=DEV)
    xb, gb = x32.bfloat16(), g32.bfloat16()
    return {"wgrad64_fp32": lambda: K.conv3d_wgrad(x32, F, 0, g32, F, WG_GRID, dwp),
            "wgrad64_bf16": lambda: K.conv3d_wgrad(xb, F, 0, gb, F, WG_GRID, dwp,
                                                   vox_per_block=resnet3d.WGRAD_VOX_BF16)}, rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="", help="append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("trunk_dtype_bench needs a GPU")
    from oracle import recipe
    from dl_cs.models import swin3D
    dev = torch.cuda.get_device_name(0)
    variants = {}
    for fam, net in nets().items():
        for tag, (T, Y, X) in GRIDS.items():
            x = recipe.crandn(11, (1, 1, T, Y, X)).to(DEV).requires_grad_()
            dy = recipe.crandn(12, (1, 1, T, Y, X)).to(DEV)
            for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
                variants[f"{fam}_{tag}_{name}"] = call(net, x, dy, dt)
    try:
        res = interleaved(variants, args.rounds, args.reps)
    finally:
        swin3D.set_compute_dtype(torch.float32)
    for k, (med, mn) in res.items():
        print(f"{k:16s} fwd + bwd: median {med / 1e3:8.3f} ms  min {mn / 1e3:8.3f} ms")
    for fam in ("res", "se", "cbam"):
        for tag in GRIDS:
            f, b = res[f"{fam}_{tag}_fp32"], res[f"{fam}_{tag}_bf16"]
            print(f"{fam:5s} {tag:5s} bf16 / fp32 {b[0] / f[0]:.4f}")
            emit(dict(what="trunk_dtype", family=fam, grid=tag, device=dev, fp32_ms=f[0] / 1e3, bf16_ms=b[0] / 1e3,
                      fp32_min_ms=f[1] / 1e3, bf16_min_ms=b[1] / 1e3, bf16_over_fp32=b[0] / f[0], rounds=args.rounds,
                      reps=args.reps), args.out)
    wv, rows = wgrad_variants()
    wres = interleaved(wv, args.rounds, 10)
    flop = 2.0 * 27 * F * F * rows
    f, b = wres["wgrad64_fp32"], wres["wgrad64_bf16"]
    for k, (med, mn) in wres.items():
        print(f"{k:16s} median {med:9.1f} us  min {mn:9.1f} us  {flop / med / 1e6:7.1f} TFLOP/s")
    print(f"wgrad 64 x 64 bf16 / fp32 {b[0] / f[0]:.4f}; bf16 at {flop / b[0] / 1e6 / BF16_DENSE_TFLOPS:.4f} of the "
          f"dense bf16 peak ({BF16_DENSE_TFLOPS:.0f} TFLOP/s)")
    emit(dict(what="wgrad64", grid=list(WG_GRID), device=dev, fp32_us=f[0], bf16_us=b[0], fp32_min_us=f[1],
              bf16_min_us=b[1], bf16_over_fp32=b[0] / f[0], bf16_tflops=flop / b[0] / 1e6,
              bf16_frac_of_dense_peak=flop / b[0] / 1e6 / BF16_DENSE_TFLOPS, rounds=args.rounds, reps=10), args.out)


if __name__ == "__main__":
    main()
