"""Time the CBAM spatial-gate passes (csrc/cbam.hip) at the benchmark slice, 28 x 192 x 160
voxels (860,160 rows), for F = 64 and 256, against the SE kernels that move the same rows:

  1. cbam_scale_res_relu vs se_scale_res_relu and cbam_bwd_apply vs se_bwd_apply: the same
     bytes plus a 1/F map (two for bwd_apply), by achieved bytes/s (aim >= 0.90 of the SE kernel);
  2. cbam_chan_mean vs se_pool (one tensor read) and cbam_bwd_rowdot vs se_bwd_reduce (three
     tensors read), same aim; cbam_bwd_reduce vs se_bwd_reduce is printed with them;
  3. the three map kernels (stencil5, its transposed form, stencil5_wgrad) in us each; the aim
     is that their sum stays below one se_pool call at F = 64;
  4. one training step of the 2-unroll, 2-block, 64-feature CBAM-ResNet PGD vs the same step
     of the SE-ResNet PGD (python tools/cbam_bench.py step), se_bench.py step's configuration.

One process, the variants alternate inside every round, each sample is HIP events around
`reps` launches; the median and the minimum over the rounds are printed, and one JSON line per
measurement.  An F = 64 tensor is 220 MB, inside the 256 MiB Infinity Cache, so those rates can
exceed HBM's; F = 256 (881 MB) streams from HBM.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from se_bench import DEV, HBM_PEAK, K, emit, interleaved  # noqa: E402

GRID = (1, 28, 192, 160)
N_SLICE = 28 * 192 * 160
# (cbam kernel, the SE kernel of the same rows, row-tensor bytes per element of each, maps per voxel of the cbam one)
PAIRS = [("cbam_scale_res_relu", "se_scale_res_relu", 12, 1), ("cbam_bwd_apply", "se_bwd_apply", 16, 2),
         ("cbam_chan_mean", "se_pool", 4, 1), ("cbam_bwd_rowdot", "se_bwd_reduce", 12, 1),
         ("cbam_bwd_reduce", "se_bwd_reduce", 12, 2)]


def kernels(args):
    pool64 = None
    for F in args.features:
        N, B = N_SLICE, 1
        n = N * F
        o, g, r = (torch.randn((N, F), device=DEV) for _ in range(3))
        out = torch.empty((N, F), device=DEV)
        gate = torch.rand((B, F), device=DEV)
        dm = torch.randn((B, F), device=DEV)
        small = torch.empty((B, F), device=DEV)
        q, da, m0 = (torch.randn(GRID, device=DEV) for _ in range(3))
        m1 = torch.empty(GRID, device=DEV)
        w5, b5 = torch.randn((125,), device=DEV), torch.randn((1,), device=DEV)
        dw5, db5 = torch.zeros((125,), device=DEV), torch.zeros((1,), device=DEV)
        variants = {
            "se_scale_res_relu": lambda: K.se_scale_res_relu(o, gate, r, B, N, F, out=out),
            "cbam_scale_res_relu": lambda: K.cbam_scale_res_relu(o, gate, q, r, GRID, F, out=out),
            "se_bwd_apply": lambda: K.se_bwd_apply(g, r, gate, dm, B, N, F, dout=out),
            "cbam_bwd_apply": lambda: K.cbam_bwd_apply(g, r, gate, q, da, dm, GRID, F, dout=out),
            "se_pool": lambda: K.se_pool(o, B, N, F, mean=small),
            "cbam_chan_mean": lambda: K.cbam_chan_mean(o, gate, GRID, F, out=m1),
            "se_bwd_reduce": lambda: K.se_bwd_reduce(g, r, o, B, N, F, dgate=small),
            "cbam_bwd_rowdot": lambda: K.cbam_bwd_rowdot(g, r, o, gate, GRID, F, dq=m1),
            "cbam_bwd_reduce": lambda: K.cbam_bwd_reduce(g, r, o, q, da, GRID, F, dgate=small),
            "stencil5": lambda: K.cbam_stencil5(m0, w5, b5, GRID, out=m1),
            "stencil5_transposed": lambda: K.cbam_stencil5(m0, w5, None, GRID, transposed=True, out=m1),
            "stencil5_wgrad": lambda: K.cbam_stencil5_wgrad(q, m0, GRID, dw5, db5),
        }
        nbytes = {c: bpe * n + 4 * N * maps for c, _, bpe, maps in PAIRS}
        nbytes.update({s: bpe * n for _, s, bpe, _ in PAIRS})
        nbytes.update(stencil5=8 * N, stencil5_transposed=8 * N, stencil5_wgrad=8 * N)
        res = interleaved(variants, args.rounds, args.reps)
        rate = {k: nbytes[k] / (res[k][0] * 1e-6) for k in res}
        for k, (med, mn) in res.items():
            print(f"F={F:3d} {k:20s}: median {med:8.1f} us  min {mn:8.1f} us  {rate[k] / 1e12:6.3f} TB/s "
                  f"({rate[k] / HBM_PEAK:.2f} of the 8 TB/s HBM peak)")
            emit(dict(what="kernel", F=F, rows=N, kernel=k, median_us=med, min_us=mn, bytes=nbytes[k],
                      tb_per_s=rate[k] / 1e12), args.out)
        ratios = {f"{c}_rate_over_{s}": rate[c] / rate[s] for c, s, _, _ in PAIRS}
        maps_us = sum(res[k][0] for k in ("stencil5", "stencil5_transposed", "stencil5_wgrad"))
        if F == 64:
            pool64 = res["se_pool"][0]
        print(f"F={F:3d} bytes/s vs the SE kernel (aim >= 0.90): " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
        print(f"F={F:3d} map kernels {maps_us:.1f} us per block" +
              (f" vs se_pool at F = 64 {pool64:.1f} us (aim: below)" if pool64 is not None else ""))
        emit(dict(what="ratios", F=F, map_kernels_us=maps_us, se_pool_f64_us=pool64, **ratios), args.out)
        del o, g, r, out
        torch.cuda.empty_cache()


def step(args):
    from oracle import recipe
    from dl_cs.config import get_cfg
    from dl_cs.models import swin3D, unrolledCBAM, unrolledSE
    from dl_cs.mri import transforms as T
    swin3D.set_compute_dtype(torch.float32)
    B, E, C, Tt, Y, X = 1, 1, 8, 16, 192, 160               # Tp = 16 + 2 * 6 = 28

    def make(mod):
        cfg = get_cfg()
        P = cfg.MODEL.PARAMETERS
        P.NUM_UNROLLS, P.NUM_RESBLOCKS, P.NUM_FEATURES, P.NUM_EMAPS, P.RR = 2, 2, 64, 1, 16
        P.CONV_BLOCK.COMPLEX, P.FIX_STEP_SIZE = False, True
        m = mod.ProximalGradientDescent(cfg)
        recipe.fill_module(m, 7)
        return m.to(DEV)

    maps = recipe.sense_maps(1, B, E, C, Y, X).to(DEV)
    mask = recipe.binary_mask(2, (B, 1, Tt, Y, X)).to(DEV)
    y = (recipe.crandn(3, (B, C, Tt, Y, X)).to(DEV) * mask)
    target = recipe.crandn(4, (B, E, Tt, Y, X)).to(DEV)
    A = T.SenseModel(maps, weights=mask)

    def train_step(m):
        def run():
            m.zero_grad(set_to_none=True)
            loss = torch.mean(torch.abs(target - m(y=y, A=A, x0=None)))
            loss.backward()
        return run

    steps = {"se": train_step(make(unrolledSE)), "cbam": train_step(make(unrolledCBAM))}
    res = interleaved(steps, args.rounds, 2)
    host = {}
    for k, fn in steps.items():                              # host time to enqueue one step (no synchronise inside)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        host[k] = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
    for k, (med, mn) in res.items():
        print(f"{k:5s} training step: median {med / 1e3:8.2f} ms  min {mn / 1e3:8.2f} ms  (host enqueue {host[k]:.2f} ms)")
    ratio = res["cbam"][0] / res["se"][0]
    print(f"CBAM / SE step time {ratio:.3f}")
    emit(dict(what="step", shape=[B, E, C, Tt, Y, X], se_ms=res["se"][0] / 1e3, cbam_ms=res["cbam"][0] / 1e3,
              se_min_ms=res["se"][1] / 1e3, cbam_min_ms=res["cbam"][1] / 1e3, cbam_over_se=ratio,
              se_host_enqueue_ms=host["se"], cbam_host_enqueue_ms=host["cbam"]), args.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", nargs="?", default="kernels", choices=["kernels", "step", "all"])
    ap.add_argument("--features", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="", help="append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cbam_bench needs a GPU")
    if args.what in ("kernels", "all"):
        kernels(args)
    if args.what in ("step", "all"):
        step(args)


if __name__ == "__main__":
    main()
