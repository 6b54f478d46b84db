"""Time the squeeze-excitation passes (csrc/se.hip) at the benchmark slice, 28 x 192 x 160
voxels (860,160 rows), for F = 64 and 256, against the existing kernels of the same shape:

  1. se_pool (two-stage, deterministic) vs dlcs_colsum (fp32 atomics) on the same rows, B = 1;
  2. se_scale_res_relu, se_bwd_apply and se_bwd_reduce vs dlcs_axpby (fp32 -> fp32, b != 0: two
     reads and one write per element) on the same element count, by achieved bytes/s -- each
     pass scaled by its own bytes per element (12, 16, 12; axpby 12);
  3. one training step of the 2-unroll, 2-block, 64-feature SE-ResNet PGD vs the same step of
     the ResNet PGD (python tools/se_bench.py step).

Variants alternate inside one process; each sample is HIP events around `reps` launches; the
median and the minimum over the rounds are printed, and one JSON line per measurement.
An F = 64 tensor is 220 MB, inside the 256 MiB Infinity Cache, so those rates can exceed HBM's;
F = 256 (881 MB) streams from HBM.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dl-swin-gan_amd"))
from dl_cs.models import _ops as K  # noqa: E402

DEV = "cuda"
N_SLICE = 28 * 192 * 160
HBM_PEAK = 8.0e12


def sample(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per launch


def interleaved(variants, rounds, reps, between=None):
    """{name: fn} -> {name: (median us, min us)}; the variants alternate within every round."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            if between is not None:
                between()
            ts[k].append(sample(fn, reps))
    return {k: (statistics.median(v), min(v)) for k, v in ts.items()}


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def kernels(args):
    for F in args.features:
        N, B = N_SLICE, 1
        n = N * F
        o = torch.randn((N, F), device=DEV)
        g = torch.randn((N, F), device=DEV)
        r = torch.randn((N, F), device=DEV)
        out = torch.empty((N, F), device=DEV)
        gate = torch.rand((B, F), device=DEV)
        dm = torch.randn((B, F), device=DEV)
        mean = torch.empty((B, F), device=DEV)
        cs = torch.zeros((F,), device=DEV)
        y = torch.randn((N, F), device=DEV)
        variants = {
            "colsum": lambda: K.colsum(o, cs, rows=N, C=F, ld=F),
            "se_pool": lambda: K.se_pool(o, B, N, F, mean=mean),
            "axpby": lambda: K.axpby(o, y, 0.5, 0.5),
            "se_scale_res_relu": lambda: K.se_scale_res_relu(o, gate, r, B, N, F, out=out),
            "se_bwd_apply": lambda: K.se_bwd_apply(g, r, gate, dm, B, N, F, dout=out),
            "se_bwd_reduce": lambda: K.se_bwd_reduce(g, r, o, B, N, F, dgate=mean),
        }
        bytes_per_elt = {"colsum": 4, "se_pool": 4, "axpby": 12, "se_scale_res_relu": 12, "se_bwd_apply": 16,
                         "se_bwd_reduce": 12}
        res = interleaved(variants, args.rounds, args.reps, between=cs.zero_)
        rate = {k: bytes_per_elt[k] * n / (res[k][0] * 1e-6) for k in res}
        for k, (med, mn) in res.items():
            print(f"F={F:3d} {k:18s}: median {med:8.1f} us  min {mn:8.1f} us  {rate[k] / 1e12:5.2f} TB/s "
                  f"({rate[k] / HBM_PEAK:.2f} of the 8 TB/s HBM peak)")
            emit(dict(what="kernel", F=F, rows=N, kernel=k, median_us=med, min_us=mn, bytes=bytes_per_elt[k] * n,
                      tb_per_s=rate[k] / 1e12, of_hbm_peak=rate[k] / HBM_PEAK), args.out)
        print(f"F={F:3d} se_pool / colsum time {res['se_pool'][0] / res['colsum'][0]:.3f} (target <= 1.10); bytes/s vs axpby: "
              + ", ".join(f"{k} {rate[k] / rate['axpby']:.3f}" for k in ("se_scale_res_relu", "se_bwd_apply", "se_bwd_reduce"))
              + " (target >= 1 / 1.15 = 0.870)")
        emit(dict(what="ratios", F=F, pool_over_colsum=res["se_pool"][0] / res["colsum"][0],
                  **{k + "_rate_over_axpby": rate[k] / rate["axpby"]
                     for k in ("se_scale_res_relu", "se_bwd_apply", "se_bwd_reduce")}), args.out)
        del o, g, r, out, y
        torch.cuda.empty_cache()


def step(args):
    from oracle import recipe
    from dl_cs.config import get_cfg
    from dl_cs.models import swin3D, unrolled, unrolledSE
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

    steps = {"resnet": train_step(make(unrolled)), "se": train_step(make(unrolledSE))}
    res = interleaved(steps, args.rounds, 2)
    # host time to enqueue one step (no synchronise inside): a step whose enqueue takes as long as
    # the step itself is bound by the host, and kernels added to it do not show in its time
    host = {}
    for k, fn in steps.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        host[k] = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
    for k, (med, mn) in res.items():
        print(f"{k:7s} training step: median {med / 1e3:8.2f} ms  min {mn / 1e3:8.2f} ms  (host enqueue {host[k]:.2f} ms)")
    ratio = res["se"][0] / res["resnet"][0]
    print(f"SE / ResNet step time {ratio:.3f}")
    emit(dict(what="step", shape=[B, E, C, Tt, Y, X], resnet_ms=res["resnet"][0] / 1e3, se_ms=res["se"][0] / 1e3,
              resnet_min_ms=res["resnet"][1] / 1e3, se_min_ms=res["se"][1] / 1e3, se_over_resnet=ratio,
              resnet_host_enqueue_ms=host["resnet"], se_host_enqueue_ms=host["se"]), args.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", nargs="?", default="kernels", choices=["kernels", "step", "all"])
    ap.add_argument("--features", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="", help="append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("se_bench needs a GPU")
    if args.what in ("kernels", "all"):
        kernels(args)
    if args.what in ("step", "all"):
        step(args)


if __name__ == "__main__":
    main()
