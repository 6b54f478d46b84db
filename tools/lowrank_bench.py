"""Time the locally low-rank block kernels (csrc/lowrank.hip) and what the DSLR family builds
from them at the shipped configuration (configs/config_dslr.yaml): E, T, Y, X = 2, 20, 192,
160, 16 x 16 blocks at stride 8 (525 blocks), rank 8, 8 coils.

  a. each of the five kernels: time and algorithmic bytes/s (the operands it must read and
     the result it must write, from the shapes), against the 8 TB/s HBM peak.  Every
     operand here (at most 43 MB) fits the 256 MiB Infinity Cache, so a rate can exceed HBM's;
  b. one low-rank normal application  L -> extract(A^H A combine(L R^H)) R:
     fused (dlcs_lr_compose, dlcs_sense_normal, dlcs_lr_project_l) against unfused
     (torch.bmm, dlcs_lr_combine, dlcs_sense_normal, dlcs_lr_extract, torch.bmm) on the same
     inputs, alternating; and their outputs are compared (NRMSE);
  c. one forward + backward of the 2-D and of the 1-D CNN (2 resblocks, 128 features) in both
     compute dtypes -- fp32 on the generic conv3d_k3 kernels with the 3 x 3 / 3-tap weights
     embedded in 27 taps, bf16 on the plane conv (csrc/conv2d.hip) -- beside one 10-step CG
     solve for L (11 normal applications);
  d. the initialiser: dlcs_lr_decompose (the block SVD kernel, HIP events) against
     Decompose(svd='host') called with the same GPU image (copy to the host, extract and
     torch.linalg.svd there, copy back; wall time around a synchronised call), on a rank-r
     image with 1 % noise and on a Gaussian image, with the kernel's sweep counts
     (--svd-only runs this part alone).

One process; the variants alternate inside every round; each sample is HIP events around
`reps` calls after a warm-up; median and minimum over the rounds.  --markdown FILE writes the
tables of DESIGN.md's section from the medians.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from se_bench import DEV, HBM_PEAK, emit, interleaved, sample  # noqa: E402  (also puts the package on sys.path)

from dl_cs.models import _ops as K  # noqa: E402


def crandn(*shape):
    return torch.randn(*shape, dtype=torch.complex64, device=DEV)


def svd_part(args, lr, op, md):
    """d. the initialiser on the device against the host path, in the same process."""
    E, Tt, Y, X = args.shape
    b, r = args.block, args.rank
    host = lr.Decompose(b, r, [1, E, Tt, Y, X], True)
    u, v = crandn(r, E, 1, Y, X), crandn(r, 1, Tt, 1, 1)
    scale = (0.75 ** torch.arange(r, device=DEV, dtype=torch.float32)).reshape(r, 1, 1, 1, 1)
    images = {"rank-r + 1 % noise": ((scale * u * v).sum(0) + 0.01 * crandn(E, Tt, Y, X)).contiguous(),
              "Gaussian": crandn(E, Tt, Y, X)}
    md += ["", "| initial factors of one image | median ms | min ms | sweeps (blocks) |", "|---|---|---|---|"]
    for tag, img in images.items():
        dev_fn = lambda: lr.decompose_blocks(img, op, r)

        def host_fn():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host(img[None])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6
        for _ in range(3):
            dev_fn()
        host_fn()
        td, th = [], []
        for _ in range(args.rounds):                       # the two alternate inside every round
            td.append(sample(dev_fn, args.reps))
            th.append(host_fn())
        info = lr.decompose_blocks(img, op, r, return_info=True)[2].cpu()
        hist = {int(k): int((info == k).sum()) for k in info.unique()}
        Ld, Rd = dev_fn()
        Lh, Rh = host(img[None])
        ref = torch.bmm(Lh, Rh.conj().transpose(1, 2))
        diff = float((torch.bmm(Ld, Rd.conj().transpose(1, 2)) - ref).norm() / ref.norm())
        for name, t in (("dlcs_lr_decompose", td), ("Decompose(svd='host'), GPU image", th)):
            emit(dict(what="decompose", image=tag, variant=name, median_us=statistics.median(t), min_us=min(t),
                      sweeps=hist, device_vs_host_nrmse=diff), args.out)
        hs = ", ".join(f"{k}: {n}" for k, n in hist.items())
        md += [f"| dlcs_lr_decompose, {tag} | {statistics.median(td) / 1e3:.3f} | {min(td) / 1e3:.3f} | {hs} |",
               f"| Decompose(svd='host') on the same GPU image, copies included | {statistics.median(th) / 1e3:.1f} | "
               f"{min(th) / 1e3:.1f} | |"]
        md += [f"| L R^H of the two, NRMSE | {diff:.2e} | | |"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[2, 20, 192, 160], metavar=("E", "T", "Y", "X"))
    ap.add_argument("--block", type=int, default=16)
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--coils", type=int, default=8)
    ap.add_argument("--features", type=int, default=128)
    ap.add_argument("--resblocks", type=int, default=2)
    ap.add_argument("--cg-steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--svd-only", action="store_true", help="only part d, the initialiser")
    ap.add_argument("--out", default=None, help="append one JSON line per measurement")
    ap.add_argument("--markdown", default=None, help="write the result tables as markdown")
    args = ap.parse_args()

    from dl_cs.models import resnet1d, resnet2d, swin3D
    from dl_cs.mri import lowrank as lr, transforms as T
    from dl_cs.mri.algorithms import ConjugateGradient
    swin3D.set_compute_dtype(torch.float32)
    torch.manual_seed(0)
    E, Tt, Y, X = args.shape
    b, r, C = args.block, args.rank, args.coils
    op = lr.ArrayToBlocks(b, [1, E, Tt, Y, X], True).to(DEV)
    N, P = op.num_blocks, E * b * b
    img, blocks, L, R = crandn(E, Tt, Y, X), crandn(N, P, Tt), crandn(N, P, r), crandn(N, Tt, r)
    c8 = lambda t: t.numel() * 8
    md = [f"Shapes: image {E} x {Tt} x {Y} x {X} ({c8(img) / 1e6:.1f} MB), {N} blocks of {b} x {b}, block tensor "
          f"{c8(blocks) / 1e6:.1f} MB, L {c8(L) / 1e6:.1f} MB, R {c8(R) / 1e6:.2f} MB; rank {r}, {C} coils.", ""]
    if args.svd_only:
        with torch.no_grad():
            svd_part(args, lr, op, md)
        return finish(md, args)

    # ---- a. the five kernels
    nbytes = {"extract": c8(img) + c8(blocks), "combine": c8(blocks) + c8(img), "compose": c8(L) + c8(R) + c8(img),
              "project_l": c8(img) + c8(R) + c8(L), "project_r": c8(img) + c8(L) + c8(R)}
    with torch.no_grad():
        res = interleaved({
            "extract": lambda: lr._extract_raw(op, img, False),
            "combine": lambda: lr._combine_raw(op, blocks, True),
            "compose": lambda: lr._compose_raw(op, L, R, True),
            "project_l": lambda: lr._project_l_raw(op, img, R, False),
            "project_r": lambda: lr._project_r_raw(op, img, L, False)}, args.rounds, args.reps)
    md += ["| kernel | median us | min us | algorithmic MB | TB/s | of the 8 TB/s HBM peak |", "|---|---|---|---|---|---|"]
    for k, (med, mn) in res.items():
        rate = nbytes[k] / (med * 1e-6)
        emit(dict(what="kernel", kernel=k, median_us=med, min_us=mn, bytes=nbytes[k], tb_per_s=rate / 1e12,
                  of_hbm_peak=rate / HBM_PEAK), args.out)
        md.append(f"| dlcs_lr_{k} | {med:.1f} | {mn:.1f} | {nbytes[k] / 1e6:.1f} | {rate / 1e12:.2f} | {rate / HBM_PEAK:.2f} |")

    # ---- b. one normal application, fused against unfused
    maps = crandn(1, E, C, 1, Y, X)
    maps = maps / torch.sqrt((maps.abs() ** 2).sum(dim=(1, 2), keepdim=True))
    mask = (torch.rand((1, 1, Tt, Y, X), device=DEV) < 0.1).float()
    A = T.SenseModel(maps, weights=mask)
    bt = lambda m: m.conj().transpose(1, 2)

    def fused():
        x = lr._compose_raw(op, L, R, True)
        return lr._project_l_raw(op, A.normal(x[None], 0.0)[0], R, False)

    def unfused():
        x = lr._combine_raw(op, torch.bmm(L, bt(R)), True)
        return torch.bmm(lr._extract_raw(op, A.normal(x[None], 0.0)[0], False), R)

    def sense_only():
        return A.normal(img[None], 0.0)
    with torch.no_grad():
        a, u = fused(), unfused()
        diff = float((a - u).abs().pow(2).sum().sqrt() / u.abs().pow(2).sum().sqrt())
        res = interleaved({"fused": fused, "unfused": unfused, "sense_normal": sense_only}, args.rounds, args.reps)
    for k, (med, mn) in res.items():
        emit(dict(what="normal", variant=k, median_us=med, min_us=mn, fused_vs_unfused_nrmse=diff), args.out)
    f, uf, sn = res["fused"][0], res["unfused"][0], res["sense_normal"][0]
    md += ["", "| one normal application | median us | min us |", "|---|---|---|",
           f"| fused: compose, SENSE normal, project_l | {f:.1f} | {res['fused'][1]:.1f} |",
           f"| unfused: bmm, combine, SENSE normal, extract, bmm | {uf:.1f} | {res['unfused'][1]:.1f} |",
           f"| the SENSE normal operator alone | {sn:.1f} | {res['sense_normal'][1]:.1f} |", "",
           f"Fused / unfused time {f / uf:.3f}; block half alone (minus the SENSE normal) {f - sn:.1f} us against "
           f"{uf - sn:.1f} us; outputs agree to NRMSE {diff:.2e}."]

    # ---- c. the CNNs beside one CG solve
    net2 = resnet2d.ResNet(args.resblocks, 2 * r * E, args.features, 3).to(DEV)
    net1 = resnet1d.ResNet(args.resblocks, 2 * r, args.features, 3, circular_pad=True).to(DEV)
    x2 = crandn(N, r * E, b, b).requires_grad_()
    x1 = crandn(N, r, Tt).requires_grad_()

    def train(net, x, dtype=torch.float32):
        def fn():
            swin3D.set_compute_dtype(dtype)                   # read by the network at every call
            net.zero_grad(set_to_none=True)
            x.grad = None
            torch.sum(net(x).abs() ** 2).backward()
        return fn

    def cg():
        with torch.no_grad():
            normal = lambda q: lr._project_l_raw(op, A.normal(lr._compose_raw(op, q, R, True)[None], 0.0)[0], R, False)
            return ConjugateGradient(normal, args.cg_steps)(L, lr._project_l_raw(op, img, R, False))
    bf = torch.bfloat16
    res = interleaved({"cnn2d_fwd_bwd": train(net2, x2), "cnn2d_fwd_bwd_bf16": train(net2, x2, bf),
                       "cnn1d_fwd_bwd": train(net1, x1), "cnn1d_fwd_bwd_bf16": train(net1, x1, bf), "cg_solve_L": cg},
                      args.rounds, max(1, args.reps // 5))
    swin3D.set_compute_dtype(torch.float32)
    for k, (med, mn) in res.items():
        emit(dict(what="unroll_part", part=k, median_us=med, min_us=mn), args.out)
    ms = lambda k: f"{res[k][0] / 1e3:.2f} | {res[k][1] / 1e3:.2f}"
    ratio = lambda k: f"{res[k][0] / res[k + '_bf16'][0]:.2f}"
    md += ["", "| part of one unroll | fp32 median ms | fp32 min ms | bf16 median ms | bf16 min ms | fp32 / bf16 |",
           "|---|---|---|---|---|---|",
           f"| 2-D CNN forward + backward ([{N}, {2 * r * E}, {b}, {b}], {args.features} features, {args.resblocks} "
           f"resblocks) | {ms('cnn2d_fwd_bwd')} | {ms('cnn2d_fwd_bwd_bf16')} | {ratio('cnn2d_fwd_bwd')} |",
           f"| 1-D CNN forward + backward ([{N}, {2 * r}, {Tt} + {2 * net1.pad_size}]) | {ms('cnn1d_fwd_bwd')} | "
           f"{ms('cnn1d_fwd_bwd_bf16')} | {ratio('cnn1d_fwd_bwd')} |",
           f"| one {args.cg_steps}-step CG solve for L, forward ({args.cg_steps + 1} normal applications) | "
           f"{ms('cg_solve_L')} | | | |"]
    with torch.no_grad():
        svd_part(args, lr, op, md)
    finish(md, args)


def finish(md, args):
    text = "\n".join(md) + "\n"
    print(text)
    if args.markdown:
        with open(args.markdown, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
