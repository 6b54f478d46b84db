"""Generate tests/golden/dslr.npz by importing the REFERENCE's DSLR family.

Runs only where the reference is present (see make_golden.py):

    python tests/golden/make_golden_dslr.py

From dl_cs/mri/lowrank.py: the geometry, window weights, extract and combine of
ArrayToBlocks at the three operator cases of tests/dslr_oracle.py (A, B: odd sizes,
C: a zero-weight row), and Decompose at case A on a rank-2-plus-noise image (only
gauge-free quantities: the composed image and the singular values; the generator
asserts a relative gap (S_r - S_{r+1}) / S_1 >= 0.05 in every block).

From dl_cs/models/dslr.py: the five AltMin networks at case A (E, C, T, Y, X = 2, 4, 8,
12, 20; b = 4, r = 3; 8 features, 1 resblock, 2 unrolls, 3 CG steps), forward and
backward of the complex-L1 loss, run in fp32 and in float64.  Stored: L0, R0 (the SVD
gauge is arbitrary and the CNNs are not phase-equivariant, so they cannot be
regenerated), PGD's power-method start vectors as drawn, and per network the float64
output, loss, per-tensor gradient norms, a fixed sample of the concatenated gradient,
the fp32 run's own distance from float64 (output and gradient; asserted < 2.5e-6) and
the state_dict keys.  Everything else is regenerated from oracle/recipe seeds.

ReLU decisions: the volumes hold 1e4-1e5 pre-activations per layer, so some always lie
within 1e-3 rms of zero; what the fixture needs is that none of them flips between the
fp32 and the float64 run, which is what the generator counts and asserts (0 flips), and
it prints the smallest |pre-activation| / rms.  Nothing of the reference is copied.
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
import dslr_oracle as D  # noqa: E402


def _cfg():
    cfg = MG._pgd_cfg(D.MODEL["unrolls"])
    P = cfg.MODEL.PARAMETERS
    P.NUM_RESBLOCKS, P.NUM_FEATURES, P.NUM_EMAPS = D.MODEL["resblocks"], D.MODEL["features"], D.MODEL["E"]
    P.FIX_STEP_SIZE = False                                   # the MoDL penalties get gradients
    P.DSLR = MG._Cfg()
    P.DSLR.BLOCK_SIZE, P.DSLR.NUM_BASIS, P.DSLR.OVERLAPPING, P.DSLR.NUM_CG_STEPS = \
        D.MODEL["b"], D.MODEL["r"], True, D.MODEL["cg"]
    return cfg


def gen_operators(out, rlr):
    for tag, (b, E, T, Y, X) in D.GEO_CASES.items():
        op = rlr.ArrayToBlocks(b, [1, E, T, Y, X], True)
        out[f"geo_{tag}"] = np.array([op.pad_x[0], op.pad_x[1], op.pad_y[0], op.pad_y[1], op.nx_pad, op.ny_pad,
                                      op.num_blocks_x, op.num_blocks_y, op.num_blocks, op.block_stride])
        out[f"w_{tag}"] = op.weights[0, 0, 0].real.numpy().astype(np.float32)
        x, B = D.geo_inputs(tag)
        ext = op.extract(x[None].clone())
        assert tuple(ext.shape) == tuple(B.shape)
        D.put_sampled(out, f"ext_{tag}", ext.numpy())
        out[f"comb_{tag}"] = op.combine(B.clone())[0].numpy()
        print(f"case {tag}: {op.num_blocks_y} x {op.num_blocks_x} blocks, pads {op.pad_y} {op.pad_x}, "
              f"min weight {float(op.weights.real.min()):.4g}")
    # Decompose at case A
    b, E, T, Y, X = D.GEO_CASES["A"]
    dec = rlr.Decompose(b, D.DEC_RANK, [1, E, T, Y, X], True)
    img = D.lowrank_image()
    L, R = dec(img[None].clone())
    S = torch.svd(dec.block_op(img[None].clone()))[1]
    gap = float(((S[:, D.DEC_RANK - 1] - S[:, D.DEC_RANK]) / S[:, 0]).min())
    print(f"decompose: smallest relative gap (S_r - S_r+1) / S_1 = {gap:.3g}")
    assert gap >= 0.05
    out["dec_S"] = S[:, :D.DEC_RANK].numpy()
    out["dec_img"] = dec((L, R), adjoint=True)[0].numpy()


def _run(cls, cfg, T, rlr, data, dtype, v0):
    """One fwd + bwd of the reference network at dtype; v0: a list to record the power
    method's draws into (fp32 run) or to replay from (float64 run)."""
    cd = torch.complex64 if dtype == torch.float32 else torch.complex128
    model = cls(cfg)
    model.eval()
    D.fill(model, D.MODEL["seed"])
    model = model.to(dtype)
    maps, mask, y, target, L0, R0 = (t.to(cd) if t.is_complex() else t.to(dtype) for t in data)
    E, Tt, Y, X = target.shape[1:]
    op = rlr.ArrayToBlocks(D.MODEL["b"], [1, E, Tt, Y, X], True).to(dtype)
    acts, hooks = [], []
    for m in model.modules():
        if type(m).__name__ == "Activation" and isinstance(m.activ, torch.nn.ReLU):
            hooks.append(m.register_forward_pre_hook(lambda mod, inp: acts.append(inp[0].detach().clone())))
    rand, k = torch.rand, [0]

    def fake_rand(*a, **kw):
        if kw.get("dtype") != torch.complex64:
            return rand(*a, **kw)
        if dtype == torch.float32:
            v0.append(rand(*a, **kw))
            return v0[-1]
        k[0] += 1
        return v0[k[0] - 1].to(cd)
    torch.rand = fake_rand
    try:
        pred = model(y=y, A=T.SenseModel(maps, weights=mask), BlockOp=op, L0=L0.clone(), R0=R0.clone())
    finally:
        torch.rand = rand
        for h in hooks:
            h.remove()
    loss = torch.mean(torch.abs(target - pred))
    loss.backward()
    grads = {n: p.grad.detach().double() for n, p in model.named_parameters() if p.grad is not None}
    return pred.detach(), float(loss.detach()), grads, acts, sorted(model.state_dict().keys())


def gen_models(out, T, rlr, rd):
    cfg = _cfg()
    maps, mask, y, target = D.model_inputs()
    E, Tt, Y, X = target.shape[1:]
    init = T.SenseModel(maps, weights=mask)(y, adjoint=True)
    L0, R0 = rlr.Decompose(D.MODEL["b"], D.MODEL["r"], [1, E, Tt, Y, X], True)(init.clone())
    out["L0"], out["R0"] = L0.numpy(), R0.numpy()
    data = (maps, mask, y, target, L0, R0)
    classes = {"pgd": rd.AltMinPGD, "cg-v1": rd.AltMinCGv1, "cg-v2": rd.AltMinCGv2, "modl-v1": rd.AltMinMoDLv1,
               "modl-v2": rd.AltMinMoDLv2}
    for arch in D.ARCHS:
        v0 = []
        p32, l32, g32, a32, keys = _run(classes[arch], cfg, T, rlr, data, torch.float32, v0)
        p64, l64, g64, a64, _ = _run(classes[arch], cfg, T, rlr, data, torch.float64, v0)
        flips = sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(a32, a64))
        rel = min(float(a.abs().min() / a.pow(2).mean().sqrt()) for a in a64)
        names = sorted(g64)
        cat32 = np.concatenate([g32[n].numpy().reshape(-1) for n in names])
        cat64 = np.concatenate([g64[n].numpy().reshape(-1) for n in names])
        e_out = D.nrmse(p64.numpy(), p32.numpy())
        floor = D.nrmse(cat64, cat32)
        print(f"{arch}: loss {l64:.6g}; fp32 vs float64: output {e_out:.3g}, gradients {floor:.3g}; "
              f"{sum(a.numel() for a in a64)} ReLU inputs, {flips} flips, smallest |pre-activation| / rms {rel:.3g}")
        assert flips == 0, "a ReLU decision differs between the fp32 and the float64 run"
        assert floor < 2.5e-6 and e_out < 2.5e-6
        out[f"{arch}_pred"] = p64[0].numpy().astype(np.complex64)
        out[f"{arch}_loss"] = np.array(l64)
        out[f"{arch}_floor"] = np.array([e_out, floor])
        out[f"{arch}_state_keys"] = np.array(keys)
        out[f"{arch}_grad_names"] = np.array(names)
        out[f"{arch}_grad_norms"] = np.array([float(g64[n].norm()) for n in names])
        out[f"{arch}_grad_sample"] = cat64[D.sample_index(cat64.size)]
        if arch == "pgd":
            assert len(v0) == 2 * D.MODEL["unrolls"]
            out["pgd_v0"] = np.stack([v.numpy() for v in v0])         # [2 unrolls, N, r, 1]: (for R, for L) per unroll


def main():
    T = MG._import_ref()[0]
    import dl_cs.models.dslr as rd
    import dl_cs.mri.lowrank as rlr
    torch.manual_seed(0)
    out = {}
    gen_operators(out, rlr)
    gen_models(out, T, rlr, rd)
    MG._save("dslr", **out)
    size = os.path.getsize(os.path.join(HERE, "dslr.npz"))
    assert size <= os.path.getsize(os.path.join(HERE, "cbam.npz")), size


if __name__ == "__main__":
    main()
