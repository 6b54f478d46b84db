"""Comparison helpers for golden fixtures (full tensors or norm + fixed sample)."""
import numpy as np

NSAMPLE = 4096


def sample_index(numel):
    """Must match tests/golden/make_golden.py::sample_index."""
    rng = np.random.default_rng(numel)
    return np.sort(rng.choice(numel, size=min(NSAMPLE, numel), replace=False))


def _np(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu()
        if x.is_complex():
            x = x.to(__import__("torch").complex128)
        else:
            x = x.double()
        x = x.numpy()
    return np.asarray(x)


def nrmse(ref, x):
    ref = np.asarray(ref).astype(np.complex128).reshape(-1)
    x = np.asarray(x).astype(np.complex128).reshape(-1)
    den = np.linalg.norm(ref)
    return float(np.linalg.norm(x - ref) / (den if den > 0 else 1.0))


def golden_err(g, key, x):
    """NRMSE of tensor x against golden entry ``key`` (full or sampled form)."""
    a = _np(x)
    if key in g:
        assert a.shape == g[key].shape, (key, a.shape, g[key].shape)
        return nrmse(g[key], a)
    shape = tuple(g[key + "@shape"])
    assert a.shape == shape, (key, a.shape, shape)
    flat = a.reshape(-1)
    e_sample = nrmse(g[key + "@sample"], flat[sample_index(flat.size)])
    ref_norm = float(g[key + "@norm"])
    e_norm = abs(float(np.linalg.norm(flat.astype(np.complex128))) - ref_norm) / max(ref_norm, 1e-30)
    return max(e_sample, e_norm)


def has(g, key):
    return key in g or (key + "@sample") in g


def grad_keys(g, prefix):
    out = set()
    for k in g:
        if k.startswith(prefix + "grad::"):
            out.add(k[len(prefix + "grad::"):].split("@")[0])
    return sorted(out)


def oracle_grads(loss_fn, sd, dtype, trainable=None):
    """Parameter gradients of loss_fn(P, cast) evaluated by the CPU oracle at
    `dtype` (torch.float32 or torch.float64) on the weights of state dict `sd`;
    cast(t) converts an input tensor to the matching real / complex dtype."""
    import torch
    cd = torch.complex128 if dtype == torch.float64 else torch.complex64

    def cast(t):
        t = t.detach().cpu()
        return t.to(cd) if t.is_complex() else (t.to(dtype) if t.is_floating_point() else t)

    P = {}
    for k, v in sd.items():
        v = v.detach().cpu()
        if torch.is_floating_point(v):
            v = v.to(dtype).clone().requires_grad_(trainable is None or bool(trainable(k)))
        elif v.is_complex():                      # an input whose gradient is wanted too
            v = v.to(cd).clone().requires_grad_(trainable is None or bool(trainable(k)))
        P[k] = v
    loss_fn(P, cast).backward()
    return {k: v.grad.numpy() for k, v in P.items() if torch.is_tensor(v) and v.grad is not None}


def assert_f64_floor(hip, o32, o64, label, min_tol=1e-5, factor=4.0):
    """Per gradient tensor n (in all three dicts):
         NRMSE(hip[n] vs o64[n]) <= max(min_tol, factor * NRMSE(o32[n] vs o64[n])),
    i.e. the HIP build is held to the fp32 oracle's own distance from a float64
    evaluation (the floor set by ReLU masks / L1 signs that flip for values within
    fp32 rounding of 0), not to a fixed loose tolerance.  Prints the measured floors."""
    rows = []
    for n in sorted(set(hip) & set(o32) & set(o64)):
        h = hip[n].detach().cpu().numpy() if hasattr(hip[n], "detach") else np.asarray(hip[n])
        floor = nrmse(o64[n], o32[n])
        err = nrmse(o64[n], h)
        rows.append((err / max(min_tol, factor * floor), err, floor, n))
    assert rows, f"{label}: no gradients compared"
    rows.sort(reverse=True)
    r = rows[0]
    print(f"{label}: {len(rows)} grads vs f64; worst err/bound {r[0]:.3g} ({r[3]}: err {r[1]:.3g}, "
          f"oracle32 floor {r[2]:.3g}); largest floor {max(x[2] for x in rows):.3g}, "
          f"largest err {max(x[1] for x in rows):.3g}")
    bad = [x for x in rows if x[0] > 1.0]
    assert not bad, bad[:5]


# Gradient floor of the fp32 Swin path, whose 160 -> 160 convs (and K = 160 patch
# GEMMs) run on the f16x3 split -- 22-bit operands with one power-of-two scale per
# tensor (conv3d_f16x3.inc).  The matrix core's accumulate truncates toward -inf:
# about 0.1 ulp (of the tile's rms) per fresh six-product tile, the same sign for
# every output (tools/probe/mfma_chain.hip).  Coherent over a tensor, that bias
# survives the network's column sums (bias and norm gradients over 3e5 rows) where
# element errors average out: rounds 3-4 needed 5e-5 / 16x, then 2e-5 / 8x, here.
# The input-gradient convs now alternate the sign of their per-step tiles (the
# bias cancels; profiles/r04s_grad_accuracy.txt: column-sum error 2.1e-5 -> 5e-7), and every
# gradient is back inside the fp32 bound: worst 5.5e-6 at X = 160 (a norm weight,
# floor 1.3e-6; r04s).  Bound: max(1e-5, 4 x the fp32 oracle's own floor).
H3_GRAD_TOL = 1e-5
H3_FACTOR = 4.0


def captured_masks(cap):
    """The ReLU decisions one HIP network call took (dl_cs.models.engine.CAPTURE
    entry): post-ReLU activations in the patch-blocked layout (and, for the
    PatchGAN, its token-level one) -> boolean NCDHW masks in the oracle's ReLU
    call order."""
    import torch
    B, D, H, W = cap["grid"]
    out = []
    for t in cap["relu_inputs"]:
        C = t.shape[-1]
        m = (t.detach().float().cpu() > 0)
        m = m.reshape(B, D // 4, H // 4, W // 4, 4, 4, 4, C).permute(0, 1, 4, 2, 5, 3, 6, 7)
        out.append(m.reshape(B, D, H, W, C).permute(0, 4, 1, 2, 3).contiguous())
    for t in cap.get("tokens", []):
        C = t.shape[-1]
        m = (t.detach().float().cpu() > 0).reshape(B, D // 4, H // 4, W // 4, C)
        out.append(m.permute(0, 4, 1, 2, 3).contiguous())
    return out


class HipMasks:
    """Per-network-call mask lists captured from a HIP forward; relu() hands out
    a fresh oracle MaskedRelu for the next network call (in forward order), and
    stats() summarises how far the HIP decisions sit from the oracle's own."""

    def __init__(self, caps):
        self.calls = [captured_masks(c) for c in caps]
        self.k = 0
        self.relus = []

    def reset(self):
        self.k = 0

    def relu(self):
        from oracle.dlcs_oracle import MaskedRelu
        r = MaskedRelu(self.calls[self.k])
        self.k += 1
        self.relus.append(r)
        return r

    def stats(self):
        st = [s for r in self.relus for s in r.stats]
        return sum(n for n, _ in st), max([x for _, x in st] + [0.0])


def assert_masked_f64(hip, lf, sd, trainable, masks, label, min_tol=1e-5, factor=4.0):
    """assert_f64_floor with the oracle's ReLU decisions fixed to the HIP forward's
    (masks: HipMasks; lf(P, cast, masks) evaluates the loss).  The fp32 and float64
    oracles then differ from HIP only by arithmetic, so the per-tensor bound
    max(1e-5, 4 x oracle32 floor) holds at rounding level; the number of HIP
    decisions that differ from the float64 oracle's own, and the largest
    |pre-activation| / RMS among them, are printed (a wrong mask would sit far
    from 0)."""
    import torch

    def run(dt):
        masks.reset()
        return oracle_grads(lambda P, c: lf(P, c, masks), sd, dt, trainable)
    o32 = run(torch.float32)
    masks.relus = []
    o64 = run(torch.float64)
    n, rel = masks.stats()
    print(f"{label}: {n} HIP ReLU decisions differ from the float64 oracle's, largest |pre-act|/rms {rel:.3g}")
    assert rel < 1e-4, (label, n, rel)
    assert_f64_floor(hip, o32, o64, label + " (HIP masks)", min_tol, factor)


def attn_reference(qkv, table, labels, mask, nwin, N, heads, hd, window, scale, dout, round_q=True,
                   with_lse=False):
    """float64 window attention fwd + bwd on the (already rounded) operands:
    vst:139-170 with the relative-position bias of vst:111-129 and the -100 shift
    mask of vst:342-355 (from region labels) or an explicit additive mask.
    Returns (out, dqkv, dtable), with_lse: also the log-sum-exp [nwin, heads, N]."""
    import itertools
    import torch
    wd, wh, ww = window
    coords = torch.tensor(list(itertools.product(range(wd), range(wh), range(ww))))[:N]
    rel = coords[:, None, :] - coords[None, :, :]
    idx = (rel[..., 0] + wd - 1) * (2 * wh - 1) * (2 * ww - 1) + (rel[..., 1] + wh - 1) * (2 * ww - 1) + rel[..., 2] + ww - 1
    C = heads * hd
    x = qkv.double().view(nwin, N, 3, heads, hd).permute(2, 0, 3, 1, 4)        # [3, nw, h, N, hd]
    q = x[0] * scale
    if round_q:
        q = q.to(torch.bfloat16).double()                                       # the bf16 kernels round scale*q
    q = q.requires_grad_()
    k = x[1].clone().requires_grad_()
    v = x[2].clone().requires_grad_()
    tb = table.double().clone().requires_grad_()
    s = q @ k.transpose(-1, -2) + tb[idx.reshape(-1)].reshape(N, N, heads).permute(2, 0, 1)[None]
    if labels is not None:
        lab = labels.view(nwin, N)
        s = s + torch.where(lab[:, None, :, None] != lab[:, None, None, :], -100.0, 0.0).double()
    if mask is not None:
        s = s + mask.double()[torch.arange(nwin) % mask.shape[0]][:, None]
    o = torch.softmax(s, -1) @ v                                                # [nw, h, N, hd]
    o.backward(dout.double().view(nwin, N, heads, hd).permute(0, 2, 1, 3))
    out = o.permute(0, 2, 1, 3).reshape(nwin * N, C)
    dq = (q.grad * scale).permute(0, 2, 1, 3).reshape(nwin * N, C)
    dk = k.grad.permute(0, 2, 1, 3).reshape(nwin * N, C)
    dv = v.grad.permute(0, 2, 1, 3).reshape(nwin * N, C)
    res = (out.detach(), torch.cat([dq, dk, dv], 1).detach(), tb.grad.detach())
    return res + (torch.logsumexp(s, -1).detach(),) if with_lse else res


def attn_fwd_dtype(qkv, table, labels, mask, nwin, N, heads, hd, window, scale, dt, dout=None):
    """Window attention evaluated in dtype dt: out [rows, C], lse [nwin, heads, N] and,
    with dout, (dqkv [rows, 3C], dtable)."""
    import itertools
    import torch
    wd, wh, ww = window
    coords = torch.tensor(list(itertools.product(range(wd), range(wh), range(ww))))[:N]
    rel = coords[:, None, :] - coords[None, :, :]
    idx = (rel[..., 0] + wd - 1) * (2 * wh - 1) * (2 * ww - 1) + (rel[..., 1] + wh - 1) * (2 * ww - 1) + rel[..., 2] + ww - 1
    xq = qkv.to(dt).clone().requires_grad_()
    tb = table.to(dt).clone().requires_grad_()
    x = xq.view(nwin, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    s = (x[0] * scale) @ x[1].transpose(-1, -2) + tb[idx.reshape(-1)].reshape(N, N, heads).permute(2, 0, 1)[None]
    if labels is not None:
        lab = labels.view(nwin, N)
        s = s + torch.where(lab[:, None, :, None] != lab[:, None, None, :], -100.0, 0.0).to(dt)
    if mask is not None:
        s = s + mask.to(dt)[torch.arange(nwin) % mask.shape[0]][:, None]
    o = (torch.softmax(s, -1) @ x[2]).permute(0, 2, 1, 3).reshape(nwin * N, heads * hd)
    lse = torch.logsumexp(s, -1)
    if dout is None:
        return o.detach(), lse.detach()
    o.backward(dout.to(dt))
    return o.detach(), lse.detach(), xq.grad, tb.grad
