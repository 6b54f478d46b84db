"""CPU restatement of the DSLR family in plain PyTorch, at the dtype of its inputs
(complex64 / complex128), written from the operators' equations:

  blocks    an image [E, T, Y, X] is zero-padded to [b (Y // b + 1), b (X // b + 1)]
            (left pad = half the difference rounded down), cut into b x b blocks at
            stride b / 2, n = by nbx + bx, row p = e b^2 + iy b + ix, and every element
            is multiplied by w[iy] w[ix], w = sqrt of the periodic Hann window
  combine   the windowed blocks are added back at their places, the pad is cropped and
            the image divided by weights + 1e-8, weights = combine_0(extract(1))
  nets      2-D ResNet on L (zero padding), 1-D ResNet on R (circular time pad); both
            with the in-place-ReLU algebra r0 = relu(conv0 u), t = relu(conv_a r),
            r' = relu(conv_b t + r), out = conv_f r_L + u
  AltMin    the five unrolled alternating-minimisation networks over (L, R)

Everything is a function of a state dict P; `relu` may be replaced (MaskedRelu) and
`acts` (a list) collects every conv pre-activation that a ReLU reads.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dlcs_oracle as O
from oracle import recipe

EPS = 1e-8


# ------------------------------------------------------------------ geometry and block operators
class Geo:
    def __init__(self, b, E, T, Y, X, dtype=torch.float64):
        self.b, self.s, self.E, self.T, self.Y, self.X = b, b // 2, E, T, Y, X
        self.py = self._pad(Y)
        self.px = self._pad(X)
        self.Yp, self.Xp = Y + sum(self.py), X + sum(self.px)
        self.nby = (self.Yp - b) // self.s + 1
        self.nbx = (self.Xp - b) // self.s + 1
        self.N = self.nby * self.nbx
        # periodic Hann: 0.5 (1 - cos(2 pi n / b)); the fp32 window of the operator under test
        # is torch.hann_window(b) ** 0.5, whose rounding is part of what the tolerance covers
        n = torch.arange(b, dtype=torch.float64)
        self.w1 = torch.sqrt(0.5 * (1.0 - torch.cos(2.0 * math.pi * n / b))).to(dtype)
        self.w2 = (self.w1[:, None] * self.w1[None, :])
        ones = torch.ones((E, T, Y, X), dtype=torch.complex128 if dtype == torch.float64 else torch.complex64)
        self.weights = combine(self, extract(self, ones), divide=False).real[0, 0].clone()

    def _pad(self, n):
        left = (self.b * (n // self.b + 1) - n) // 2
        return (left, left if n % 2 == 0 else left + 1)


def extract(g, image, divide=False):
    """[E, T, Y, X] -> [N, E b^2, T]."""
    if divide:
        image = image / (g.weights + EPS)
    x = F.pad(image, g.px + g.py)
    out = []
    for by in range(g.nby):
        for bx in range(g.nbx):
            blk = x[:, :, by * g.s:by * g.s + g.b, bx * g.s:bx * g.s + g.b] * g.w2      # [E, T, b, b]
            out.append(blk.permute(0, 2, 3, 1).reshape(g.E * g.b * g.b, g.T))
    return torch.stack(out)


def combine(g, blocks, divide=True):
    """[N, E b^2, T] -> [E, T, Y, X]."""
    out = blocks.new_zeros((g.E, g.T, g.Yp, g.Xp))
    for by in range(g.nby):
        for bx in range(g.nbx):
            blk = blocks[by * g.nbx + bx].reshape(g.E, g.b, g.b, g.T).permute(0, 3, 1, 2) * g.w2
            out[:, :, by * g.s:by * g.s + g.b, bx * g.s:bx * g.s + g.b] += blk
    out = out[:, :, g.py[0]:g.py[0] + g.Y, g.px[0]:g.px[0] + g.X]
    return out / (g.weights + EPS) if divide else out


def bt(m):
    return m.conj().transpose(1, 2)


def compose(g, L, R, divide=True):
    return combine(g, torch.bmm(L, bt(R)), divide)


def project_l(g, image, R, divide=False):
    return torch.bmm(extract(g, image, divide), R)


def project_r(g, image, L, divide=False):
    return torch.bmm(bt(extract(g, image, divide)), L)


def decompose(g, image, rank):
    U, S, Vh = torch.linalg.svd(extract(g, image), full_matrices=False)
    sq = S[:, None, :rank].sqrt()
    return U[:, :, :rank] * sq, bt(Vh)[:, :, :rank] * sq, S


def power_method(A, v0, num_iter=10, eps=1e-6):
    """The largest eigenvalue of A^H A for each A [n, m, k]: the norm of (A^H A) v after
    num_iter normalised steps from v0 [n, k, 1]."""
    AhA = torch.bmm(bt(A), A)
    v = v0
    for _ in range(num_iter):
        v = torch.bmm(AhA, v)
        ev = (v.abs() ** 2).sum(1).sqrt()
        v = v / (ev.reshape(-1, 1, 1) + eps)
    return ev.reshape(-1)


# ------------------------------------------------------------------ the two CNNs
def _trunk(P, pre, u, conv, nblocks, relu, acts):
    def c(h, name):
        return conv(h, P[f"{pre}{name}.layers.2.conv.weight"], P[f"{pre}{name}.layers.2.conv.bias"])

    def act(z):
        if acts is not None:
            acts.append(z.detach())
        return relu(z)
    r = act(c(u, "init_layer"))
    for k in range(nblocks):
        t = act(c(r, f"res_blocks.{k}.layers.0"))
        r = act(c(t, f"res_blocks.{k}.layers.1") + r)
    return c(r, "final_layer") + u


def resnet2d(P, pre, x, nblocks, relu=F.relu, acts=None):
    """x complex [N, C, b, b] -> the same shape; zero padding."""
    C = x.shape[1]
    u = torch.cat((x.real, x.imag), dim=1)
    o = _trunk(P, pre, u, lambda h, w, b: F.conv2d(h, w, b, padding=1), nblocks, relu, acts)
    return torch.complex(o[:, :C].contiguous(), o[:, C:].contiguous())


def resnet1d(P, pre, x, nblocks, relu=F.relu, acts=None):
    """x complex [N, C, T] -> the same shape; circular time pad of 2 nblocks + 2."""
    C, pad = x.shape[1], 2 * nblocks + 2
    u = F.pad(torch.cat((x.real, x.imag), dim=1), (pad, pad), mode="circular")
    o = _trunk(P, pre, u, lambda h, w, b: F.conv1d(h, w, b, padding=1), nblocks, relu, acts)
    o = o[:, :, pad:o.shape[2] - pad]
    return torch.complex(o[:, :C].contiguous(), o[:, C:].contiguous())


# ------------------------------------------------------------------ SENSE and CG
def sense_normal(x, maps, mask):
    """A^H A x: x [E, T, Y, X], maps [1, E, C, 1, Y, X], mask [1, 1, T, Y, X] (in A and in A^H)."""
    return O.sense_adjoint(O.sense_forward(x[None], maps, mask), maps, mask)[0]


def sense_adjoint(y, maps, mask):
    """y [1, C, T, Y, X] -> [E, T, Y, X]."""
    return O.sense_adjoint(y, maps, mask)[0]


def cg(normal, x, rhs, num_iter):
    r = rhs - normal(x)
    rs = (r.conj() * r).sum().real
    p = r
    for _ in range(num_iter):
        Ap = normal(p)
        alpha = rs / (p.conj() * Ap).sum()
        x = x + alpha * p
        r = r - alpha * Ap
        rs_new = (r.conj() * r).sum().real
        p = (rs_new / rs) * p + r
        rs = rs_new
    return x


# ------------------------------------------------------------------ the unrolled networks
ARCHS = ("pgd", "cg-v1", "cg-v2", "modl-v1", "modl-v2")


def altmin(arch, P, g, y, maps, mask, L0, R0, *, num_unrolls, nblocks, num_cg=3, share=False, v0=None,
           relu=F.relu, acts=None):
    """The five networks; returns the image [E, T, Y, X].  v0: PGD's power-method start
    vectors, [(for R, for L)] per unroll."""
    r, E, b = L0.shape[2], g.E, g.b
    N = L0.shape[0]

    def cnn_l(L, i):
        k = 0 if share else i
        z = resnet2d(P, f"spatial_cnn_update.{k}.", L.transpose(1, 2).reshape(N, r * E, b, b), nblocks, relu, acts)
        return z.reshape(N, r, E * b * b).transpose(1, 2)

    def cnn_r(R, i):
        k = 0 if share else i
        return resnet1d(P, f"temporal_cnn_update.{k}.", R.transpose(1, 2), nblocks, relu, acts).transpose(1, 2)

    def aha_blocks(L, R):
        return extract(g, sense_normal(compose(g, L, R), maps, mask))

    aty_img = sense_adjoint(y, maps, mask)
    aty = extract(g, aty_img)
    L, R = L0, R0
    if arch == "pgd":
        for i in range(num_unrolls):
            gx = extract(g, sense_normal(compose(g, L, R), maps, mask) - aty_img)
            gl, gr = torch.bmm(gx, R), torch.bmm(bt(gx), L)
            sl = -0.9 / power_method(R, v0[i][0].to(R.dtype)).max()
            sr = -0.9 / power_method(L, v0[i][1].to(L.dtype)).max()
            L, R = L + sl * gl, R + sr * gr
            L, R = cnn_l(L, i), cnn_r(R, i)
        return compose(g, L, R)

    def lam(name):
        if arch == "modl-v1":
            return P[name]
        return 1e2 * torch.clamp(P[name], min=0.0)

    def dc_l(L, R, zl=None):
        l = 0.0 if zl is None else lam("lambda_l")
        normal = lambda q: l * q + torch.bmm(aha_blocks(q, R), R)
        rhs = torch.bmm(aty, R) + (0.0 if zl is None else l * zl)
        return cg(normal, L, rhs, num_cg)

    def dc_r(R, L, zr=None):
        l = 0.0 if zr is None else lam("lambda_r")
        normal = lambda q: l * q + torch.bmm(bt(aha_blocks(L, q)), L)
        rhs = torch.bmm(bt(aty), L) + (0.0 if zr is None else l * zr)
        return cg(normal, R, rhs, num_cg)

    if arch in ("cg-v1", "cg-v2"):
        for i in range(num_unrolls):
            if arch == "cg-v1":
                L = dc_l(L, R)
                R = dc_r(R, L)
                L, R = cnn_l(L, i), cnn_r(R, i)
            else:
                L = cnn_l(dc_l(L, R), i)
                R = cnn_r(dc_r(R, L), i)
        return compose(g, L, R)
    if arch == "modl-v1":
        for i in range(num_unrolls):
            L = dc_l(L, R, cnn_l(L, i))
            R = dc_r(R, L, cnn_r(R, i))
        return compose(g, L, R)
    assert arch == "modl-v2"
    zl, zr = torch.zeros_like(L0), torch.zeros_like(R0)
    for i in range(num_unrolls):
        L = dc_l(L, R if i == 0 else zr, zl)
        zl = cnn_l(L, i)
        R = dc_r(R, zl, zr)
        zr = cnn_r(R, i)
    return compose(g, zl, zr)


# ------------------------------------------------------------------ fixture recipe (generator and tests)
# operator cases: b, E, T, Y, X.  A: 7 x 11 blocks; B: odd sizes, pads (1, 2), edge weights
# down to 0.25; C: a zero left pad, so the first row's weight is exactly 0
GEO_CASES = {"A": (4, 2, 5, 12, 20), "B": (4, 2, 5, 9, 13), "C": (4, 1, 3, 11, 14)}
# Decompose's rank: with b = 4 the last corner block holds one pixel (the window's first tap is 0
# and the right pad takes the rest), so its matrix has rank E = 2 and only r <= 2 leaves a gap there
DEC_RANK = 2
# the model case (case A's geometry with T = 8: the 1-D net's time axis is 8 + 2 * 4 = 16)
MODEL = dict(E=2, C=4, T=8, Y=12, X=20, b=4, r=3, features=8, resblocks=1, unrolls=2, cg=3, seed=91)
NSAMPLE = 1024
LAMBDA_INIT = {"modl-v1": (1.0, 2.0), "modl-v2": (5e-3, 5e-3)}


def nrmse(ref, x):
    ref = np.asarray(ref).astype(np.complex128).reshape(-1)
    x = np.asarray(x).astype(np.complex128).reshape(-1)
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300))


def sample_index(numel):
    rng = np.random.default_rng(numel)
    return np.sort(rng.choice(numel, size=min(NSAMPLE, numel), replace=False))


def put_sampled(out, key, a):
    """Store the norm and a fixed sample of a (whole when it has at most 2 NSAMPLE elements)."""
    flat = np.asarray(a).reshape(-1)
    if flat.size <= 2 * NSAMPLE:
        out[key] = np.asarray(a)
    else:
        out[key + "@norm"] = np.array(float(np.linalg.norm(flat.astype(np.complex128))))
        out[key + "@sample"] = flat[sample_index(flat.size)]


def sampled_err(g, key, a):
    """NRMSE of a against what put_sampled stored under key."""
    a = np.asarray(a)
    if key in g:
        assert a.shape == g[key].shape
        return nrmse(g[key], a)
    flat = a.reshape(-1)
    e_norm = abs(float(np.linalg.norm(flat.astype(np.complex128))) - float(g[key + "@norm"])) / float(g[key + "@norm"])
    return max(nrmse(g[key + "@sample"], flat[sample_index(flat.size)]), e_norm)


def geo_inputs(tag):
    """(image [E, T, Y, X], blocks [N, E b^2, T]) of an operator case."""
    b, E, T, Y, X = GEO_CASES[tag]
    k = 40 * list(GEO_CASES).index(tag)
    N = (2 * (Y // b + 1) - 1) * (2 * (X // b + 1) - 1)
    return recipe.crandn(800 + k, (E, T, Y, X)), recipe.crandn(801 + k, (N, E * b * b, T))


def lowrank_image():
    """Case A's image for Decompose: rank DEC_RANK over (space, time) plus 1 % noise, so every
    block matrix has DEC_RANK dominant singular values and a clear gap after them."""
    b, E, T, Y, X = GEO_CASES["A"]
    u = recipe.crandn(850, (DEC_RANK, E, 1, Y, X)).to(torch.complex128)
    v = recipe.crandn(851, (DEC_RANK, 1, T, 1, 1)).to(torch.complex128)
    s = torch.tensor([1.0, 0.6], dtype=torch.float64).reshape(DEC_RANK, 1, 1, 1, 1)
    return ((s * u * v).sum(0) + 0.01 * recipe.crandn(852, (E, T, Y, X))).to(torch.complex64)


def model_inputs():
    """maps [1, E, C, 1, Y, X], mask [1, 1, T, Y, X], y [1, C, T, Y, X], target [1, E, T, Y, X]."""
    m = MODEL
    maps = recipe.sense_maps(92, 1, m["E"], m["C"], m["Y"], m["X"])
    mask = recipe.binary_mask(93, (1, 1, m["T"], m["Y"], m["X"]))
    y = recipe.crandn(94, (1, m["C"], m["T"], m["Y"], m["X"])) * mask
    target = recipe.crandn(95, (1, m["E"], m["T"], m["Y"], m["X"]))
    return maps, mask, y, target


def fill(model, seed):
    """recipe.fill_module, with the MoDL penalties lambda_l / lambda_r put back to their
    initial values (the recipe would treat them as biases: 0.05 U(-1, 1), which the clamp
    of the v2 network turns into 0 half of the time)."""
    keep = {n: p.detach().clone() for n, p in model.named_parameters() if n in ("lambda_l", "lambda_r")}
    recipe.fill_module(model, seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n in keep:
                p.copy_(keep[n])
    return model


def param_shapes(arch):
    """{state_dict key: shape} of a network at the MODEL case (weights and biases of the
    2-D and 1-D nets of every unroll, the MoDL penalties)."""
    m = MODEL
    F, c2, c1 = m["features"], 2 * m["r"] * m["E"], 2 * m["r"]
    out = {}
    for i in range(m["unrolls"]):
        for top, cin, k in ((f"spatial_cnn_update.{i}.", c2, (3, 3)), (f"temporal_cnn_update.{i}.", c1, (3,))):
            layers = [("init_layer", cin, F)] + \
                [(f"res_blocks.{j}.layers.{h}", F, F) for j in range(m["resblocks"]) for h in (0, 1)] + \
                [("final_layer", F, cin)]
            for name, ci, co in layers:
                out[f"{top}{name}.layers.2.conv.weight"] = (co, ci) + k
                out[f"{top}{name}.layers.2.conv.bias"] = (co,)
    if arch in LAMBDA_INIT:
        out["lambda_l"] = out["lambda_r"] = (1,)
    return out


def oracle_params(arch, dtype=torch.float64, seed=None, share=False):
    """The recipe's parameters of a network as leaf tensors at dtype.  share: every unroll is
    one network, which recipe.fill_module fills under its last alias (the sorted-key rule of
    oracle/recipe.py), so all of them take the last unroll's values."""
    P = {}
    last = f"_cnn_update.{MODEL['unrolls'] - 1}."
    for k, shape in param_shapes(arch).items():
        if k.startswith("lambda_"):
            v = torch.tensor([LAMBDA_INIT[arch][0 if k == "lambda_l" else 1]], dtype=torch.float32)
        else:
            name = k.replace("_cnn_update." + k.split("_cnn_update.")[1].split(".")[0] + ".", last) if share else k
            v = recipe.param_value(MODEL["seed"] if seed is None else seed, name, shape)
        P[k] = v.to(dtype).clone().requires_grad_()
    return P


def oracle_run(g, arch, dtype=torch.float64, share=False):
    """(pred, loss, grads by name) of the oracle network at dtype on the fixture inputs
    (g: the dslr golden, for L0, R0 and PGD's start vectors), complex-L1 loss."""
    cd = torch.complex128 if dtype == torch.float64 else torch.complex64
    m = MODEL
    maps, mask, y, target = model_inputs()
    geo = Geo(m["b"], m["E"], m["T"], m["Y"], m["X"], dtype)
    P = oracle_params(arch, dtype, share=share)
    v0 = None
    if arch == "pgd":
        v = torch.from_numpy(g["pgd_v0"])
        v0 = [(v[2 * i], v[2 * i + 1]) for i in range(m["unrolls"])]
    pred = altmin(arch, P, geo, y.to(cd), maps.to(cd), mask.to(dtype), torch.from_numpy(g["L0"]).to(cd),
                  torch.from_numpy(g["R0"]).to(cd), num_unrolls=m["unrolls"], nblocks=m["resblocks"], num_cg=m["cg"],
                  v0=v0, share=share)
    loss = torch.mean(torch.abs(target[0].to(cd) - pred))
    loss.backward()
    return pred.detach(), float(loss.detach()), {k: p.grad for k, p in P.items() if p.grad is not None}
