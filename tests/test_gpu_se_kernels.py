"""Direct unit checks of the squeeze-excitation kernels (csrc/se.hip) in the style of
test_gpu_glue_kernels.py: every reference is float64 (or exact) on the CPU, every
output sits between sentinel margins, the pad columns [C, ld) of the row operands hold
1e30 on input (a read of them shows) and keep their sentinel on output.

Tolerances come from what each kernel does:
  * reductions (se_pool, se_bwd_reduce): NRMSE < 1e-6 against float64, the bar
    _colsum_check sets for fp32 column sums; two calls must agree bit for bit;
  * element-wise passes: one multiply and one add per element, each rounded once in
    fp32 (2^-24 relative each, or one rounding when fused): per element
    |got - ref64| <= 2^-22 (|o s| + |res|), which allows two roundings with margin 2;
  * the gate and its backward: max(1e-6, 4 x the distance of the same formulas in
    torch fp32 on the CPU from float64 on the same inputs).

  entry point               test
  ------------------------  -----------------------------------------------------
  dlcs_se_pool              test_se_pool, test_se_refusals
  dlcs_se_bwd_reduce        test_se_bwd_reduce, test_se_refusals
  dlcs_se_scale_res_relu    test_se_scale_res_relu, test_se_refusals
  dlcs_se_bwd_apply         test_se_bwd_apply, test_se_refusals
  dlcs_se_gate              test_se_gate, test_se_refusals
  dlcs_se_gate_bwd          test_se_gate_bwd, test_se_refusals
"""
import math

import pytest
import torch

from goldutil import nrmse
from oracle import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
GUARD = 64
SENT = -12345.0
PADV = 1e30
ERR_UNSUPPORTED, ERR_WORKSPACE = 100002, 100003

# (B, N, C, ld, misaligned): one patch / one row group; vector path with C % 8 != 0; many
# partial blocks per batch item; three items at 384 channels (2 row groups, idle lanes);
# the scalar path (C % 4 != 0); the scalar path by a 4-byte-misaligned view
SHAPES = [(1, 64, 64, 64, False), (2, 768, 40, 40, False), (2, 12288, 64, 64, False), (3, 320, 384, 384, False),
          (2, 192, 7, 8, False), (2, 768, 64, 64, True)]
_shape_params = pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:4])) + ("-mis" if s[4] else ""))
# (B, C, R)
GATE_SHAPES = [(1, 64, 16), (2, 40, 1), (3, 384, 16), (2, 1024, 256)]
_gate_params = pytest.mark.parametrize("shape", GATE_SHAPES, ids=lambda s: "x".join(map(str, s)))


def _K():
    from dl_cs.models import _ops as K
    return K


def _lib():
    from dl_cs import _lib
    return _lib.lib()


def _rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _bits(t):
    return t.view(torch.int32)


class _Buf:
    """A device tensor of `shape` between two sentinel margins, 16-B aligned or (mis) 4
    bytes past that.  init: a CPU tensor, a fill value, or None (the sentinel); get()
    checks both margins and returns the CPU copy."""

    def __init__(self, shape, init=None, mis=False):
        shape = tuple(int(s) for s in shape)
        n = math.prod(shape)
        lead = GUARD + (1 if mis else 0)
        self.buf = torch.full((lead + n + GUARD,), SENT, dtype=F32, device=DEV)
        self.lead = lead
        self.t = self.buf[lead:lead + n].view(shape)
        assert self.t.data_ptr() % 16 == (4 if mis else 0)
        if torch.is_tensor(init):
            self.t.copy_(init.reshape(shape))
        elif init is not None:
            self.t.fill_(init)

    def get(self):
        b = self.buf.cpu()
        n = self.t.numel()
        assert torch.equal(b[:self.lead], torch.full((self.lead,), SENT)), "write before the buffer"
        assert torch.equal(b[self.lead + n:], torch.full((GUARD,), SENT)), "write past the buffer"
        return b[self.lead:self.lead + n].view(self.t.shape).clone()


def _rows(B, N, C, ld, seed, offsets=True):
    """[B N, ld] operand: randn, batch item b shifted by 1 + 2 b (a segment boundary that
    is off by one row then moves a sum by O(1) of its O(N) value), pad columns 1e30."""
    x = _rnd((B * N, ld), seed)
    if offsets:
        x += (1.0 + 2.0 * torch.arange(B, dtype=F32)).repeat_interleave(N)[:, None]
    x[:, C:] = PADV
    return x


def _relu_rows(B, N, C, ld, seed, shift=0):
    """test_gpu_glue_kernels._relu_operand's recipe on [B N, ld]: exact 0.0, -0.0, NaN and
    negatives at fixed positions (k = 1, 2, 3, 4 of every 6), pad columns 1e30."""
    n = B * N * ld
    a = _rnd((n,), seed).abs() + 0.125
    k = (torch.arange(n) + shift) % 6
    a[k == 1] = 0.0
    a[k == 2] = -0.0
    a[k == 3] = float("nan")
    a[k == 4] *= -1.0
    a = a.view(B * N, ld)
    a[:, C:] = PADV
    return a


def _gates(B, C, seed):
    return torch.sigmoid(2.0 * _rnd((B, C), seed))


def _per_row(v, N):
    """[B, C] -> [B N, C]"""
    return v.repeat_interleave(N, dim=0)


# ============================================================================ reductions
@_shape_params
def test_se_pool(shape):
    K = _K()
    B, N, C, ld, mis = shape
    x = _rows(B, N, C, ld, 10)
    xd = _Buf((B * N, ld), init=x, mis=mis)
    outs = []
    for _ in range(2):
        mean = _Buf((B, C))
        K.se_pool(xd.t, B, N, C, mean=mean.t)
        outs.append(mean.get())
    ref = x[:, :C].double().view(B, N, C).mean(1)
    e = nrmse(ref.numpy(), outs[0].double().numpy())
    print(f"se_pool {shape}: NRMSE vs float64 {e:.3g}")
    assert e < 1e-6
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two calls on the same input differ"
    assert torch.equal(xd.get(), x)


@_shape_params
def test_se_bwd_reduce(shape):
    K = _K()
    B, N, C, ld, mis = shape
    o = _rows(B, N, C, ld, 20)
    g = _rows(B, N, C, ld, 21, offsets=False) + 0.5
    g[:, C:] = PADV
    rn = _relu_rows(B, N, C, ld, 22, shift=B + C)
    keep = rn > 0                                            # NaN, 0.0, -0.0 and negatives: dropped
    g[:, :C] = torch.where(keep[:, :C], g[:, :C], torch.full_like(g[:, :C], 1e18))   # a dropped row that leaks shows
    od, gd, rd = (_Buf((B * N, ld), init=t, mis=mis) for t in (o, g, rn))
    outs = []
    for _ in range(2):
        dg = _Buf((B, C))
        K.se_bwd_reduce(gd.t, rd.t, od.t, B, N, C, dgate=dg.t)
        outs.append(dg.get())
    term = torch.where(keep[:, :C], g[:, :C].double() * o[:, :C].double(), torch.zeros((), dtype=torch.float64))
    ref = term.view(B, N, C).sum(1)
    assert torch.isfinite(outs[0]).all(), "a NaN of r_next (or a dropped row) reached the sum"
    e = nrmse(ref.numpy(), outs[0].double().numpy())
    print(f"se_bwd_reduce {shape}: NRMSE vs float64 {e:.3g}")
    assert e < 1e-6
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two calls on the same input differ"


# ============================================================================ element-wise passes
@_shape_params
def test_se_scale_res_relu(shape):
    K = _K()
    B, N, C, ld, mis = shape
    o = _rows(B, N, C, ld, 30, offsets=False)
    res = _rows(B, N, C, ld, 31, offsets=False)
    s = _gates(B, C, 32) * (1.0 + torch.arange(B, dtype=F32))[:, None] / B      # items differ: a mixed-up b shows
    od, rd, sd = _Buf((B * N, ld), init=o, mis=mis), _Buf((B * N, ld), init=res, mis=mis), s.to(DEV)
    out = _Buf((B * N, ld), mis=mis)
    K.se_scale_res_relu(od.t, sd, rd.t, B, N, C, out=out.t)
    got = out.get()
    assert torch.equal(got[:, C:], torch.full((B * N, ld - C), SENT)), "pad columns written"
    prod = o[:, :C].double() * _per_row(s, N).double()
    pre = prod + res[:, :C].double()
    ref = pre.clamp_min(0.0)
    bound = 2.0 ** -22 * (prod.abs() + res[:, :C].double().abs())
    err = (got[:, :C].double() - ref).abs()
    print(f"se_scale_res_relu {shape}: worst err/bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())
    dropped = pre < -bound
    assert int(dropped.sum()) > 0
    assert torch.equal(_bits(got[:, :C][dropped]), torch.zeros(int(dropped.sum()), dtype=torch.int32)), "dropped: not +0"
    assert not bool(((got[:, :C] == 0) & (_bits(got[:, :C]) != 0)).any()), "-0 written"
    # out aliasing res: the same bits, o untouched
    K.se_scale_res_relu(od.t, sd, rd.t, B, N, C, out=rd.t)
    alias = rd.get()
    assert torch.equal(_bits(alias[:, :C]), _bits(got[:, :C]))
    assert torch.equal(alias[:, C:], res[:, C:])
    assert torch.equal(od.get(), o)


@_shape_params
def test_se_bwd_apply(shape):
    K = _K()
    B, N, C, ld, mis = shape
    g0 = _rows(B, N, C, ld, 40, offsets=False)
    rn = _relu_rows(B, N, C, ld, 41, shift=C)
    s = _gates(B, C, 42) * (1.0 + torch.arange(B, dtype=F32))[:, None] / B
    dm = _rnd((B, C), 43) * (1.0 + torch.arange(B, dtype=F32))[:, None]
    gd, rd = _Buf((B * N, ld), init=g0, mis=mis), _Buf((B * N, ld), init=rn, mis=mis)
    dout = _Buf((B * N, ld), mis=mis)
    K.se_bwd_apply(gd.t, rd.t, s.to(DEV), dm.to(DEV), B, N, C, dout=dout.t)
    g1, d = gd.get(), dout.get()
    keep = rn[:, :C] > 0
    gz = torch.where(keep, g0[:, :C], torch.zeros_like(g0[:, :C]))
    assert torch.equal(_bits(g1[:, :C]), _bits(gz)), "g is not relu_grad's result"
    gr = g0[:, :C].contiguous().to(DEV)                                         # and bitwise dlcs_relu_grad itself
    K.relu_grad(gr, rn[:, :C].contiguous().to(DEV))
    assert torch.equal(_bits(g1[:, :C]), _bits(gr.cpu()))
    assert torch.equal(g1[:, C:], g0[:, C:]), "pad columns of g written"
    assert torch.equal(d[:, C:], torch.full((B * N, ld - C), SENT)), "pad columns of dout written"
    prod = gz.double() * _per_row(s, N).double()
    dmr = _per_row(dm, N).double()
    bound = 2.0 ** -22 * (prod.abs() + dmr.abs())
    err = (d[:, :C].double() - (prod + dmr)).abs()
    print(f"se_bwd_apply {shape}: worst err/bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())
    assert torch.equal(_bits(d[:, :C][~keep]), _bits(_per_row(dm, N)[~keep])), "a dropped position is not 0 s + dmean"
    assert torch.equal(_bits(rd.get()), _bits(rn))


# ============================================================================ gate
def _gate_params_values(B, C, R, seed):
    """FC weights at the recipe's scale times 8 (the fixtures' spread), recipe biases."""
    w1 = 8.0 * recipe.param_value(seed, "layers.1.fc.weight", (R, C))
    b1 = recipe.param_value(seed, "layers.1.fc.bias", (R,))
    w2 = 8.0 * recipe.param_value(seed, "layers.3.fc.weight", (C, R))
    b2 = recipe.param_value(seed, "layers.3.fc.bias", (C,))
    mean = _rnd((B, C), seed + 1) * (1.0 + torch.arange(B, dtype=F32))[:, None]
    return w1, b1, w2, b2, mean


def _gate_ref(mean, w1, b1, w2, b2, dt):
    m, w1, b1, w2, b2 = (t.to(dt) for t in (mean, w1, b1, w2, b2))
    h = torch.relu(m @ w1.T + b1)
    return h, torch.sigmoid(h @ w2.T + b2)


def _floor_check(label, got, o32, o64, den=None):
    """NRMSE(got vs float64) <= max(1e-6, 4 x NRMSE(torch fp32 CPU vs float64)); den: the norm
    to relate both to (default: the float64 value's)."""
    den = float(o64.norm()) if den is None else den
    den = den if den > 0 else 1.0
    floor = float((o32.double() - o64).norm()) / den
    err = float((got.double() - o64).norm()) / den
    print(f"{label}: err {err:.3g}, fp32 CPU floor {floor:.3g}, bound {max(1e-6, 4 * floor):.3g}")
    assert err <= max(1e-6, 4.0 * floor), label


@_gate_params
def test_se_gate(shape):
    K = _K()
    B, C, R = shape
    w1, b1, w2, b2, mean = _gate_params_values(B, C, R, 50)
    hid, gate = _Buf((B, R)), _Buf((B, C))
    K.se_gate(mean.to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), hidden=hid.t, gate=gate.t)
    h32, s32 = _gate_ref(mean, w1, b1, w2, b2, F32)
    h64, s64 = _gate_ref(mean, w1, b1, w2, b2, torch.float64)
    h, s = hid.get(), gate.get()
    print(f"se_gate {shape}: gates {float(s64.min()):.3g} .. {float(s64.max()):.3g}, {int((h64 == 0).sum())} of "
          f"{h64.numel()} hidden units off")
    _floor_check(f"se_gate {shape} hidden", h, h32, h64)
    _floor_check(f"se_gate {shape} gate", s, s32, s64)
    assert bool((h >= 0).all()) and not bool(((h == 0) & (_bits(h) != 0)).any())
    # a hidden unit the float64 evaluation switches off by more than rounding is exactly off
    z64 = mean.double() @ w1.double().T + b1.double()
    assert bool((h[z64 < -1e-5 * float(z64.abs().max())] == 0).all())


def _gate_bwd_ref(dgate, gate, hidden, mean, w1, w2, inv_n, dt):
    dgate, s, h, m, w1, w2 = (t.to(dt) for t in (dgate, gate, hidden, mean, w1, w2))
    dz2 = dgate * s * (1 - s)
    dh = (dz2 @ w2) * (h > 0).to(dt)
    return dict(dw1=dh.T @ m, db1=dh.sum(0), dw2=dz2.T @ h, db2=dz2.sum(0), dmean=(dh @ w1) * inv_n)


@_gate_params
def test_se_gate_bwd(shape):
    K = _K()
    B, C, R = shape
    w1, b1, w2, b2, mean = _gate_params_values(B, C, R, 60)
    hidden, gate = _gate_ref(mean, w1, b1, w2, b2, F32)                     # the kernel's inputs, fp32
    if R > 1:
        hidden[:, 0] = 0.0                                                  # one unit off in every item
    dgate = _rnd((B, C), 62) * 3.0
    inv_n = 1.0 / 20480
    init = dict(dw1=_rnd((R, C), 63), db1=_rnd((R,), 64), dw2=_rnd((C, R), 65), db2=_rnd((C,), 66))
    bufs = {k: _Buf(v.shape, init=v) for k, v in init.items()}
    dmean = _Buf((B, C))
    K.se_gate_bwd(dgate.to(DEV), gate.to(DEV), hidden.to(DEV), mean.to(DEV), w1.to(DEV), w2.to(DEV), inv_n,
                  bufs["dw1"].t, bufs["db1"].t, bufs["dw2"].t, bufs["db2"].t, dmean=dmean.t)
    o32 = _gate_bwd_ref(dgate, gate, hidden, mean, w1, w2, inv_n, F32)
    o64 = _gate_bwd_ref(dgate, gate, hidden, mean, w1, w2, inv_n, torch.float64)
    _floor_check(f"se_gate_bwd {shape} dmean", dmean.get(), o32["dmean"], o64["dmean"])
    for k, v in init.items():
        got = bufs[k].get()
        # added to: the buffer is init + gradient; both sides relative to the gradient's norm
        _floor_check(f"se_gate_bwd {shape} {k}", got, v + o32[k], v.double() + o64[k], den=float(o64[k].norm()))
    off = (hidden == 0).all(0)                                              # units off in every batch item
    assert int(off.sum()) > 0 or R == 1
    assert torch.equal(bufs["dw1"].get()[off], init["dw1"][off]), "a hidden unit with h == 0 passed a gradient"
    assert torch.equal(bufs["db1"].get()[off], init["db1"][off])


# ============================================================================ refusals
def _raw(name, *args):
    K = _K()
    return int(getattr(_lib(), name)(*[K.p(a) if torch.is_tensor(a) else a for a in args], K.S()))


def test_se_refusals():
    K = _K()
    L = _lib()
    sent = lambda b: bool((b.get() == SENT).all())                          # noqa: E731
    # --- C = 1025: the row passes and the gate refuse, nothing is written
    B, N, C, R = 1, 4, 1025, 16
    x = torch.ones((B * N, C), device=DEV)
    small = torch.ones((B, C), device=DEV)
    wsb = int(L.dlcs_se_pool_workspace_bytes(B, N, C))
    ws = torch.empty((max(wsb, 1 << 20),), dtype=torch.uint8, device=DEV)
    out_rows, out_bc, out_br = _Buf((B * N, C)), _Buf((B, C)), _Buf((B, R))
    assert _raw("dlcs_se_pool", x, B, N, C, C, out_bc.t, ws, ws.numel()) == ERR_UNSUPPORTED
    assert _raw("dlcs_se_bwd_reduce", x, x, x, B, N, C, C, out_bc.t, ws, ws.numel()) == ERR_UNSUPPORTED
    assert _raw("dlcs_se_scale_res_relu", x, small, x, out_rows.t, B, N, C, C) == ERR_UNSUPPORTED
    g = _Buf((B * N, C))
    assert _raw("dlcs_se_bwd_apply", g.t, x, small, small, out_rows.t, B, N, C, C) == ERR_UNSUPPORTED
    w1, w2 = torch.ones((R, C), device=DEV), torch.ones((C, R), device=DEV)
    b1, b2 = torch.ones((R,), device=DEV), torch.ones((C,), device=DEV)
    assert _raw("dlcs_se_gate", small, w1, b1, w2, b2, B, C, R, out_br.t, out_bc.t) == ERR_UNSUPPORTED
    pg = [_Buf((R, C)), _Buf((R,)), _Buf((C, R)), _Buf((C,))]
    hid = torch.ones((B, R), device=DEV)
    assert _raw("dlcs_se_gate_bwd", small, small, hid, small, w1, w2, B, C, R, 1.0, pg[0].t, pg[1].t, pg[2].t, pg[3].t,
                out_bc.t, ws, ws.numel()) == ERR_UNSUPPORTED
    assert all(sent(b) for b in (out_rows, out_bc, out_br, g, *pg))
    # --- R = 257
    C, R = 64, 257
    small = torch.ones((B, C), device=DEV)
    w1, w2 = torch.ones((R, C), device=DEV), torch.ones((C, R), device=DEV)
    b1, b2 = torch.ones((R,), device=DEV), torch.ones((C,), device=DEV)
    hid = torch.ones((B, R), device=DEV)
    out_bc, out_br = _Buf((B, C)), _Buf((B, R))
    pg = [_Buf((R, C)), _Buf((R,)), _Buf((C, R)), _Buf((C,))]
    assert _raw("dlcs_se_gate", small, w1, b1, w2, b2, B, C, R, out_br.t, out_bc.t) == ERR_UNSUPPORTED
    assert _raw("dlcs_se_gate_bwd", small, small, hid, small, w1, w2, B, C, R, 1.0, pg[0].t, pg[1].t, pg[2].t, pg[3].t,
                out_bc.t, ws, ws.numel()) == ERR_UNSUPPORTED
    assert all(sent(b) for b in (out_bc, out_br, *pg))
    # --- workspace one byte short
    B, N, C, R = 2, 768, 64, 16
    x = torch.ones((B * N, C), device=DEV)
    small = torch.ones((B, C), device=DEV)
    hid = torch.ones((B, R), device=DEV)
    w1, w2 = torch.ones((R, C), device=DEV), torch.ones((C, R), device=DEV)
    out_bc = _Buf((B, C))
    pg = [_Buf((R, C)), _Buf((R,)), _Buf((C, R)), _Buf((C,))]
    nb = int(L.dlcs_se_pool_workspace_bytes(B, N, C))
    assert nb > 0 and nb == int(L.dlcs_se_bwd_reduce_workspace_bytes(B, N, C))
    assert _raw("dlcs_se_pool", x, B, N, C, C, out_bc.t, ws, nb - 1) == ERR_WORKSPACE
    assert _raw("dlcs_se_bwd_reduce", x, x, x, B, N, C, C, out_bc.t, ws, nb - 1) == ERR_WORKSPACE
    nbg = int(L.dlcs_se_gate_bwd_workspace_bytes(B, C, R))
    assert nbg > 0
    assert _raw("dlcs_se_gate_bwd", small, small, hid, small, w1, w2, B, C, R, 1.0, pg[0].t, pg[1].t, pg[2].t, pg[3].t,
                out_bc.t, ws, nbg - 1) == ERR_WORKSPACE
    assert _raw("dlcs_se_pool", x, B, N, C, C, out_bc.t, None, 0) == ERR_WORKSPACE
    assert all(sent(b) for b in (out_bc, *pg))
    torch.cuda.synchronize()
    # and the exact size is enough
    assert _raw("dlcs_se_pool", x, B, N, C, C, out_bc.t, ws, nb) == 0
    assert torch.equal(out_bc.get(), torch.ones((B, C)))
