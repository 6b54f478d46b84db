"""Direct unit checks of the CBAM spatial-gate kernels (csrc/cbam.hip) in the style of
test_gpu_se_kernels.py: every reference is float64 (or exact) on the CPU, every output
sits between sentinel margins, the pad columns [C, ld) of the row operands hold 1e30 on
input (a read of them shows) and keep their sentinel on output.  Row operands are built
from dense [B, D, H, W, C] values through the patch-blocked row formula (layout.hip).

Tolerances come from what each kernel does (u = 2^-24, the fp32 unit roundoff):
  * a k-term fp32 sum in any order, each term one rounded product, is within
    (k + 1) u sum|terms| of the exact value: k = 126 for the stencil (125 taps and the
    bias), k = C + 1 for the row dots (C products and the final scale);
  * scale_res_relu rounds three times (q s, that times o, the add): per element
    |got - ref64| <= 2^-21 (|q s o| + |res|), three roundings with margin 2 and more;
    bwd_apply likewise with the product (|gz q| + |da / C|) s, the magnitudes that enter
    e = gz q + da / C before it can cancel, and the addend dmean;
  * reductions over voxels (bwd_reduce, stencil5_wgrad): NRMSE < 1e-6 against float64,
    the bar _colsum_check sets for fp32 column sums; two calls agree bit for bit.

  entry point                 test
  --------------------------  ---------------------------------------------------
  dlcs_cbam_chan_mean         test_cbam_chan_mean, test_cbam_refusals
  dlcs_cbam_bwd_rowdot        test_cbam_bwd_rowdot, test_cbam_refusals
  dlcs_cbam_scale_res_relu    test_cbam_scale_res_relu, test_cbam_refusals
  dlcs_cbam_bwd_apply         test_cbam_bwd_apply, test_cbam_refusals
  dlcs_cbam_bwd_reduce        test_cbam_bwd_reduce, test_cbam_refusals
  dlcs_cbam_stencil5          test_cbam_stencil5, test_cbam_stencil5_adjoint, test_cbam_refusals
  dlcs_cbam_stencil5_wgrad    test_cbam_stencil5_wgrad, test_cbam_refusals
"""
import pytest
import torch
import torch.nn.functional as F

from goldutil import nrmse
from test_gpu_se_kernels import DEV, ERR_UNSUPPORTED, ERR_WORKSPACE, F32, PADV, SENT, _Buf, _bits, _gates, _raw, _rnd

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
ERR_INVALID = 100001

# (B, D, H, W, C, ld, misaligned): one patch; vector path with C % 8 != 0; the scalar path
# (C % 4 != 0); three items at 384 channels (a row's 64 lanes take two chunks each); many
# workgroups per item and a grid no tile divides; the scalar path by a 4-byte-misaligned view
ROW_SHAPES = [(1, 4, 4, 4, 64, 64, False), (2, 8, 12, 20, 40, 40, False), (2, 4, 8, 12, 7, 8, False),
              (3, 4, 4, 20, 384, 384, False), (1, 28, 8, 36, 64, 64, False), (2, 8, 12, 20, 40, 40, True)]
_row_params = pytest.mark.parametrize("shape", ROW_SHAPES,
                                      ids=lambda s: "x".join(map(str, s[:6])) + ("-mis" if s[6] else ""))
# (B, D, H, W): every voxel sees every border; several tiles in t and y; several in t and x;
# larger than the 4 x 8 x 32 tile in each dimension, no dimension a multiple of it; odd sizes
GRIDS = [(1, 4, 4, 4), (2, 8, 12, 20), (1, 28, 8, 36), (2, 12, 20, 40), (1, 5, 9, 33)]
_grid_params = pytest.mark.parametrize("grid", GRIDS, ids=lambda s: "x".join(map(str, s)))


def _K():
    from dl_cs.models import _ops as K
    return K


def _lib():
    from dl_cs import _lib
    return _lib.lib()


def _row_of_voxel(D, H, W):
    """[D H W] long: the patch-blocked row (within a batch item) of each dense voxel."""
    t, y, x = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
    row = (((t // 4) * (H // 4) + y // 4) * (W // 4) + x // 4) * 64 + (t % 4) * 16 + (y % 4) * 4 + x % 4
    return row.reshape(-1)


class _Case:
    """Dense random operands of one row shape, their row forms on the device."""

    def __init__(self, shape, seed):
        self.B, self.D, self.H, self.W, self.C, self.ld, self.mis = shape
        self.N = self.D * self.H * self.W
        self.grid = shape[:4]
        self.row = _row_of_voxel(self.D, self.H, self.W)
        assert sorted(self.row.tolist()) == list(range(self.N))
        self.seed = seed

    def dense(self, k, scale_items=False):
        x = _rnd((self.B, self.N, self.C), self.seed + k)
        if scale_items:
            x = x + (1.0 + 2.0 * torch.arange(self.B, dtype=F32))[:, None, None]
        return x

    def rows(self, dense):
        B, N, C = dense.shape
        out = torch.full((B, N, self.ld), PADV, dtype=F32)
        out[:, self.row, :C] = dense
        return out.view(B * N, self.ld)

    def relu_dense(self, k):
        """exact 0.0, -0.0, NaN and negatives at fixed positions (k = 1, 2, 3, 4 of every 6)."""
        n = self.B * self.N * self.C
        a = _rnd((n,), self.seed + k).abs() + 0.125
        i = (torch.arange(n) + self.C) % 6
        a[i == 1] = 0.0
        a[i == 2] = -0.0
        a[i == 3] = float("nan")
        a[i == 4] *= -1.0
        return a.view(self.B, self.N, self.C)

    def buf(self, rows):
        return _Buf(rows.shape, init=rows, mis=self.mis)

    def from_rows(self, rows):
        """rows [B N, ld] -> dense [B, N, C]"""
        return rows.view(self.B, self.N, self.ld)[:, self.row, :self.C]

    def map(self, k, offset=0.0):
        return _rnd((self.B, self.N), self.seed + k) + offset


def _item_gates(B, C, seed):
    return _gates(B, C, seed) * (1.0 + torch.arange(B, dtype=F32))[:, None] / B       # items differ: a mixed-up b shows


# ============================================================================ row dots
@_row_params
def test_cbam_chan_mean(shape):
    K = _K()
    cs = _Case(shape, 100)
    o = cs.dense(0, scale_items=True)
    s = _item_gates(cs.B, cs.C, 101)
    orow = cs.rows(o)
    od = cs.buf(orow)
    outs = []
    for _ in range(2):
        a = _Buf(cs.grid)
        K.cbam_chan_mean(od.t, s.to(DEV), cs.grid, cs.C, out=a.t)
        outs.append(a.get().view(cs.B, cs.N))
    terms = o.double() * s.double()[:, None, :] / cs.C
    ref, bound = terms.sum(-1), (cs.C + 2) * U * terms.abs().sum(-1)
    err = (outs[0].double() - ref).abs()
    print(f"cbam_chan_mean {shape}: worst err/bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two calls on the same input differ"
    assert torch.equal(od.get(), orow)


@_row_params
def test_cbam_bwd_rowdot(shape):
    K = _K()
    cs = _Case(shape, 200)
    o, g, rn = cs.dense(0), cs.dense(1) + 0.5, cs.relu_dense(2)
    keep = rn > 0                                            # NaN, 0.0, -0.0 and negatives: dropped
    g = torch.where(keep, g, torch.full_like(g, 1e18))       # a dropped element that leaks shows
    s = _item_gates(cs.B, cs.C, 203)
    od, gd, rd = cs.buf(cs.rows(o)), cs.buf(cs.rows(g)), cs.buf(cs.rows(rn))
    dq = _Buf(cs.grid)
    K.cbam_bwd_rowdot(gd.t, rd.t, od.t, s.to(DEV), cs.grid, cs.C, dq=dq.t)
    got = dq.get().view(cs.B, cs.N)
    terms = torch.where(keep, g.double() * s.double()[:, None, :] * o.double(), torch.zeros((), dtype=torch.float64))
    ref, bound = terms.sum(-1), (cs.C + 2) * U * terms.abs().sum(-1)
    assert torch.isfinite(got).all(), "a NaN of r_next (or a dropped element) reached the sum"
    err = (got.double() - ref).abs()
    print(f"cbam_bwd_rowdot {shape}: worst err/bound {float((err / bound.clamp_min(1e-300)).max()):.3g}")
    assert bool((err <= bound).all())
    assert torch.equal(_bits(gd.get()), _bits(cs.rows(g))) and torch.equal(_bits(rd.get()), _bits(cs.rows(rn)))


# ============================================================================ reduction over voxels
@_row_params
def test_cbam_bwd_reduce(shape):
    K = _K()
    cs = _Case(shape, 300)
    o, g, rn = cs.dense(0, scale_items=True), cs.dense(1) + 0.5, cs.relu_dense(2)
    keep = rn > 0
    g = torch.where(keep, g, torch.full_like(g, 1e18))
    q, da = cs.map(3, 1.0), cs.map(4, 0.5) * cs.C
    od, gd, rd = cs.buf(cs.rows(o)), cs.buf(cs.rows(g)), cs.buf(cs.rows(rn))
    outs = []
    for _ in range(2):
        ds = _Buf((cs.B, cs.C))
        K.cbam_bwd_reduce(gd.t, rd.t, od.t, q.view(cs.grid).to(DEV), da.view(cs.grid).to(DEV), cs.grid, cs.C, dgate=ds.t)
        outs.append(ds.get())
    gz = torch.where(keep, g.double(), torch.zeros((), dtype=torch.float64))
    e = gz * q.double()[:, :, None] + da.double()[:, :, None] / cs.C
    ref = (e * o.double()).sum(1)
    assert torch.isfinite(outs[0]).all(), "a NaN of r_next (or a dropped element) reached the sum"
    err = nrmse(ref.numpy(), outs[0].double().numpy())
    print(f"cbam_bwd_reduce {shape}: NRMSE vs float64 {err:.3g}")
    assert err < 1e-6
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two calls on the same input differ"


# ============================================================================ element-wise passes
@_row_params
def test_cbam_scale_res_relu(shape):
    K = _K()
    cs = _Case(shape, 400)
    o, res = cs.dense(0), cs.dense(1)
    s = _item_gates(cs.B, cs.C, 402)
    q = cs.map(3, 1.0)
    orow, rrow = cs.rows(o), cs.rows(res)
    od, rd = cs.buf(orow), cs.buf(rrow)
    out = _Buf((cs.B * cs.N, cs.ld), mis=cs.mis)
    qd = q.view(cs.grid).to(DEV)
    K.cbam_scale_res_relu(od.t, s.to(DEV), qd, rd.t, cs.grid, cs.C, out=out.t)
    rows = out.get()
    assert torch.equal(rows[:, cs.C:], torch.full((cs.B * cs.N, cs.ld - cs.C), SENT)), "pad columns written"
    got = cs.from_rows(rows)
    prod = q.double()[:, :, None] * s.double()[:, None, :] * o.double()
    pre = prod + res.double()
    bound = 2.0 ** -21 * (prod.abs() + res.double().abs())
    err = (got.double() - pre.clamp_min(0.0)).abs()
    print(f"cbam_scale_res_relu {shape}: worst err/bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())
    dropped = pre < -bound
    assert int(dropped.sum()) > 0
    assert torch.equal(_bits(got[dropped]), torch.zeros(int(dropped.sum()), dtype=torch.int32)), "dropped: not +0"
    assert not bool(((got == 0) & (_bits(got.contiguous()) != 0)).any()), "-0 written"
    # out aliasing res: the same bits, o untouched
    K.cbam_scale_res_relu(od.t, s.to(DEV), qd, rd.t, cs.grid, cs.C, out=rd.t)
    alias = rd.get()
    assert torch.equal(_bits(alias[:, :cs.C]), _bits(rows[:, :cs.C]))
    assert torch.equal(alias[:, cs.C:], rrow[:, cs.C:])
    assert torch.equal(od.get(), orow)


@_row_params
def test_cbam_bwd_apply(shape):
    K = _K()
    cs = _Case(shape, 500)
    g0, rn = cs.dense(0), cs.relu_dense(1)
    s = _item_gates(cs.B, cs.C, 502)
    dm = _rnd((cs.B, cs.C), 503) * (1.0 + torch.arange(cs.B, dtype=F32))[:, None]
    q, da = cs.map(4, 1.0), cs.map(5) * cs.C
    grow, rrow = cs.rows(g0), cs.rows(rn)
    gd, rd = cs.buf(grow), cs.buf(rrow)
    dout = _Buf((cs.B * cs.N, cs.ld), mis=cs.mis)
    K.cbam_bwd_apply(gd.t, rd.t, s.to(DEV), q.view(cs.grid).to(DEV), da.view(cs.grid).to(DEV), dm.to(DEV), cs.grid, cs.C,
                     dout=dout.t)
    g1rows, drows = gd.get(), dout.get()
    g1, d = cs.from_rows(g1rows), cs.from_rows(drows)
    keep = rn > 0
    gz = torch.where(keep, g0, torch.zeros_like(g0))
    assert torch.equal(_bits(g1.contiguous()), _bits(gz)), "g is not relu_grad's result"
    gr = g0.contiguous().to(DEV)                                                # and bitwise dlcs_relu_grad itself
    K.relu_grad(gr, rn.contiguous().to(DEV))
    assert torch.equal(_bits(g1.contiguous()), _bits(gr.cpu()))
    assert torch.equal(g1rows[:, cs.C:], grow[:, cs.C:]), "pad columns of g written"
    assert torch.equal(drows[:, cs.C:], torch.full((cs.B * cs.N, cs.ld - cs.C), SENT)), "pad columns of dout written"
    sd, dmd = s.double()[:, None, :], dm.double()[:, None, :]
    gq, daf = gz.double() * q.double()[:, :, None], (da.double() / cs.C)[:, :, None]
    ref = (gq + daf) * sd + dmd
    bound = 2.0 ** -21 * ((gq.abs() + daf.abs()) * sd + dmd.abs())
    err = (d.double() - ref).abs()
    print(f"cbam_bwd_apply {shape}: worst err/bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())
    assert torch.equal(_bits(rd.get()), _bits(rrow))


# ============================================================================ stencils
def _stencil_case(grid, seed):
    B, D, H, W = grid
    a = _rnd(grid, seed) + 1.0
    w = 0.2 * _rnd((1, 1, 5, 5, 5), seed + 1)
    b = torch.tensor([0.75])
    return a, w, b


def _conv64(x, w, b=None):
    return F.conv3d(x.double()[:, None], w.double(), None if b is None else b.double(), padding=2)[:, 0]


def _stencil_bound(x, w, b=None):
    mag = F.conv3d(x.double().abs()[:, None], w.double().abs(), None if b is None else b.double().abs(), padding=2)[:, 0]
    return 127 * U * mag


def _run_stencil(x, w, b, transposed):
    K = _K()
    xd = _Buf(x.shape, init=x)
    out = _Buf(x.shape)
    K.cbam_stencil5(xd.t, w.to(DEV), None if transposed else b.to(DEV), tuple(x.shape), transposed=transposed, out=out.t)
    got = out.get()
    assert torch.equal(xd.get(), x)
    return got


@_grid_params
def test_cbam_stencil5(grid):
    a, w, b = _stencil_case(grid, 600)
    got = _run_stencil(a, w, b, False)
    err, bound = (got.double() - _conv64(a, w, b)).abs(), _stencil_bound(a, w, b)
    print(f"cbam_stencil5 {grid}: worst err/bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())
    # transposed: the cross-correlation with the kernel flipped in all three dimensions, no bias
    gt = _run_stencil(a, w, b, True)
    wf = torch.flip(w, dims=(2, 3, 4))
    errt, boundt = (gt.double() - _conv64(a, wf)).abs(), _stencil_bound(a, wf)
    print(f"cbam_stencil5 transposed {grid}: worst err/bound {float((errt / boundt).max()):.3g}")
    assert bool((errt <= boundt).all())


@_grid_params
def test_cbam_stencil5_adjoint(grid):
    """<stencil(a) - b5, d> = <a, stencil^T(d)>, each side within its elements' bounds."""
    a, w, b = _stencil_case(grid, 610)
    d = _rnd(grid, 612)
    fa = _run_stencil(a, w, b, False).double() - float(b)
    td = _run_stencil(d, w, b, True).double()
    lhs, rhs = float((fa * d.double()).sum()), float((a.double() * td).sum())
    wf = torch.flip(w, dims=(2, 3, 4))
    bound = float((_stencil_bound(a, w, b) * d.double().abs()).sum() + (_stencil_bound(d, wf) * a.double().abs()).sum())
    print(f"cbam_stencil5 adjoint {grid}: {lhs:.9g} vs {rhs:.9g}, |diff| / bound {abs(lhs - rhs) / bound:.3g}")
    assert abs(lhs - rhs) <= bound


@_grid_params
def test_cbam_stencil5_wgrad(grid):
    K = _K()
    a, w, b = _stencil_case(grid, 620)
    dq = _rnd(grid, 622) + 0.5
    w64 = w.double().requires_grad_()
    b64 = b.double().requires_grad_()
    (F.conv3d(a.double()[:, None], w64, b64, padding=2)[:, 0] * dq.double()).sum().backward()
    init_w, init_b = _rnd((1, 1, 5, 5, 5), 623), _rnd((1,), 624)
    ad, dd = _Buf(grid, init=a), _Buf(grid, init=dq)
    outs = []
    for _ in range(2):
        dw, db = _Buf(init_w.shape, init=init_w), _Buf((1,), init=init_b)
        K.cbam_stencil5_wgrad(dd.t, ad.t, grid, dw.t, db.t)
        outs.append((dw.get(), db.get()))
    dw, db = outs[0]
    ew = float((dw.double() - (init_w.double() + w64.grad)).norm() / w64.grad.norm())
    eb = float((db.double() - (init_b.double() + b64.grad)).norm() / b64.grad.norm())
    print(f"cbam_stencil5_wgrad {grid}: NRMSE vs float64 dw5 {ew:.3g}, db5 {eb:.3g}")
    assert ew < 1e-6 and eb < 1e-6
    assert torch.equal(_bits(dw), _bits(outs[1][0])) and torch.equal(_bits(db), _bits(outs[1][1])), "two calls differ"
    assert torch.equal(ad.get(), a) and torch.equal(dd.get(), dq)


# ============================================================================ refusals
def test_cbam_refusals():
    L = _lib()
    sent = lambda b: bool((b.get() == SENT).all())                          # noqa: E731
    ws = torch.empty((1 << 20,), dtype=torch.uint8, device=DEV)

    def row_calls(B, D, H, W, C, expect):
        N = D * H * W
        x = torch.ones((B * N, C), device=DEV)
        small = torch.ones((B, C), device=DEV)
        m = torch.ones((B, D, H, W), device=DEV)
        out_rows, out_map, out_bc, g = _Buf((B * N, C)), _Buf((B, D, H, W)), _Buf((B, C)), _Buf((B * N, C))
        assert _raw("dlcs_cbam_chan_mean", x, small, B, D, H, W, C, C, out_map.t) == expect
        assert _raw("dlcs_cbam_bwd_rowdot", x, x, x, small, B, D, H, W, C, C, out_map.t) == expect
        assert _raw("dlcs_cbam_scale_res_relu", x, small, m, x, out_rows.t, B, D, H, W, C, C) == expect
        assert _raw("dlcs_cbam_bwd_reduce", x, x, x, m, m, B, D, H, W, C, C, out_bc.t, ws, ws.numel()) == expect
        assert _raw("dlcs_cbam_bwd_apply", g.t, x, small, m, m, small, out_rows.t, B, D, H, W, C, C) == expect
        assert all(sent(b) for b in (out_rows, out_map, out_bc, g))
        assert int(L.dlcs_cbam_bwd_reduce_workspace_bytes(B, D, H, W, C)) == 0

    # --- C = 1025, and a grid dimension that is no multiple of 4: the row passes refuse, nothing is written
    row_calls(1, 4, 4, 4, 1025, ERR_UNSUPPORTED)
    for dims in ((6, 4, 4), (4, 6, 4), (4, 4, 6)):
        row_calls(1, *dims, 8, ERR_UNSUPPORTED)
    # --- invalid arguments: an output aliasing the operand it may not, ld < C, a missing bias
    B, D, H, W, C = 1, 4, 4, 4, 8
    x = _Buf((B * D * H * W, C), init=1.0)
    small = torch.ones((B, C), device=DEV)
    m, m2 = _Buf((B, D, H, W), init=1.0), _Buf((B, D, H, W))
    w5 = torch.ones((125,), device=DEV)
    assert _raw("dlcs_cbam_scale_res_relu", x.t, small, m.t, x.t, x.t, B, D, H, W, C, C) == ERR_INVALID
    assert _raw("dlcs_cbam_bwd_apply", x.t, x.t, small, m.t, m.t, small, x.t, B, D, H, W, C, C) == ERR_INVALID
    assert _raw("dlcs_cbam_chan_mean", x.t, small, B, D, H, W, C, C - 1, m2.t) == ERR_INVALID
    assert _raw("dlcs_cbam_stencil5", m.t, w5, small, 0, m.t, B, D, H, W) == ERR_INVALID
    assert _raw("dlcs_cbam_stencil5", m.t, w5, None, 0, m2.t, B, D, H, W) == ERR_INVALID
    assert _raw("dlcs_cbam_stencil5", m.t, w5, None, 1, m2.t, 0, D, H, W) == ERR_INVALID
    assert sent(m2) and torch.equal(x.get(), torch.ones((B * D * H * W, C))) and torch.equal(m.get(), torch.ones((B, D, H, W)))
    # --- workspace one byte short, or missing
    B, D, H, W, C = 2, 8, 12, 20, 64
    N = D * H * W
    x = torch.ones((B * N, C), device=DEV)
    m = torch.ones((B, D, H, W), device=DEV)
    out_bc, dw, db = _Buf((B, C)), _Buf((125,)), _Buf((1,))
    nb = int(L.dlcs_cbam_bwd_reduce_workspace_bytes(B, D, H, W, C))
    nw = int(L.dlcs_cbam_stencil5_wgrad_workspace_bytes(B, D, H, W))
    assert nb > 0 and nw > 0
    assert _raw("dlcs_cbam_bwd_reduce", x, x, x, m, m, B, D, H, W, C, C, out_bc.t, ws, nb - 1) == ERR_WORKSPACE
    assert _raw("dlcs_cbam_bwd_reduce", x, x, x, m, m, B, D, H, W, C, C, out_bc.t, None, 0) == ERR_WORKSPACE
    assert _raw("dlcs_cbam_stencil5_wgrad", m, m, B, D, H, W, dw.t, db.t, ws, nw - 1) == ERR_WORKSPACE
    assert _raw("dlcs_cbam_stencil5_wgrad", m, m, B, D, H, W, dw.t, db.t, None, 0) == ERR_WORKSPACE
    assert all(sent(b) for b in (out_bc, dw, db))
    torch.cuda.synchronize()
    # and the exact size is enough: sum_v (1 * 1 + 1 / C) * 1 per channel; N voxels into the bias gradient
    assert _raw("dlcs_cbam_bwd_reduce", x, x, x, m, m, B, D, H, W, C, C, out_bc.t, ws, nb) == 0
    assert torch.allclose(out_bc.get(), torch.full((B, C), N * (1.0 + 1.0 / C)), rtol=1e-6, atol=0)
    dw0, db0 = _Buf((125,), init=0.0), _Buf((1,), init=0.0)
    assert _raw("dlcs_cbam_stencil5_wgrad", m, m, B, D, H, W, dw0.t, db0.t, ws, nw) == 0
    assert float(db0.get()) == B * N and float(dw0.get()[62]) == B * N       # the centre tap sees every voxel
