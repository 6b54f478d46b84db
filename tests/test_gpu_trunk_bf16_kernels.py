"""Kernel checks of the bf16 path of the conv trunks (ResNet / SE / CBAM regularisers):

  dlcs_conv3d_k3_wgrad, bf16, every channel pair the trunks produce (conv3d_wgrad_row.inc)
  dlcs_conv3d_k3, bf16, forward / dgrad at the trunks' channel counts (generic kernel)
  dlcs_box_pre_bf16 / _post_bwd_bf16 / _zero_bf16 against their fp32 siblings
  the nine gate row passes (dlcs_se_*_bf16, dlcs_cbam_*_bf16) against their fp32 siblings on the
  same inputs upcast from bf16

References: float64 F.conv3d autograd on the bf16-quantised operands (the convs), the fp32
sibling on the same inputs (box kernels).  Bounds: quantised operands, fp32 accumulation and
fp32 output leave only the summation order, NRMSE < 1e-5 (dbias < 1e-6); a bf16 output adds
its one rounding, NRMSE <= 4e-3 (half an ulp of 2^-8 relative per element).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from goldutil import nrmse

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
GRIDS = [(1, 8, 16, 12), (2, 4, 8, 16)]
SENT = -12345.0


@pytest.fixture(autouse=True)
def _fp32_after():
    yield
    from dl_cs.models import swin3D
    swin3D.set_compute_dtype(torch.float32)


def _K():
    from dl_cs.models import _ops as K
    return K


def _rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _to_blocked(x):
    B, C, D, H, W = x.shape
    t = x.permute(0, 2, 3, 4, 1).reshape(B, D // 4, 4, H // 4, 4, W // 4, 4, C)
    return t.permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(-1, C)


def _from_blocked(r, B, C, D, H, W):
    t = r.reshape(B, D // 4, H // 4, W // 4, 4, 4, 4, C).permute(0, 1, 4, 2, 5, 3, 6, 7)
    return t.reshape(B, D, H, W, C).permute(0, 4, 1, 2, 3)


def _rows(x, ld, fill=0.0):
    """[B, C, D, H, W] -> bf16 rows [rows, ld] on the GPU (columns >= C: fill) and the quantised tensor back."""
    B, C, D, H, W = x.shape
    r = torch.full((B * D * H * W, ld), fill)
    r[:, :C] = _to_blocked(x)
    rd = r.to(DEV, BF16)
    return rd, _from_blocked(rd[:, :C].float().cpu(), B, C, D, H, W).double()


# ---------------------------------------------------------------------------- weight gradient
# (cin, cout, cin_ld, g_ld): the trunk's 64 x 64, partial tiles, two 128s, the thin ends in rows of 8
WG_PAIRS = [(64, 64, 64, 64), (40, 64, 40, 64), (64, 24, 64, 24), (128, 64, 128, 64), (64, 128, 64, 128),
            (2, 64, 8, 64), (64, 4, 64, 8), (4, 32, 8, 32)]


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("pair", WG_PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_wgrad_bf16_pairs(pair, grid):
    """dw_packed += and dbias += on sentinel-filled buffers, vox_per_block = 256 (4 patches per
    range, so 6 / 4 ranges meet in every dW element); columns >= C of the rows hold a value that
    a kernel reading them as channels would carry into dW."""
    K = _K()
    cin, cout, cin_ld, g_ld = pair
    B, D, H, W = grid
    xd, xq = _rows(_rnd((B, cin, D, H, W), 10), cin_ld, fill=3.0)
    gd, gq = _rows(_rnd((B, cout, D, H, W), 14), g_ld, fill=-2.0)
    dwp = torch.full((27, K.pad32(cout), K.pad32(cin)), 0.5, device=DEV)
    db = torch.full((cout,), -0.25, device=DEV)
    K.conv3d_wgrad(xd, cin, 0, gd, cout, grid, dwp, vox_per_block=256, dbias=db)
    gw = torch.zeros((cout, cin, 3, 3, 3), device=DEV)
    K.conv_unpack_grad(dwp, gw, cout, cin)
    wr = torch.zeros((cout, cin, 3, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv3d(xq, wr, None, padding=1).backward(gq)
    e_w = nrmse((wr.grad + 0.5).numpy(), gw.cpu().double().numpy())
    e_b = nrmse((gq.sum(dim=(0, 2, 3, 4)) - 0.25).numpy(), db.cpu().double().numpy())
    print(f"wgrad bf16 {pair} {grid}: dW {e_w:.3g}  dbias {e_b:.3g}")
    assert e_w < 1e-5
    assert e_b < 1e-6
    # the 160-channel routes have workspaces; the tap-row kernel has none and says so
    from dl_cs import _lib
    assert _lib.lib().dlcs_conv3d_k3_wgrad_workspace_bytes(K.BF16, cin, K.pad32(cin), cout, K.pad32(cout), 0, 1,
                                                           B, D, H, W) == 0


def test_wgrad_bf16_relu_in_refused():
    """relu_in = 1 on a pair of the tap-row kernel: DLCS_ERR_UNSUPPORTED_SIZE, dW untouched (dlcs.h)."""
    K = _K()
    from dl_cs import _lib
    grid = GRIDS[0]
    xd, _ = _rows(_rnd((1, 64) + grid[1:], 10), 64)
    dwp = torch.full((27, 64, 64), SENT, device=DEV)
    with pytest.raises(_lib.DlcsError, match="unsupported size"):
        K.conv3d_wgrad(xd, 64, 1, xd, 64, grid, dwp, vox_per_block=256)
    assert bool((dwp == SENT).all())


# ---------------------------------------------------------------------------- forward / dgrad
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("cin,cout", [(64, 64), (40, 64), (128, 128), (24, 24)])
def test_conv_bf16_trunk_channels(cin, cout, grid):
    """The two epilogues the trunks use: bias + bf16 residual + ReLU-out, and the input
    gradient behind a bf16 ReLU mask; fp32 and bf16 outputs."""
    K = _K()
    B, D, H, W = grid
    w = _rnd((cout, cin, 3, 3, 3), 11) / (27 * cin) ** 0.5
    b = _rnd((cout,), 12)
    wq = w.to(BF16).double()
    xd, xq = _rows(_rnd((B, cin, D, H, W), 10), cin)
    rd, rq = _rows(_rnd((B, cout, D, H, W), 13), cout)
    wp, wdp = K.conv_pack(w.to(DEV), BF16, 0), K.conv_pack(w.to(DEV), BF16, 1)
    ref = F.relu(F.conv3d(xq, wq, b.double(), padding=1) + rq).numpy()
    xr_ = xq.clone().requires_grad_()
    F.conv3d(F.relu(xr_), wq, None, padding=1).backward(rq)
    dref = xr_.grad.numpy()
    for out_dtype, tol in ((torch.float32, 1e-5), (BF16, 4e-3)):
        f = K.conv3d(xd, cin, wp, cout, cout, grid, bias=b.to(DEV), res=rd, relu_out=1, out_dtype=out_dtype)
        d = K.conv3d(rd, cout, wdp, cin, cin, grid, mask=xd, out_dtype=out_dtype)
        assert f.dtype == out_dtype and d.dtype == out_dtype
        e_f = nrmse(ref, _from_blocked(f.float().cpu(), B, cout, D, H, W).double().numpy())
        e_d = nrmse(dref, _from_blocked(d.float().cpu(), B, cin, D, H, W).double().numpy())
        print(f"conv bf16 {cin}->{cout} {grid} out {out_dtype}: fwd {e_f:.3g}  dgrad {e_d:.3g}")
        assert max(e_f, e_d) < tol if out_dtype == torch.float32 else max(e_f, e_d) <= tol


# ---------------------------------------------------------------------------- box kernels
BOX_SHAPE, BOX_PAD = (2, 1, 3, 10, 13), 2           # box (2, 7, 10, 13) in the grid (2, 8, 12, 16)
BOX, PADDED = (7, 10, 13), (8, 12, 16)
LDC = 8


def _crnd(shape, seed):
    return torch.complex(_rnd(shape, seed), _rnd(shape, seed + 1000))


@pytest.mark.parametrize("name", ["box_pre", "box_post_bwd"])
def test_box_scatter_bf16(name):
    """Every row of the padded grid written; the bits of the fp32 sibling's output rounded to
    bf16 (a copy: exact, which is inside NRMSE <= 4e-3), +0.0 on slack rows and columns >= 2E."""
    K = _K()
    x = _crnd(BOX_SHAPE, 11).to(DEV)
    grid = (BOX_SHAPE[0],) + PADDED
    ref = getattr(K, name)(x, BOX_PAD, LDC, grid)
    rows = ref.shape[0]
    buf = torch.full((rows + 2 * 64, LDC), SENT, dtype=BF16, device=DEV)
    B, E, T, Y, X = BOX_SHAPE
    from dl_cs import _lib
    _lib.call(f"dlcs_{name}_bf16", K.p(x), K.p(buf[64:]), B, E, T, Y, X, BOX_PAD, *PADDED, LDC, K.S())
    got = buf.cpu()
    assert bool((got[:64] == SENT).all()) and bool((got[64 + rows:] == SENT).all())
    assert ref.dtype == torch.float32
    expect = ref.cpu().to(BF16)
    assert nrmse(expect.double().numpy(), got[64:64 + rows].double().numpy()) <= 4e-3
    assert torch.equal(got[64:64 + rows].view(torch.int16), expect.view(torch.int16))
    # and through the wrapper's dtype keyword
    assert torch.equal(getattr(K, name)(x, BOX_PAD, LDC, grid, dtype=BF16).cpu().view(torch.int16), expect.view(torch.int16))


def _slack_rows(B, box, padded):
    inside = torch.zeros((B, 1) + tuple(padded))
    inside[:, :, :box[0], :box[1], :box[2]] = 1
    return _to_blocked(inside)[:, 0] == 0


@pytest.mark.parametrize("C,ld", [(64, 64), (40, 40), (3, 3), (40, 44), (8, 8)])
def test_box_zero_bf16(C, ld):
    """16-B stores (C, ld multiples of 8), the scalar path (C = 3; ld = 44 is no multiple of 8):
    every slack row +0.0 in columns < C, no other element changes."""
    K = _K()
    B = 2
    rows = B * math.prod(PADDED)
    before = _rnd((rows, ld), 71)
    before[::7] = SENT
    before = before.to(BF16)
    buf = torch.full((rows + 2 * 64, ld), SENT, dtype=BF16, device=DEV)
    buf[64:64 + rows] = before.to(DEV)
    x = buf[64:64 + rows]
    out = K.box_zero(x, C, (B,) + PADDED, (B,) + BOX)
    assert out.data_ptr() == x.data_ptr()
    slack = _slack_rows(B, BOX, PADDED)
    assert int(slack.sum()) == B * (math.prod(PADDED) - math.prod(BOX))
    expect = torch.full((rows + 2 * 64, ld), SENT, dtype=BF16)
    expect[64:64 + rows] = before
    e = expect[64:64 + rows]
    e[slack, :C] = 0.0
    assert torch.equal(buf.cpu().view(torch.int16), expect.view(torch.int16))


# ---------------------------------------------------------------------------- gate row kernels
GATE_GRID = (2, 8, 12, 16)
GATE_N = 8 * 12 * 16
# (C, ld): 16-B path, 16-B path with five chunks, scalar path, 16-B path with unused columns
GATE_CL = [(64, 64), (40, 40), (3, 3), (40, 48)]
_gate_cl = pytest.mark.parametrize("C,ld", GATE_CL, ids=lambda v: str(v))


def _gate_rows(C, ld, seed, relu=False):
    """bf16 rows [B N, ld] (columns >= C: the sentinel) and their fp32 upcast, both on the GPU."""
    r = torch.full((GATE_GRID[0] * GATE_N, ld), SENT)
    v = _rnd((GATE_GRID[0] * GATE_N, C), seed)
    r[:, :C] = F.relu(v) if relu else v
    rb = r.to(DEV, BF16)
    return rb, rb.float()


def _vec(shape, seed):
    return _rnd(shape, seed).to(DEV)


def _same_twice(fn):
    a, b = fn(), fn()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "not bit-identical between two runs"
    return a


def _f32_close(name, got, ref):
    e = nrmse(ref.double().cpu().numpy(), got.double().cpu().numpy())
    print(f"{name}: fp32 output vs the fp32 sibling {e:.3g}")
    assert got.dtype == torch.float32 and e < 1e-6


def _rows_close(name, got, ref32, C, ld):
    """got bf16 [rows, ld] against the sibling's fp32 output rounded to bf16; columns >= C untouched."""
    assert got.dtype == BF16
    g, r = got.cpu(), ref32.cpu().to(BF16)
    e = nrmse(r[:, :C].double().numpy(), g[:, :C].double().numpy())
    print(f"{name}: bf16 rows vs the rounded fp32 sibling {e:.3g}")
    assert e <= 4e-3
    if ld > C:
        assert bool((g[:, C:] == SENT).all())


def _out_rows(ld, dtype):
    return torch.full((GATE_GRID[0] * GATE_N, ld), SENT, dtype=dtype, device=DEV)


@_gate_cl
def test_se_rows_bf16(C, ld):
    K = _K()
    B, N = GATE_GRID[0], GATE_N
    ob, of = _gate_rows(C, ld, 1)
    resb, resf = _gate_rows(C, ld, 2, relu=True)
    gb, gf = _gate_rows(C, ld, 3)
    rnb, rnf = _gate_rows(C, ld, 4, relu=True)
    gate, dmean = torch.sigmoid(_vec((B, C), 5)), _vec((B, C), 6)
    _f32_close("se_pool", _same_twice(lambda: K.se_pool(ob, B, N, C)), K.se_pool(of, B, N, C))
    _rows_close("se_scale_res_relu", K.se_scale_res_relu(ob, gate, resb, B, N, C, out=_out_rows(ld, BF16)),
                K.se_scale_res_relu(of, gate, resf, B, N, C, out=_out_rows(ld, torch.float32)), C, ld)
    _f32_close("se_bwd_reduce", _same_twice(lambda: K.se_bwd_reduce(gb, rnb, ob, B, N, C)),
               K.se_bwd_reduce(gf, rnf, of, B, N, C))
    g2b, g2f = gb.clone(), gf.clone()
    _rows_close("se_bwd_apply dout", K.se_bwd_apply(g2b, rnb, gate, dmean, B, N, C, dout=_out_rows(ld, BF16)),
                K.se_bwd_apply(g2f, rnf, gate, dmean, B, N, C, dout=_out_rows(ld, torch.float32)), C, ld)
    assert torch.equal(g2b.float(), g2f)                   # the masked gradient: a select, exact in either format
    assert torch.equal(g2b[:, :C], torch.where(rnb[:, :C] > 0, gb[:, :C], torch.zeros_like(gb[:, :C])))


@_gate_cl
def test_cbam_rows_bf16(C, ld):
    K = _K()
    B = GATE_GRID[0]
    ob, of = _gate_rows(C, ld, 11)
    resb, resf = _gate_rows(C, ld, 12, relu=True)
    gb, gf = _gate_rows(C, ld, 13)
    rnb, rnf = _gate_rows(C, ld, 14, relu=True)
    gate, dmean = torch.sigmoid(_vec((B, C), 15)), _vec((B, C), 16)
    q, da = _vec(GATE_GRID, 17), _vec(GATE_GRID, 18)
    _f32_close("cbam_chan_mean", _same_twice(lambda: K.cbam_chan_mean(ob, gate, GATE_GRID, C)),
               K.cbam_chan_mean(of, gate, GATE_GRID, C))
    _rows_close("cbam_scale_res_relu", K.cbam_scale_res_relu(ob, gate, q, resb, GATE_GRID, C, out=_out_rows(ld, BF16)),
                K.cbam_scale_res_relu(of, gate, q, resf, GATE_GRID, C, out=_out_rows(ld, torch.float32)), C, ld)
    _f32_close("cbam_bwd_rowdot", _same_twice(lambda: K.cbam_bwd_rowdot(gb, rnb, ob, gate, GATE_GRID, C)),
               K.cbam_bwd_rowdot(gf, rnf, of, gate, GATE_GRID, C))
    _f32_close("cbam_bwd_reduce", _same_twice(lambda: K.cbam_bwd_reduce(gb, rnb, ob, q, da, GATE_GRID, C)),
               K.cbam_bwd_reduce(gf, rnf, of, q, da, GATE_GRID, C))
    g2b, g2f = gb.clone(), gf.clone()
    _rows_close("cbam_bwd_apply dout",
                K.cbam_bwd_apply(g2b, rnb, gate, q, da, dmean, GATE_GRID, C, dout=_out_rows(ld, BF16)),
                K.cbam_bwd_apply(g2f, rnf, gate, q, da, dmean, GATE_GRID, C, dout=_out_rows(ld, torch.float32)), C, ld)
    assert torch.equal(g2b.float(), g2f)
    assert torch.equal(g2b[:, :C], torch.where(rnb[:, :C] > 0, gb[:, :C], torch.zeros_like(gb[:, :C])))
