"""Kernel checks of the plane conv (csrc/conv2d.hip, dlcs.h "Plane conv"): the bf16 k = 3
convolution over independent planes that the DSLR family's 2-D and 1-D ResNets run on in
compute dtype bf16.

  dlcs_conv2d_k3            forward (bias + residual + ReLU-out) and dgrad behind a bf16 ReLU mask
  dlcs_conv2d_k3_wgrad      dW += and dbias += in a fixed order, through the caller's workspace
  dlcs_conv2d_pack_weights / dlcs_conv2d_unpack_wgrad

Reference: float64 F.conv2d / F.conv1d (autograd for the gradients) on the CPU, fed the
bf16-rounded operands.  Bounds (those of test_gpu_trunk_bf16_kernels.py): quantised operands,
fp32 accumulation and fp32 output leave only the summation order, NRMSE < 1e-5; a bf16 output
adds its one rounding, NRMSE <= 4e-3 (half an ulp of 2^-8 relative per element).

Shapes (N, H, W, KH).  KH = 3: 5 planes of 4 x 4 (16 per tile: a partial tile), 3 of 8 x 8
(4 per tile), 2 of 16 x 16 (1 per tile, two workgroups), 3 of 5 x 7 (an odd plane, 7 per tile).
KH = 1: 5 sequences of 24 and of 14 (the second as N = 1, H = 5).
"""
import pytest
import torch
import torch.nn.functional as F

from goldutil import nrmse

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
SENT = -12345.0
SLACK = 3.0e4          # in the rows' columns >= C: a kernel reading them as channels carries it into the result
GUARD = 7              # sentinel rows before and after an output

SHAPES = [(5, 4, 4, 3), (3, 8, 8, 3), (2, 16, 16, 3), (3, 5, 7, 3), (5, 1, 24, 1), (1, 5, 14, 1)]
SMALL = [(12, 8), (8, 8), (8, 12)]
BIG = [(32, 128), (128, 128), (128, 32)]
CASES = [(s, p) for s in SHAPES for p in SMALL] + [((2, 16, 16, 3), p) for p in BIG]
_ids = lambda c: f"{'x'.join(map(str, c[0]))}-{c[1][0]}to{c[1][1]}"


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


def _ld(c):
    """A row length with slack: the next multiple of 8 above c (c itself a multiple of 8: c + 8)."""
    return c // 8 * 8 + 8


def _rows(x, ld, dtype=BF16):
    """[N, C, H, W] -> rows [N H W, ld] on the GPU (columns >= C: SLACK) and the quantised tensor back (float64)."""
    N, C, H, W = x.shape
    r = torch.full((N * H * W, ld), SLACK)
    r[:, :C] = x.permute(0, 2, 3, 1).reshape(-1, C)
    rd = r.to(DEV, dtype)
    return rd, rd[:, :C].float().cpu().reshape(N, H, W, C).permute(0, 3, 1, 2).double()


def _unrows(r, N, C, H, W):
    return r[:, :C].float().cpu().reshape(N, H, W, C).permute(0, 3, 1, 2).double()


def _conv(x, w, b, KH):
    """The reference conv: x [N, C, H, W]; KH 3: conv2d, KH 1: conv1d along W of every (n, h)."""
    if KH == 3:
        return F.conv2d(x, w, b, padding=1)
    N, C, H, W = x.shape
    o = F.conv1d(x.permute(0, 2, 1, 3).reshape(N * H, C, W), w, b, padding=1)
    return o.reshape(N, H, -1, W).permute(0, 2, 1, 3)


def _weight(cout, cin, KH, seed):
    shape = (cout, cin, 3, 3) if KH == 3 else (cout, cin, 3)
    return _rnd(shape, seed) / (3 * KH * cin) ** 0.5


def _guarded(rows, ld, dtype):
    buf = torch.full((rows + 2 * GUARD, ld), SENT, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + rows]


def _assert_guard(buf, rows, C):
    s = torch.tensor(SENT, dtype=buf.dtype)
    assert bool((buf[:GUARD] == s).all()) and bool((buf[GUARD + rows:] == s).all()), "guard rows written"
    assert bool((buf[GUARD:GUARD + rows, C:] == s).all()), "columns >= C written"


# ---------------------------------------------------------------------------- forward / dgrad
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_dgrad(case):
    """bias + residual + ReLU-out, and the input gradient behind a bf16 ReLU mask; fp32 output
    (fp32 residual) and bf16 output (bf16 residual) into slices of sentinel-filled buffers."""
    K = _K()
    (N, H, W, KH), (cin, cout) = case
    planes = (N, H, W, KH)
    rows = N * H * W
    w = _weight(cout, cin, KH, 11)
    b = _rnd((cout,), 12)
    wq = w.to(BF16).double()
    xd, xq = _rows(_rnd((N, cin, H, W), 10), _ld(cin))
    wp, wdp = K.conv2d_pack(w.to(DEV), 0), K.conv2d_pack(w.to(DEV), 1)
    for out_dtype, tol in ((torch.float32, 1e-5), (BF16, 4e-3)):
        rd, rq = _rows(_rnd((N, cout, H, W), 13), _ld(cout), out_dtype)      # forward residual / dgrad input
        gd, gq = (rd, rq) if out_dtype == BF16 else _rows(rq.float(), _ld(cout))
        ref = F.relu(_conv(xq, wq, b.double(), KH) + rq).numpy()
        xr = xq.clone().requires_grad_()
        _conv(F.relu(xr), wq, None, KH).backward(gq)
        fbuf, f = _guarded(rows, _ld(cout), out_dtype)
        dbuf, d = _guarded(rows, _ld(cin), out_dtype)
        K.conv2d(xd, cin, wp, cout, _ld(cout), planes, bias=b.to(DEV), res=rd, relu_out=1, out=f)
        K.conv2d(gd, cout, wdp, cin, _ld(cin), planes, mask=xd, out=d)
        _assert_guard(fbuf, rows, cout)
        _assert_guard(dbuf, rows, cin)
        e_f = nrmse(ref, _unrows(f, N, cout, H, W).numpy())
        e_d = nrmse(xr.grad.numpy(), _unrows(d, N, cin, H, W).numpy())
        print(f"conv2d {cin}->{cout} {planes} out {out_dtype}: fwd {e_f:.3g}  dgrad {e_d:.3g}")
        assert max(e_f, e_d) < tol if out_dtype == torch.float32 else max(e_f, e_d) <= tol


@pytest.mark.parametrize("planes", [(5, 4, 4, 3), (3, 5, 7, 3), (5, 1, 24, 1), (1, 5, 14, 1)], ids=lambda s: "x".join(map(str, s)))
def test_planes_independent(planes):
    """Scaling one plane's input changes that plane's output only: the others share its tile and
    are bitwise equal."""
    K = _K()
    N, H, W, KH = planes
    cin, cout = 12, 8
    wp = K.conv2d_pack(_weight(cout, cin, KH, 11).to(DEV), 0)
    x = _rnd((N, cin, H, W), 10)
    nseq, per = (N, H * W) if KH == 3 else (N * H, W)
    x2 = x.clone()
    if KH == 3:
        x2[1] *= 2.0
    else:
        x2[1 // H, :, 1 % H] *= 2.0                                   # sequence 1 = (n, h) = divmod(1, H)
    a = K.conv2d(_rows(x, _ld(cin))[0], cin, wp, cout, 8, planes, out_dtype=torch.float32).reshape(nseq, per, 8)
    b = K.conv2d(_rows(x2, _ld(cin))[0], cin, wp, cout, 8, planes, out_dtype=torch.float32).reshape(nseq, per, 8)
    others = [i for i in range(nseq) if i != 1]
    assert torch.equal(a[others], b[others])
    assert torch.equal(2.0 * a[1], b[1])                              # a power of two: exact in every format


# ---------------------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_wgrad(case):
    """dW += onto 0.5 and dbias += onto -0.25, 128 pixels per range (2 planes of 16 x 16: 4 ranges
    meet in every dW element); the queried workspace suffices and one byte less is refused; two
    runs give the same bits."""
    K = _K()
    from dl_cs import _lib
    (N, H, W, KH), (cin, cout) = case
    planes = (N, H, W, KH)
    xd, xq = _rows(_rnd((N, cin, H, W), 10), _ld(cin))
    gd, gq = _rows(_rnd((N, cout, H, W), 14), _ld(cout))
    wr = torch.zeros((cout, cin, 3, 3) if KH == 3 else (cout, cin, 3), dtype=torch.float64, requires_grad=True)
    _conv(xq, wr, None, KH).backward(gq)
    res = []
    for _ in range(2):
        dwp = torch.full((KH * 3, K.pad32(cout), K.pad32(cin)), 0.5, device=DEV)
        db = torch.full((cout,), -0.25, device=DEV)
        K.conv2d_wgrad(xd, cin, gd, cout, planes, dwp, pix_per_block=128, dbias=db)
        gw = torch.zeros(tuple(wr.shape), device=DEV)
        K.conv2d_unpack_grad(dwp, gw, cout, cin)
        res.append((gw.cpu(), db.cpu()))
    e_w = nrmse((wr.grad + 0.5).numpy(), res[0][0].double().numpy())
    e_b = nrmse((gq.sum(dim=(0, 2, 3)) - 0.25).numpy(), res[0][1].double().numpy())
    print(f"conv2d wgrad {cin}->{cout} {planes}: dW {e_w:.3g}  dbias {e_b:.3g}")
    assert e_w < 1e-5
    assert e_b < 1e-5
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    nb = int(_lib.lib().dlcs_conv2d_k3_wgrad_workspace_bytes(K.pad32(cin), K.pad32(cout), N, H, W, KH, 128))
    nrange = (N * H * W + 127) // 128
    assert nb >= nrange * KH * 3 * K.pad32(cout) * K.pad32(cin) * 4
    if planes == (2, 16, 16, 3):
        assert nrange == 4
    ws = torch.empty((nb,), dtype=torch.uint8, device=DEV)
    dwp = torch.full((KH * 3, K.pad32(cout), K.pad32(cin)), SENT, device=DEV)
    args = (K.p(xd), cin, xd.shape[-1], K.pad32(cin), K.p(gd), cout, gd.shape[-1], K.pad32(cout), K.p(dwp), None, N, H, W, KH,
            128, K.p(ws))
    with pytest.raises(_lib.DlcsError, match="workspace too small"):
        _lib.call("dlcs_conv2d_k3_wgrad", *args, nb - 1, K.S())
    assert bool((dwp == SENT).all())


# ---------------------------------------------------------------------------- unsupported sizes
@pytest.mark.parametrize("planes,cin,cout", [((2, 17, 4, 3), 8, 8), ((2, 4, 17, 3), 8, 8), ((2, 1, 257, 1), 8, 8),
                                             ((2, 4, 4, 3), 257, 8), ((2, 4, 4, 3), 8, 257)])
def test_unsupported_sizes(planes, cin, cout):
    """Beyond the documented limits every entry raises NotImplementedError (the "unsupported size"
    status) before any launch: the sentinel-filled outputs are untouched."""
    K = _K()
    N, H, W, KH = planes
    rows = N * H * W
    x = torch.zeros((rows, _ld(cin)), dtype=BF16, device=DEV)
    g = torch.zeros((rows, _ld(cout)), dtype=BF16, device=DEV)
    wp = torch.zeros((KH * 3, K.pad32(cout), K.pad32(cin)), dtype=BF16, device=DEV)
    out = torch.full((rows, _ld(cout)), SENT, dtype=BF16, device=DEV)
    with pytest.raises(NotImplementedError):
        K.conv2d(x, cin, wp, cout, _ld(cout), planes, out=out)
    dwp = torch.full((KH * 3, K.pad32(cout), K.pad32(cin)), SENT, device=DEV)
    db = torch.full((cout,), SENT, device=DEV)
    with pytest.raises(NotImplementedError):
        K.conv2d_wgrad(x, cin, g, cout, planes, dwp, dbias=db)
    torch.cuda.synchronize()
    assert bool((out.float() == torch.tensor(SENT).to(BF16).float()).all())
    assert bool((dwp == SENT).all()) and bool((db == SENT).all())
    if max(cin, cout) > 256:
        w = torch.zeros((cout, cin, 3, 3) if KH == 3 else (cout, cin, 3), device=DEV)
        with pytest.raises(NotImplementedError):
            K.conv2d_pack(w, 0)
        with pytest.raises(NotImplementedError):
            K.conv2d_unpack_grad(dwp, w, cout, cin)
        assert bool((w == 0).all())


# ---------------------------------------------------------------------------- pack / unpack
@pytest.mark.parametrize("KH", [3, 1])
@pytest.mark.parametrize("mode", [0, 1])
def test_pack_unpack_round_trip(KH, mode):
    K = _K()
    cout, cin = 12, 40
    T = KH * 3
    w = _weight(cout, cin, KH, 21)
    wp = K.conv2d_pack(w.to(DEV), mode).float().cpu()
    wq = w.to(BF16).float().reshape(cout, cin, T)
    exp = torch.zeros((T, 32, 64) if mode == 0 else (T, 64, 32))
    if mode == 0:
        exp[:, :cout, :cin] = wq.permute(2, 0, 1)
    else:
        exp[:, :cin, :cout] = wq.flip(2).permute(2, 1, 0)
    assert torch.equal(wp, exp)
    # unpack reads the forward layout [tap][cout_pad][cin_pad]: the round trip of mode 0 gives the
    # rounded weight back, that of mode 1 (as the gradient layout of the transposed conv) its flip
    back = torch.full((cin, cout) + tuple(w.shape[2:]), 0.25, device=DEV) if mode else torch.full(tuple(w.shape), 0.25, device=DEV)
    K.conv2d_unpack_grad(wp.to(DEV), back, *((cin, cout) if mode else (cout, cin)))
    want = wq.reshape(w.shape) if mode == 0 else wq.flip(2).permute(1, 0, 2).reshape(back.shape)
    assert torch.equal(back.cpu(), want + 0.25)
    K.conv2d_unpack_grad(wp.to(DEV), back, *((cin, cout) if mode else (cout, cin)), accumulate=0)
    assert torch.equal(back.cpu(), want)
