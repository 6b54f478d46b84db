"""Work skipped on the cropped pad frames of the time axis (fp32 split path, C = 160).

The network pads T circularly and crops the pad after the final conv, so the crop's gradient is
exactly zero on the pad frames and each k3 input gradient widens the non-zero band by one frame
per side.  The weight gradients take that band as a live-frame window and skip the rest; the
final conv's forward computes only the 4-frame slabs the crop reads.  Inputs and budget as
tests/test_gpu_kernels.py: a gradient-sized g (~1e-7), NRMSE <= 2e-6 against a float64
F.conv3d backward."""
import functools

import pytest
import torch
import torch.nn.functional as F

from goldutil import nrmse
from oracle import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = 160
TOL = 2e-6


def _K():
    from dl_cs.models import _ops as K
    return K


def _rnd(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g)


def _to_blocked(x):
    """[B, C, D, H, W] -> blocked rows [B*D*H*W, C] (layout.hip)."""
    B, Cc, D, H, W = x.shape
    t = x.permute(0, 2, 3, 4, 1).reshape(B, D // 4, 4, H // 4, 4, W // 4, 4, Cc)
    return t.permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(-1, Cc)


def _from_blocked(r, B, Cc, D, H, W):
    t = r.reshape(B, D // 4, H // 4, W // 4, 4, 4, 4, Cc).permute(0, 1, 4, 2, 5, 3, 6, 7)
    return t.reshape(B, D, H, W, Cc).permute(0, 4, 1, 2, 3)


def _windowed(g, win):
    """g [B, C, D, H, W] with the frames outside [t_lo, t_hi) zeroed."""
    z = torch.zeros_like(g)
    z[:, :, win[0]:win[1]] = g[:, :, win[0]:win[1]]
    return z


# ---------------------------------------------------------------- 160 -> 160 weight gradient
# (grid, window): each pair chosen for a join of the live-unit sequence
WG_CASES = [
    ((1, 12, 8, 8), (3, 9)),       # one half -> two halves -> one half
    ((1, 12, 8, 8), (2, 10)),
    ((1, 8, 8, 8), (3, 5)),        # no interior slab: slab 0's second half, then slab 1's first
    ((1, 4, 8, 8), (1, 3)),        # a single slab, both halves live
    ((2, 8, 12, 20), (3, 5)),      # two batch items, odd patch count in y, more ranges
    ((1, 16, 8, 8), (6, 10)),      # a whole dead slab at each end (pad = 6)
]


@functools.lru_cache(maxsize=None)
def _wg_inputs(grid):
    B, D, H, W = grid
    x = _rnd((B, C, D, H, W), 41)
    g = _rnd((B, C, D, H, W), 44) * 1e-7
    return x, g


def _wg_reference(grid, win):
    x, g = _wg_inputs(grid)
    w_ = torch.zeros((C, C, 3, 3, 3), dtype=torch.float64).requires_grad_()
    F.conv3d(x.double(), w_, None, padding=1).backward(_windowed(g, win).double())
    return w_.grad


def _wg_planes(grid, win=None):
    """Planes of x and of g.  With a window, g keeps its values on every frame the kernel must
    not read (the dead two-frame units) and is zero, as the caller promises, on the frames
    outside the window that share a live unit with a frame inside it (an odd t_lo or t_hi)."""
    K = _K()
    x, g = _wg_inputs(grid)
    if win is not None:
        g = g.clone()
        g[:, :, win[0] // 2 * 2:win[0]] = 0
        g[:, :, win[1]:(win[1] + 1) // 2 * 2] = 0
    return K.split2(_to_blocked(x).to(DEV)), K.split2(_to_blocked(g).to(DEV))


@pytest.mark.parametrize("grid,win", WG_CASES)
def test_wgrad_f16x3_window(grid, win):
    """The windowed weight gradient equals the float64 gradient of g zeroed outside the window,
    while the kernel's g keeps its values on the dead units: those rows are not read (and the
    plane scale still comes from the whole tensor).  The kernel skips whole two-frame units, so
    a frame outside an odd-ended window that shares a unit with a frame inside is read, and must
    be zero as the caller promises (_wg_planes)."""
    K = _K()
    px, pg = _wg_planes(grid, win)
    dwp = torch.zeros((27, C, C), device=DEV)
    K.conv3d_wgrad_f16x3(px, pg, grid, dwp, live=win)
    gw = torch.zeros((C, C, 3, 3, 3), device=DEV)
    K.conv_unpack_grad(dwp, gw, C, C)
    err = nrmse(_wg_reference(grid, win).numpy(), gw.cpu().double().numpy())
    print(f"wgrad f16x3 {grid} window {win}: NRMSE {err:.3e}")
    assert err < TOL
    # run-to-run deterministic, and accumulating into dW
    dwp2 = torch.full((27, C, C), 0.5, device=DEV)
    K.conv3d_wgrad_f16x3(px, pg, grid, dwp2, live=win)
    assert torch.equal(dwp2, dwp + 0.5)
    dwp3 = torch.zeros((27, C, C), device=DEV)
    K.conv3d_wgrad_f16x3(px, pg, grid, dwp3, live=win)
    assert torch.equal(dwp3, dwp)


def test_wgrad_f16x3_window_edges():
    """An empty window leaves dW untouched; the full window is the un-windowed call bit for bit."""
    K = _K()
    grid = (1, 12, 8, 8)
    px, pg = _wg_planes(grid)
    pre = _rnd((27, C, C), 45).to(DEV)
    for win in [(5, 5), (7, 3), (12, 12), (0, 0)]:
        dwp = pre.clone()
        K.conv3d_wgrad_f16x3(px, pg, grid, dwp, live=win)
        assert torch.equal(dwp, pre), win
    plain = torch.zeros((27, C, C), device=DEV)
    K.conv3d_wgrad_f16x3(px, pg, grid, plain)
    for win in [(0, 12), (-3, 40)]:
        dwp = torch.zeros((27, C, C), device=DEV)
        K.conv3d_wgrad_f16x3(px, pg, grid, dwp, live=win)
        assert torch.equal(dwp, plain), win


# ---------------------------------------------------------------- thin final conv
THIN_GRIDS = [(1, 12, 8, 12), (2, 8, 12, 20)]


@functools.lru_cache(maxsize=None)
def _thin_inputs(grid):
    B, D, H, W = grid
    e = 4
    x160 = _rnd((B, C, D, H, W), 81)
    w_fin = _rnd((e, C, 3, 3, 3), 83) / (27 * C) ** 0.5
    b4 = _rnd((e,), 85)
    g4 = _rnd((B, e, D, H, W), 89) * 1e-7
    return x160, w_fin, b4, g4


@pytest.mark.parametrize("grid,slabs", [(THIN_GRIDS[0], (1, 2)), (THIN_GRIDS[1], (0, 1))])
def test_thin_out_slab_window(grid, slabs):
    """Final conv forward on a slab window: the rows of the window's slabs match float64, every
    other row (and the columns past the four channels) keeps a sentinel prefill bit for bit."""
    K = _K()
    B, D, H, W = grid
    e, rows = 4, B * D * H * W
    x160, w_fin, b4, _ = _thin_inputs(grid)
    px = K.split2(_to_blocked(x160).to(DEV))
    wo = K.thin_pack_f16x3(K.conv_pack(w_fin.to(DEV), torch.float32, 0), e, C, 1)
    sentinel = 1234.5
    o = torch.full((rows, 8), sentinel, device=DEV)
    K.conv3d_thin_out_planes(px, wo, e, 8, grid, bias=b4.to(DEV), out=o, slabs=slabs)
    ref = F.conv3d(x160.double(), w_fin.double(), b4.double(), padding=1)
    oc = o.cpu()
    got = _from_blocked(oc[:, :e], B, e, D, H, W)
    f0, f1 = 4 * slabs[0], 4 * slabs[1]
    err = nrmse(ref[:, :, f0:f1].numpy(), got[:, :, f0:f1].double().numpy())
    print(f"thin out {grid} slabs {slabs}: NRMSE {err:.3e}")
    assert err < TOL
    outside = torch.ones(D, dtype=torch.bool)
    outside[f0:f1] = False
    assert torch.equal(got[:, :, outside], torch.full_like(got[:, :, outside], sentinel))
    assert torch.equal(oc[:, e:], torch.full_like(oc[:, e:], sentinel))
    # the whole range of slabs is the un-windowed call
    o_all = torch.full((rows, 8), sentinel, device=DEV)
    K.conv3d_thin_out_planes(px, wo, e, 8, grid, bias=b4.to(DEV), out=o_all, slabs=(0, D // 4))
    o_ref = torch.full((rows, 8), sentinel, device=DEV)
    K.conv3d_thin_out_planes(px, wo, e, 8, grid, bias=b4.to(DEV), out=o_ref)
    assert torch.equal(o_all, o_ref)
    assert torch.equal(got[:, :, f0:f1], _from_blocked(o_ref.cpu()[:, :e], B, e, D, H, W)[:, :, f0:f1])


def _live_slab(t, win, D):
    """Slab t is live for the thin weight gradient iff its frames widened by the tap halo meet the window."""
    return max(4 * t - 1, win[0], 0) < min(4 * t + 5, win[1], D)


@pytest.mark.parametrize("grid,win", [
    (THIN_GRIDS[0], (5, 7)),       # slab 1 alone: slabs 0 and 2 are dead
    (THIN_GRIDS[0], (4, 8)),       # frames 4 and 7 reach slabs 0 and 2 through the halo: all live
    (THIN_GRIDS[1], (0, 2)),       # slab 0 of both batch items, slab 1 dead
    (THIN_GRIDS[1], (1, 4)),       # frame 3 reaches slab 1 through the halo: all live
])
def test_thin_wgrad_frame_window(grid, win):
    """Final conv weight gradient with g zero outside the window: float64 budget, run-to-run
    deterministic; the dead slabs' rows of the 160-channel planes are poisoned with NaN, so a
    finite result shows they are not read."""
    K = _K()
    B, D, H, W = grid
    e, rows = 4, B * D * H * W
    x160, w_fin, _, g4 = _thin_inputs(grid)
    gz = _windowed(g4, win)
    px = K.split2(_to_blocked(x160).to(DEV))
    dead = torch.tensor([not _live_slab(t, win, D) for t in range(D // 4)])
    if dead.any():
        pl = px[:rows * 640].view(torch.float16).view(B, D // 4, (H // 4) * (W // 4) * 64, 320)
        pl[:, dead.to(DEV)] = float("nan")
    gd = torch.full((rows, 8), float("nan"))
    gd[:, :e] = _to_blocked(gz)
    gd = gd.to(DEV)
    gmax = K.absmax(_to_blocked(gz).to(DEV))
    dwp = torch.zeros((27, K.pad32(e), C), device=DEV)
    K.conv3d_thin_wgrad_planes(px, gd, e, gmax, 0, grid, dwp, live=win)
    gw = torch.zeros((e, C, 3, 3, 3), device=DEV)
    K.conv_unpack_grad(dwp, gw, e, C)
    w_ = w_fin.double().requires_grad_()
    F.conv3d(x160.double(), w_, None, padding=1).backward(gz.double())
    err = nrmse(w_.grad.numpy(), gw.cpu().double().numpy())
    print(f"thin wgrad {grid} window {win} (dead slabs {dead.tolist()}): NRMSE {err:.3e}")
    assert err < TOL
    dwp2 = torch.zeros_like(dwp)
    K.conv3d_thin_wgrad_planes(px, gd, e, gmax, 0, grid, dwp2, live=win)
    assert torch.equal(dwp, dwp2)


def test_thin_wgrad_window_edges():
    """Empty window: dW untouched; full window: the un-windowed call bit for bit."""
    K = _K()
    grid = THIN_GRIDS[0]
    B, D, H, W = grid
    e, rows = 4, B * D * H * W
    x160, _, _, g4 = _thin_inputs(grid)
    px = K.split2(_to_blocked(x160).to(DEV))
    gd = torch.zeros((rows, 8))
    gd[:, :e] = _to_blocked(g4)
    gd = gd.to(DEV)
    gmax = K.absmax(gd)
    pre = _rnd((27, K.pad32(e), C), 46).to(DEV)
    dwp = pre.clone()
    K.conv3d_thin_wgrad_planes(px, gd, e, gmax, 0, grid, dwp, live=(6, 6))
    assert torch.equal(dwp, pre)
    plain = torch.zeros_like(pre)
    K.conv3d_thin_wgrad_planes(px, gd, e, gmax, 0, grid, plain)
    full = torch.zeros_like(pre)
    K.conv3d_thin_wgrad_planes(px, gd, e, gmax, 0, grid, full, live=(0, D))
    assert torch.equal(full, plain)


# ---------------------------------------------------------------- engine
def test_swinnet_windows_change_nothing_read(monkeypatch):
    """One SwinNet forward + backward on the split path (fp32, C = 160, T = 4 so D = 12 with
    pad = 4), as built and with the window arguments stripped from the K.* wrappers: output and
    dL/dx bit-identical (the forward only drops rows nothing reads; dL/dx does not pass through
    a weight gradient), every parameter gradient within the fp32 kernel budget of the other run."""
    from dl_cs.models import _ops as K
    from dl_cs.models import swin3D
    old = swin3D.get_compute_dtype()
    swin3D.set_compute_dtype(torch.float32)
    try:
        net = swin3D.SwinTransformer3DNet(num_swinblocks=1, in_chans=4, chans=C, kernel_size=3, window_size=(4, 4))
        net.eval()
        recipe.fill_module(net, 31)
        net = net.to(DEV)
        xin = recipe.crandn(32, (1, 2, 4, 16, 16)).to(DEV)
        gr = recipe.crandn(33, (1, 2, 4, 16, 16)).to(DEV)

        def run():
            net.zero_grad(set_to_none=True)
            x = xin.clone().requires_grad_()
            y = net(x)
            (y.real * gr.real + y.imag * gr.imag).sum().backward()
            return y.detach().clone(), x.grad.clone(), {n: p.grad.clone() for n, p in net.named_parameters()
                                                        if p.grad is not None}

        seen = []
        wg, to, tw = K.conv3d_wgrad_f16x3, K.conv3d_thin_out_planes, K.conv3d_thin_wgrad_planes

        def spy(fn, key):
            def f(*a, **kw):
                seen.append((key, kw.get(key)))
                return fn(*a, **kw)
            return f
        monkeypatch.setattr(K, "conv3d_wgrad_f16x3", spy(wg, "live"))
        monkeypatch.setattr(K, "conv3d_thin_out_planes", spy(to, "slabs"))
        monkeypatch.setattr(K, "conv3d_thin_wgrad_planes", spy(tw, "live"))
        y1, dx1, g1 = run()
        # D = 12, pad = 4: final conv slab 1; go on [4, 8), g_h on [3, 9), g_out on [2, 10)
        assert ("slabs", (1, 2)) in seen
        assert [v for k, v in seen if k == "live"] == [(4, 8), (3, 9), (2, 10), None]

        def strip(fn, key):
            def f(*a, **kw):
                kw.pop(key, None)
                return fn(*a, **kw)
            return f
        monkeypatch.setattr(K, "conv3d_wgrad_f16x3", strip(wg, "live"))
        monkeypatch.setattr(K, "conv3d_thin_out_planes", strip(to, "slabs"))
        monkeypatch.setattr(K, "conv3d_thin_wgrad_planes", strip(tw, "live"))
        y0, dx0, g0 = run()
    finally:
        swin3D.set_compute_dtype(old)
    assert torch.equal(y1, y0)
    assert torch.equal(dx1, dx0)
    assert g1.keys() == g0.keys() and len(g1) > 0
    for n in g1:
        err = nrmse(g0[n].cpu().numpy(), g1[n].cpu().numpy())
        assert err < TOL, (n, err)
