"""2-D ResNet on the spatial basis L of the DSLR family (r2d = dl_cs/models/resnet2d.py),
MI355X build.

Same classes, constructor arguments and state_dict keys as the reference (r2d:108-263):
init ConvBlock (no activation), num_resblocks ResBlocks, final pre-activation ConvBlock
back to in_chans, plus the input residual, with nn.ReLU(inplace=True) pre-activations
(r2d:45, :173-195, :258) -- the in-place-ReLU algebra of resnet3d:

    u  = cat(re, im)                       r2d:225-231
    r0 = relu(conv0(u))
    t  = relu(conv_a(r_k)) ;  r_{k+1} = relu(conv_b(t) + r_k)
    out = conv_f(r_L) + u                  r2d:258

The network runs as one HIP autograd node on the generic Conv3d k3 kernels
(dlcs_conv3d_k3 / dlcs_conv3d_k3_wgrad): the N blocks [N, C, b, b] become the depth
planes of one (1, N rounded up to 4, b, b) grid and every 3 x 3 weight sits in the
centre depth tap of a 27-tap weight whose other 18 taps are zero, so planes do not mix
and the H, W border is the conv's own zero padding.  The weight gradients are the
centre-tap slices of the 27-tap gradient.  The zero taps cost 3x the multiplies of a
2-D kernel (9x for the 1-D net, resnet1d.py, which embeds along W the same way).

`embedded_forward` / `embedded_backward` take a real [1, C, D, H, W] tensor and the
embedding; resnet1d.py reuses them.

Compute dtype bf16 (swin3D.set_compute_dtype) runs the same algebra as a second node,
_PlaneFn, on the plane conv (dlcs_conv2d_k3 / dlcs_conv2d_k3_wgrad, csrc/conv2d.hip): the
blocks are independent planes of channels-last rows [N b b, ld], any b <= 16, 9 taps (3 for
the 1-D net) instead of 27.  r, t and every feature-width gradient are stored in bf16; the
convs accumulate in fp32, add bias and residual in fp32 and round once.  Weights, weight and
bias gradients, u, the final conv's output, the init dgrad's output and the complex boundary
stay fp32, and so do the two residuals that cross the boundary (+ u forward, + go backward).
The weight and bias gradients are summed in a fixed order: two runs give the same bits.
"""
import torch
from torch import nn

from . import _ops as K
from ._standalone import to_blocked, from_blocked
from .resnet3d import _conv, _dgrad
from .swin3D import get_compute_dtype


def _pad4(n):
    return (n + 3) // 4 * 4


def _pad8(n):
    return (n + 7) // 8 * 8


def _wgrad(x, cin, g, cout, grid, gw, gb, rows):
    """resnet3d._wgrad with the weight-gradient kernel's voxel range per workgroup sized for
    these grids: they hold 1e4-1e5 voxels (a Swin slice: 1e6), and at the default 16384 voxels
    per workgroup the launch would be 2 to 9 ranges x 27 taps on 256 CUs.  About 64 ranges."""
    vox = min(16384, max(512, (rows // 64 + 63) // 64 * 64))
    dwp = torch.zeros((27, K.pad32(cout), K.pad32(cin)), dtype=torch.float32, device=x.device)
    K.conv3d_wgrad(x, cin, 0, g, cout, grid, dwp, vox_per_block=vox)
    K.conv_unpack_grad(dwp, gw, cout, cin)
    K.colsum(g, gb, rows=rows, C=cout, ld=g.shape[-1])


class _Identity(nn.Module):
    """Normalization 'none' (r2d:12-32) and Activation (r2d:35-55) placeholders: they hold
    the reference's positions in ConvBlock.layers; the fused node applies the ReLUs."""

    def __init__(self, type):
        super().__init__()
        self.type = type


class _Conv(nn.Module):
    """r2d:58-71 -- holds the torch conv (weights, default init); the fused node reads them."""

    def __init__(self, conv):
        super().__init__()
        self.conv = conv


class ConvBlock(nn.Module):
    """r2d:108-156 -- Norm -> Act -> Conv (pre-activation)."""
    NAME, CONV = 'Conv2D', nn.Conv2d

    def __init__(self, in_chans, out_chans, kernel_size, act_type='relu', norm_type='none', is_complex=False):
        super().__init__()
        if is_complex:
            raise NotImplementedError("dl_cs HIP DSLR: COMPLEX: False (configs/config_dslr.yaml)")
        if norm_type != 'none' or act_type not in ('relu', 'none'):
            raise NotImplementedError("dl_cs HIP DSLR: norm 'none', activation relu / none")
        self.in_chans, self.out_chans, self.is_complex, self.name = in_chans, out_chans, is_complex, self.NAME
        conv = self.CONV(in_chans, out_chans, kernel_size, padding=(kernel_size - 1) // 2)
        self.layers = nn.Sequential(_Identity(norm_type), _Identity(act_type), _Conv(conv))

    def forward(self, input):
        raise NotImplementedError("dl_cs: ConvBlock runs inside ResNet's fused HIP node")

    def __repr__(self):
        return f'{self.name}(in_chans={self.in_chans}, out_chans={self.out_chans})'


class ResBlock(nn.Module):
    """r2d:159-195 -- two pre-activation ConvBlocks and a residual connection."""
    BLOCK = ConvBlock

    def __init__(self, in_chans, out_chans, kernel_size, is_complex=False):
        super().__init__()
        assert in_chans == out_chans                              # the ResNet never resamples (r2d:220)
        self.layers = nn.Sequential(self.BLOCK(in_chans, out_chans, kernel_size, act_type='relu', is_complex=is_complex),
                                    self.BLOCK(out_chans, out_chans, kernel_size, act_type='relu', is_complex=is_complex))
        self.resample = nn.Identity()

    def forward(self, input):
        raise NotImplementedError("dl_cs: ResBlock runs inside ResNet's fused HIP node")


# ------------------------------------------------------------------ the fused node
def embedded_forward(P, names, x, embed):
    """x fp32 [1, C, D, H, W] -> (out of the same shape, saved).  embed(w) places a 2-D or
    1-D weight in a zero [cout, cin, 3, 3, 3] weight."""
    _, C, D, H, W = x.shape
    grid = (1, _pad4(D), _pad4(H), _pad4(W))
    ld = _pad8(C)
    F = P[names["init_w"]].shape[0]
    u = to_blocked(x, ld, torch.float32)
    r = [_conv(u, C, embed(P[names["init_w"]]), F, F, grid, bias=P[names["init_b"]], relu_out=1)]
    ts = []
    for wa, ba, wb, bb in names["blocks"]:
        t = _conv(r[-1], F, embed(P[wa]), F, F, grid, bias=P[ba], relu_out=1)
        ts.append(t)
        r.append(_conv(t, F, embed(P[wb]), F, F, grid, bias=P[bb], res=r[-1], relu_out=1))
    o = _conv(r[-1], F, embed(P[names["final_w"]]), C, ld, grid, bias=P[names["final_b"]], res=u,
              out_dtype=torch.float32)
    return from_blocked(o, tuple(x.shape)), dict(u=u, r=r, ts=ts, grid=grid, C=C, F=F, ld=ld, shape=tuple(x.shape))


def embedded_backward(P, names, sv, gout, grads, embed, centre):
    """Backward of embedded_forward (resnet3d.resnet_backward's algebra); grads[name] +=
    centre(27-tap gradient) for the weights, the column sums for the biases."""
    grid, C, F, ld = sv["grid"], sv["C"], sv["F"], sv["ld"]
    rows = grid[0] * grid[1] * grid[2] * grid[3]
    r, ts, u = sv["r"], sv["ts"], sv["u"]

    def wgrad(x, cin, g, cout, wname, bname):
        g3 = torch.zeros((cout, cin, 3, 3, 3), dtype=torch.float32, device=g.device)
        _wgrad(x, cin, g, cout, grid, g3, grads[bname], rows)
        grads[wname] += centre(g3)

    go = to_blocked(gout.contiguous(), ld, torch.float32)                           # dL/d out (and the + u path)
    wgrad(r[-1], F, go, C, names["final_w"], names["final_b"])
    g = _dgrad(go, C, embed(P[names["final_w"]]), F, F, grid, mask=r[-1])           # dL/d o_L (through relu)
    for k in reversed(range(len(ts))):
        wa, ba, wb, bb = names["blocks"][k]
        wgrad(ts[k], F, g, F, wb, bb)
        gt = _dgrad(g, F, embed(P[wb]), F, F, grid, mask=ts[k])
        wgrad(r[k], F, gt, F, wa, ba)
        gr = _dgrad(gt, F, embed(P[wa]), F, F, grid, res=g)                         # dL/d r_k (conv + residual)
        g = K.relu_grad(gr, r[k])                                                   # dL/d o_k
    wgrad(u, C, g, F, names["init_w"], names["init_b"])
    du = _dgrad(g, F, embed(P[names["init_w"]]), C, ld, grid, res=go, out_dtype=torch.float32)
    return from_blocked(du, sv["shape"])


# ------------------------------------------------------------------ the bf16 node (plane conv)
def _to_rows(x, ld):
    """fp32 [N, C, H, W] -> channels-last rows [N H W, ld] (zero slack columns)."""
    N, C, H, W = x.shape
    rows = torch.zeros((N * H * W, ld), dtype=torch.float32, device=x.device)
    rows.view(N, H, W, ld)[..., :C] = x.permute(0, 2, 3, 1)
    return rows


def _from_rows(rows, shape):
    N, C, H, W = shape
    return rows.view(N, H, W, rows.shape[-1])[..., :C].permute(0, 3, 1, 2).contiguous()


def _wgrad_pix(rows):
    """Pixel range per workgroup of the plane conv's weight gradient: about 48 ranges (each
    is a launch of KH 3 workgroups per 128 output channels and one partial slab to add)."""
    return min(16384, max(256, (rows // 48 + 63) // 64 * 64))


def plane_forward(P, names, x, KH):
    """x fp32 [N, C, H, W] (KH 3: N planes) or [N, C, 1, W] (KH 1: N sequences) -> (out, saved)."""
    N, C, H, W = x.shape
    planes = (N, H, W, KH)
    ld = _pad8(C)
    F = P[names["init_w"]].shape[0]
    Fld = _pad8(F)
    u32 = _to_rows(x, ld)                                     # the input residual is added unrounded
    u = K.cast(u32, torch.bfloat16)
    conv = lambda a, cin, w, cout, out_ld, **kw: K.conv2d(a, cin, K.conv2d_pack(P[w], 0), cout, out_ld, planes, **kw)
    r = [conv(u, C, names["init_w"], F, Fld, bias=P[names["init_b"]], relu_out=1)]
    ts = []
    for wa, ba, wb, bb in names["blocks"]:
        t = conv(r[-1], F, wa, F, Fld, bias=P[ba], relu_out=1)
        ts.append(t)
        r.append(conv(t, F, wb, F, Fld, bias=P[bb], res=r[-1], relu_out=1))
    o = conv(r[-1], F, names["final_w"], C, ld, bias=P[names["final_b"]], res=u32, out_dtype=torch.float32)
    return _from_rows(o, tuple(x.shape)), dict(u=u, r=r, ts=ts, planes=planes, C=C, F=F, ld=ld, Fld=Fld,
                                               shape=tuple(x.shape))


def plane_backward(P, names, sv, gout, grads):
    """Backward of plane_forward; grads[name] += the weight and bias gradients (fp32)."""
    planes, C, F, ld, Fld = sv["planes"], sv["C"], sv["F"], sv["ld"], sv["Fld"]
    rows = planes[0] * planes[1] * planes[2]
    r, ts, u = sv["r"], sv["ts"], sv["u"]
    pix = _wgrad_pix(rows)

    def wgrad(x, cin, g, cout, wname, bname):
        dwp = torch.zeros((planes[3] * 3, K.pad32(cout), K.pad32(cin)), dtype=torch.float32, device=g.device)
        K.conv2d_wgrad(x, cin, g, cout, planes, dwp, pix_per_block=pix, dbias=grads[bname])
        K.conv2d_unpack_grad(dwp, grads[wname], cout, cin)

    dgrad = lambda g, cout_w, w, cin_w, out_ld, **kw: K.conv2d(g, cout_w, K.conv2d_pack(P[w], 1), cin_w, out_ld, planes, **kw)
    go32 = _to_rows(gout, ld)                                                       # the + u path, unrounded
    go = K.cast(go32, torch.bfloat16)
    wgrad(r[-1], F, go, C, names["final_w"], names["final_b"])
    g = dgrad(go, C, names["final_w"], F, Fld, mask=r[-1])                          # dL/d o_L (through relu)
    for k in reversed(range(len(ts))):
        wa, ba, wb, bb = names["blocks"][k]
        wgrad(ts[k], F, g, F, wb, bb)
        gt = dgrad(g, F, wb, F, Fld, mask=ts[k])
        wgrad(r[k], F, gt, F, wa, ba)
        g = dgrad(gt, F, wa, F, Fld, res=g, mask=None)                              # dL/d r_k (conv + residual)
        g = K.relu_grad(g, r[k])                                                    # dL/d o_k
    wgrad(u, C, g, F, names["init_w"], names["init_b"])
    du = dgrad(g, F, names["init_w"], C, ld, res=go32, out_dtype=torch.float32)
    return _from_rows(du, sv["shape"])


class _PlaneFn(torch.autograd.Function):
    """One node per network call in compute dtype bf16: x fp32 [N, C, H, W]."""

    @staticmethod
    def forward(ctx, x, meta, *plist):
        P = dict(zip(meta["order"], plist))
        out, sv = plane_forward(P, meta["names"], x.to(torch.float32), meta["KH"])
        ctx.state = (P, sv, meta)
        return out

    @staticmethod
    def backward(ctx, gout):
        P, sv, meta = ctx.state
        grads = {n: torch.zeros_like(p) for n, p in P.items()}
        gx = plane_backward(P, meta["names"], sv, gout.to(torch.float32), grads)
        ctx.state = None
        return (gx, None) + tuple(grads[n] for n in meta["order"])


class _EmbeddedFn(torch.autograd.Function):
    """One node per network call: x fp32 [1, C, D, H, W]."""

    @staticmethod
    def forward(ctx, x, meta, *plist):
        P = dict(zip(meta["order"], plist))
        out, sv = embedded_forward(P, meta["names"], x.to(torch.float32), meta["embed"])
        ctx.state = (P, sv, meta)
        return out

    @staticmethod
    def backward(ctx, gout):
        P, sv, meta = ctx.state
        grads = {n: torch.zeros_like(p) for n, p in P.items()}
        gx = embedded_backward(P, meta["names"], sv, gout.to(torch.float32), grads, meta["embed"], meta["centre"])
        ctx.state = None
        return (gx, None) + tuple(grads[n] for n in meta["order"])


def _embed_hw(w):
    """[cout, cin, 3, 3] -> [cout, cin, 3, 3, 3] with the weight in the centre depth tap."""
    w3 = torch.zeros(w.shape[:2] + (3, 3, 3), dtype=w.dtype, device=w.device)
    w3[:, :, 1] = w
    return w3


class ResNet(nn.Module):
    """r2d:198-263 -- the 2-D ResNet: complex [N, C, b, b] -> the same shape."""
    NAME, BLOCK, RES = "ResNet2D", ConvBlock, ResBlock
    EMBED = staticmethod(_embed_hw)
    CENTRE = staticmethod(lambda g3: g3[:, :, 1])
    KH = 3             # tap rows of the plane conv (the bf16 node)

    def __init__(self, num_resblocks, in_chans, chans, kernel_size, use_complex_layers=False, circular_pad=False):
        super().__init__()
        if use_complex_layers:
            raise NotImplementedError(f"dl_cs HIP {self.NAME}: COMPLEX: False (configs/config_dslr.yaml)")
        if kernel_size != 3:
            raise NotImplementedError(f"dl_cs HIP {self.NAME}: kernel size 3 (dlcs_conv3d_k3)")
        self.use_complex_layers = use_complex_layers
        self.circular_pad = circular_pad
        self.pad_size = (2 * num_resblocks + 2) * (kernel_size - 1) // 2           # r2d:211
        self.init_layer = self.BLOCK(in_chans, chans, kernel_size, act_type='none')
        self.res_blocks = nn.ModuleList([self.RES(chans, chans, kernel_size) for _ in range(num_resblocks)])
        self.final_layer = self.BLOCK(chans, in_chans, kernel_size, act_type='relu')

    def _run(self, x):
        """x through the fused node of the compute dtype: fp32 [1, C, D, H, W] (the embedding),
        bf16 [N, C, H, W] (planes; the 1-D net passes [N, C, 1, T'])."""
        dtype = get_compute_dtype()
        if dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError(f"dl_cs HIP {self.NAME}: compute dtype float32 or bfloat16 (got {dtype})")
        if not x.is_cuda:
            raise RuntimeError(f"dl_cs HIP {self.NAME} needs GPU tensors (no CPU fallback in the product path)")
        params = dict(self.named_parameters())
        order = list(params.keys())
        c = lambda pre: (f"{pre}.layers.2.conv.weight", f"{pre}.layers.2.conv.bias")
        (iw, ib), (fw, fb) = c("init_layer"), c("final_layer")
        blocks = [c(f"res_blocks.{k}.layers.0") + c(f"res_blocks.{k}.layers.1") for k in range(len(self.res_blocks))]
        names = dict(init_w=iw, init_b=ib, final_w=fw, final_b=fb, blocks=blocks)
        if dtype == torch.bfloat16:
            meta = dict(order=order, names=names, KH=self.KH)
            return _PlaneFn.apply(x, meta, *[params[n] for n in order])
        meta = dict(order=order, names=names, embed=self.EMBED, centre=self.CENTRE)
        return _EmbeddedFn.apply(x, meta, *[params[n] for n in order])

    def forward(self, input):
        """input complex64 [N, C, b, b] -> the same shape (fp32: b a multiple of 4; bf16: any b <= 16)."""
        N, C, H, W = input.shape
        if get_compute_dtype() == torch.bfloat16:
            u = torch.cat((input.real, input.imag), dim=1)
            o = self._run(u)
            return torch.complex(o[:, :C].contiguous(), o[:, C:].contiguous())
        if H % 4 or W % 4:
            raise NotImplementedError(f"dl_cs HIP {self.NAME}: block size a multiple of 4 (the conv grid)")
        u = torch.cat((input.real, input.imag), dim=1)                              # r2d:225-231
        o = self._run(u.permute(1, 0, 2, 3).unsqueeze(0))[0].permute(1, 0, 2, 3)    # blocks = depth planes
        return torch.complex(o[:, :C].contiguous(), o[:, C:].contiguous())          # r2d:233-240
