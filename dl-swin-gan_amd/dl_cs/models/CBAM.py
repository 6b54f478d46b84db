"""CBAM 3D ResNet regularizer (MODEL_TYPE 'CBAM') of the reference's unrolledCBAM
network, MI355X build.

Same classes, constructor arguments and state_dict keys as the reference
(CBAM = dl_cs/models/CBAM.py:60-134, 371-521, 565-639).  The conv trunk is resnet3d's
fused node, the channel gate (CABlock: the max-pool branch is commented out in the
reference, CBAM:411,421) is se3d's on the dlcs_se_* kernels, and the spatial gate
(SABlock: mean over channels -> Conv3d(1, 1, 5, padding 2), no sigmoid, no max map)
runs on the dlcs_cbam_* kernels (cbam.hip).

As in se3d.py the pre-activation ReLUs are in place (CBAM:491-494 build resnet3d's
ConvBlocks), so a block's residual adds relu(input) and every block output is only
consumed through a ReLU.  With F channels, N = Tp Y X voxels per batch item (time pad
included) and taps outside the grid reading 0:

    o   = conv_b(relu(conv_a(r_k)))
    m   = mean_v o ;  h = relu(W1 m + b1) ;  s = sigmoid(W2 h + b2)        CBAM:518
    a[b, v] = (1 / F) sum_c s[b, c] o[b, v, c]                              map
    q[b, v] = b5 + sum_d w5[d] a[b, v + d]                                  map, CBAM:519
    r_{k+1} = relu(q[b, v] s[b, c] o[b, v, c] + r_k)                        CBAM:521 + the next ReLU

Backward of one block from g = dL/dr_{k+1}, gz = g [r_{k+1} > 0] (also the residual
gradient into r_k):

    dq[b, v] = sum_c gz s[b, c] o[b, v, c]
    db5 += sum dq ;  dw5[d] += sum_{b, v} dq[b, v] a[b, v + d]
    da[b, v] = sum_d w5[d] dq[b, v - d]
    e = gz q[b, v] + da[b, v] / F ;  ds[b, c] = sum_v e o  -> se_gate_bwd -> dm[b, c]
    do = e s[b, c] + dm[b, c]                               conv_b's output gradient
"""
import torch
from torch import nn

from . import _ops as K
from .resnet3d import PAD_CIN, _conv, _dgrad, _wgrad
from .swin3D import Activation, ConvBlock, Conv3d, get_compute_dtype

_FUSED = "dl_cs: runs inside CBAMResNet's fused HIP node"


def _pool_type(type):
    if type not in ('channel', 'spatial'):
        raise ValueError('Invalid type')
    return type


class GlobalMaxPool(nn.Module):
    """CBAM:60-87 -- max over (T, Y, X) ('channel') or over channels ('spatial'); the
    reference constructs it and never calls it."""

    def __init__(self, type):
        super().__init__()
        self.mpool = nn.Identity()
        self.type = _pool_type(type)

    def forward(self, input):
        raise NotImplementedError("dl_cs HIP CBAMResNet: the max-pool branches are disabled in the reference")


class GlobalAvgPool(nn.Module):
    """CBAM:90-117 -- mean over (T, Y, X) ('channel') or over channels ('spatial')."""

    def __init__(self, type):
        super().__init__()
        self.apool = nn.Identity()
        self.type = _pool_type(type)

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class FC(nn.Module):
    """CBAM:120-134 -- nn.Linear."""

    def __init__(self, in_chans, out_chans):
        super().__init__()
        self.fc = nn.Linear(in_chans, out_chans)

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class CABlock(nn.Module):
    """CBAM:371-422 -- GlobalAvgPool -> FC(out_chans, rr) -> ReLU -> FC(rr, out_chans) -> sigmoid."""

    def __init__(self, out_chans, rr, norm_type='none', is_complex=False):
        super().__init__()
        if is_complex:
            raise NotImplementedError("dl_cs HIP CBAMResNet: COMPLEX: False")
        self.is_complex = is_complex
        self.layers = nn.Sequential(FC(out_chans, rr), Activation("relu"), FC(rr, out_chans), Activation("sigmoid"))
        self.avgpool = nn.Sequential(GlobalAvgPool("channel"))

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class SABlock(nn.Module):
    """CBAM:425-475 -- mean over channels -> Conv3d(1, 1, kernel_size=5, padding=2)."""

    def __init__(self, act_type='relu', norm_type='none', is_complex=False):
        super().__init__()
        if is_complex:
            raise NotImplementedError("dl_cs HIP CBAMResNet: COMPLEX: False")
        self.is_complex = is_complex
        self.avgpool = nn.Sequential(GlobalAvgPool("spatial"))
        self.layers = nn.Sequential(Conv3d(in_chans=1, out_chans=1, kernel_size=5))

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class CBAMResBlock(nn.Module):
    """CBAM:477-521 -- two pre-activation ConvBlocks scaled by the channel gate, then by
    the spatial map of the scaled tensor, plus the residual."""

    def __init__(self, chans, kernel_size, rr, act_type='relu', is_complex=False):
        super().__init__()
        self.layers1 = nn.Sequential(
            ConvBlock(chans, chans, kernel_size, act_type=act_type, is_complex=is_complex),
            ConvBlock(chans, chans, kernel_size, act_type=act_type, is_complex=is_complex))
        self.CAmodule = nn.Sequential(CABlock(chans, rr, is_complex=is_complex))
        self.SAmodule = nn.Sequential(SABlock(is_complex=is_complex))

    def forward(self, input):
        raise NotImplementedError(_FUSED)


def cbamresnet_forward(P, names, x, nblocks, pad):
    """x complex64 [B, E, T, Y, X] -> (out complex64, saved)."""
    B, E, T, Y, X = x.shape
    Tp = T + 2 * pad
    if Tp % 4 or Y % 4 or X % 4:
        raise NotImplementedError("dl_cs HIP path: T+2*pad, Y and X must be multiples of 4")
    grid = (B, Tp, Y, X)
    N = Tp * Y * X
    cin = 2 * E
    F = P[names["init_w"]].shape[0]
    u = K.swin_pre(x.contiguous(), torch.float32, pad, PAD_CIN)
    r = [_conv(u, cin, P[names["init_w"]], F, F, grid, bias=P[names["init_b"]], relu_out=1)]
    ts, os_, ms, hs, ss, as_, qs = [], [], [], [], [], [], []
    for k in range(nblocks):
        wa, ba, wb, bb, w1, b1, w2, b2, w5, b5 = (P[n] for n in names["blocks"][k])
        t = _conv(r[-1], F, wa, F, F, grid, bias=ba, relu_out=1)
        o = _conv(t, F, wb, F, F, grid, bias=bb)
        m = K.se_pool(o, B, N, F)
        h, s = K.se_gate(m, w1, b1, w2, b2)
        a = K.cbam_chan_mean(o, s, grid, F)
        q = K.cbam_stencil5(a, w5, b5, grid)
        r.append(K.cbam_scale_res_relu(o, s, q, r[-1], grid, F))
        ts.append(t); os_.append(o); ms.append(m); hs.append(h); ss.append(s); as_.append(a); qs.append(q)
    o = _conv(r[-1], F, P[names["final_w"]], cin, PAD_CIN, grid, bias=P[names["final_b"]], res=u,
              out_dtype=torch.float32)
    out = K.swin_post(o, (B, E, T, Y, X), pad)
    from . import engine
    if engine.CAPTURE is not None:                   # test hook: ReLU decisions in the oracle's call order
        order = [t for k in range(nblocks) for t in (r[k], ts[k])] + [r[-1]]
        engine.CAPTURE.append(dict(relu_inputs=order, grid=grid, C=F))
    return out, dict(u=u, r=r, ts=ts, os=os_, ms=ms, hs=hs, ss=ss, as_=as_, qs=qs, grid=grid, cin=cin, F=F,
                     shape=(B, E, T, Y, X), pad=pad)


def cbamresnet_backward(P, names, sv, gout, grads):
    grid, cin, F, pad = sv["grid"], sv["cin"], sv["F"], sv["pad"]
    B = grid[0]
    N = grid[1] * grid[2] * grid[3]
    rows = B * N
    r, ts, u = sv["r"], sv["ts"], sv["u"]
    go = K.swin_post_bwd(gout.contiguous(), torch.float32, pad, PAD_CIN)           # dL/d out (and the + u path)
    # final layer: out = conv_f(r_L) + b_f + u
    _wgrad(r[-1], F, go, cin, grid, grads[names["final_w"]], grads[names["final_b"]], rows)
    g = _dgrad(go, cin, P[names["final_w"]], F, F, grid)                            # dL/d r_L
    for k in reversed(range(len(ts))):
        wa, ba, wb, bb, w1, b1, w2, b2, w5, b5 = (P[n] for n in names["blocks"][k])
        gwa, gba, gwb, gbb, gw1, gb1, gw2, gb2, gw5, gb5 = (grads[n] for n in names["blocks"][k])
        o, m, h, s, a, q = sv["os"][k], sv["ms"][k], sv["hs"][k], sv["ss"][k], sv["as_"][k], sv["qs"][k]
        # r_{k+1} = relu(q s o + r_k), q = b5 + w5 * mean_c(s o), s = gate(mean_v(o))
        dq = K.cbam_bwd_rowdot(g, r[k + 1], o, s, grid, F)
        K.cbam_stencil5_wgrad(dq, a, grid, gw5, gb5)
        da = K.cbam_stencil5(dq, w5, None, grid, transposed=True)
        ds = K.cbam_bwd_reduce(g, r[k + 1], o, q, da, grid, F)
        dm = K.se_gate_bwd(ds, s, h, m, w1, w2, 1.0 / N, gw1, gb1, gw2, gb2)
        do = K.cbam_bwd_apply(g, r[k + 1], s, q, da, dm, grid, F)                   # g is now gz = dL/d(q s o + r_k)
        _wgrad(ts[k], F, do, F, grid, gwb, gbb, rows)
        gt = _dgrad(do, F, wb, F, F, grid, mask=ts[k])
        _wgrad(r[k], F, gt, F, grid, gwa, gba, rows)
        g = _dgrad(gt, F, wa, F, F, grid, res=g)                                    # dL/d r_k (conv + residual)
    g = K.relu_grad(g, r[0])                                                        # dL/d o_0
    # init layer: o_0 = conv0(u) + b0 ;  du = conv0^T(g) + go (the final residual)
    _wgrad(u, cin, g, F, grid, grads[names["init_w"]], grads[names["init_b"]], rows)
    du = _dgrad(g, F, P[names["init_w"]], cin, PAD_CIN, grid, res=go, out_dtype=torch.float32)
    return K.swin_pre_bwd(du, sv["shape"], pad)


class _CbamResNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, meta, *plist):
        P = dict(zip(meta["order"], plist))
        out, sv = cbamresnet_forward(P, meta["names"], x.to(torch.complex64), meta["nblocks"], meta["pad"])
        ctx.state = (P, sv, meta)
        return out

    @staticmethod
    def backward(ctx, gout):
        P, sv, meta = ctx.state
        grads = {n: torch.zeros_like(p) for n, p in P.items()}
        gx = cbamresnet_backward(P, meta["names"], sv, gout.to(torch.complex64), grads)
        ctx.state = None
        return (gx, None) + tuple(grads[n] for n in meta["order"])


class CBAMResNet(nn.Module):
    """CBAM:565-639 -- init ConvBlock (no activation), num_resblocks CBAMResBlocks,
    final pre-activation ConvBlock back to in_chans, plus the input residual."""

    def __init__(self, num_resblocks, in_chans, chans, kernel_size, rr, act_type='relu', use_complex_layers=False,
                 circular_pad=True):
        super().__init__()
        if use_complex_layers:
            raise NotImplementedError("dl_cs HIP CBAMResNet: COMPLEX: False (configs/config_cbam.yaml)")
        if kernel_size != 3 or act_type != 'relu' or not circular_pad:
            raise NotImplementedError("dl_cs HIP CBAMResNet: kernel 3, relu, circular pad (configs/config_cbam.yaml)")
        if not (1 <= chans <= 1024 and 1 <= rr <= 256):
            raise NotImplementedError("dl_cs HIP CBAMResNet: 1 <= NUM_FEATURES <= 1024, 1 <= RR <= 256 (dlcs_se_gate)")
        self.use_complex_layers = use_complex_layers
        self.circular_pad = circular_pad
        self.pad_size = (2 * num_resblocks + 2) * (kernel_size - 1) // 2                  # CBAM:578
        self.init_layer = ConvBlock(in_chans, chans, kernel_size, act_type='none')
        self.se_res_blocks = nn.ModuleList([CBAMResBlock(chans, kernel_size, rr, act_type=act_type)
                                            for _ in range(num_resblocks)])
        self.final_layer = ConvBlock(chans, in_chans, kernel_size, act_type=act_type)

    def _names(self):
        c = lambda pre: (f"{pre}.conv.weight", f"{pre}.conv.bias")
        f = lambda pre: (f"{pre}.fc.weight", f"{pre}.fc.bias")
        blocks = []
        for k in range(len(self.se_res_blocks)):
            b = f"se_res_blocks.{k}"
            blocks.append(c(f"{b}.layers1.0.layers.2") + c(f"{b}.layers1.1.layers.2") +
                          f(f"{b}.CAmodule.0.layers.0") + f(f"{b}.CAmodule.0.layers.2") +
                          c(f"{b}.SAmodule.0.layers.0"))
        iw, ib = c("init_layer.layers.2")
        fw, fb = c("final_layer.layers.2")
        return dict(init_w=iw, init_b=ib, final_w=fw, final_b=fb, blocks=blocks)

    def forward(self, input):
        if get_compute_dtype() != torch.float32:
            raise NotImplementedError("dl_cs HIP CBAMResNet: fp32 (the generic conv kernels; no bf16 wgrad at 64 ch)")
        if not input.is_cuda:
            raise RuntimeError("dl_cs HIP CBAMResNet needs GPU tensors (no CPU fallback in the product path)")
        params = dict(self.named_parameters())
        order = list(params.keys())
        meta = dict(order=order, names=self._names(), nblocks=len(self.se_res_blocks), pad=self.pad_size)
        return _CbamResNetFn.apply(input, meta, *[params[n] for n in order])
