"""Squeeze-excitation 3D ResNet regularizer (MODEL_TYPE 'SE') of the reference's
unrolledSE network, MI355X build.

Same classes, constructor arguments and state_dict keys as the reference
(se3d = dl_cs/models/se3d.py:302-515).  The conv trunk is resnet3d's fused node
(the same generic Conv3d k3 kernels, patch-blocked channels-last rows); around it
the per-(batch item, channel) gate runs on the dlcs_se_* kernels (se.hip).

As in resnet3d.py the pre-activation ReLUs are in place (se3d:416-417 build the
ConvBlocks of resnet3d), so a block's residual adds relu(input) and every block
output is only ever consumed through a ReLU; the HIP forward stores r = relu(.)
directly.  With N = Tp Y X voxels per batch item (time pad included), R = rr the
hidden width (se3d:325 passes rr straight to FC(out_chans, rr)):

    u   = pre(x)                                cat(re, im), circular T pad
    r0  = relu(conv0(u))
    t_k = relu(conv_a(r_k))
    o_k = conv_b(t_k)                           bias, no ReLU
    m_k = mean over voxels of o_k               GlobalAvgPool (se3d:92)
    h_k = relu(W1 m_k + b1);  s_k = sigmoid(W2 h_k + b2)
    r_{k+1} = relu(s_k o_k + r_k)               se3d:435-438 + the next in-place ReLU
    out = conv_f(r_L) + u ;  x' = post(out)

Backward of one block from g = dL/dr_{k+1}:

    gz = g [r_{k+1} > 0]                        also the residual gradient into r_k
    ds = sum over voxels of gz o_k
    dz2 = ds s (1 - s);  dW2 += dz2^T h;  db2 += sum_b dz2
    dh = (dz2 W2) [h > 0];  dW1 += dh^T m;  db1 += sum_b dh;  dm = dh W1
    do_k = gz s + dm / N                        conv_b's output gradient
"""
import torch
from torch import nn

from . import _ops as K
from .resnet3d import PAD_CIN, _conv, _dgrad, _wgrad
from .swin3D import Activation, ConvBlock, get_compute_dtype

_FUSED = "dl_cs: runs inside SeResNet's fused HIP node"


class GlobalAvgPool(nn.Module):
    """se3d:80-97 -- mean over (T, Y, X) of each channel."""

    def __init__(self):
        super().__init__()
        self.gpool = nn.Identity()

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class FC(nn.Module):
    """se3d:100-114 -- nn.Linear."""

    def __init__(self, in_chans, out_chans):
        super().__init__()
        self.fc = nn.Linear(in_chans, out_chans)

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class SeBlock(nn.Module):
    """se3d:302-348 -- GlobalAvgPool -> FC(out_chans, rr) -> ReLU -> FC(rr, out_chans) -> sigmoid."""

    def __init__(self, out_chans, rr, norm_type='none', is_complex=False):
        super().__init__()
        if is_complex:
            raise NotImplementedError("dl_cs HIP SeResNet: COMPLEX: False")
        self.is_complex = is_complex
        self.layers = nn.Sequential(GlobalAvgPool(), FC(out_chans, rr), Activation("relu"), FC(rr, out_chans),
                                    Activation("sigmoid"))

    def forward(self, input):
        raise NotImplementedError(_FUSED)


class SeResBlock(nn.Module):
    """se3d:401-438 -- two pre-activation ConvBlocks scaled by a SeBlock's gate, plus the residual."""

    def __init__(self, chans, kernel_size, rr, act_type='relu', is_complex=False):
        super().__init__()
        self.layers1 = nn.Sequential(
            ConvBlock(chans, chans, kernel_size, act_type=act_type, is_complex=is_complex),
            ConvBlock(chans, chans, kernel_size, act_type=act_type, is_complex=is_complex))
        self.layers2 = SeBlock(chans, rr, is_complex=is_complex)

    def forward(self, input):
        raise NotImplementedError(_FUSED)


def seresnet_forward(P, names, x, nblocks, pad):
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
    ts, os_, ms, hs, ss = [], [], [], [], []
    for k in range(nblocks):
        wa, ba, wb, bb, w1, b1, w2, b2 = (P[n] for n in names["blocks"][k])
        t = _conv(r[-1], F, wa, F, F, grid, bias=ba, relu_out=1)
        o = _conv(t, F, wb, F, F, grid, bias=bb)
        m = K.se_pool(o, B, N, F)
        h, s = K.se_gate(m, w1, b1, w2, b2)
        r.append(K.se_scale_res_relu(o, s, r[-1], B, N, F))
        ts.append(t); os_.append(o); ms.append(m); hs.append(h); ss.append(s)
    o = _conv(r[-1], F, P[names["final_w"]], cin, PAD_CIN, grid, bias=P[names["final_b"]], res=u,
              out_dtype=torch.float32)
    out = K.swin_post(o, (B, E, T, Y, X), pad)
    from . import engine
    if engine.CAPTURE is not None:                   # test hook: ReLU decisions in the oracle's call order
        order = [t for k in range(nblocks) for t in (r[k], ts[k])] + [r[-1]]
        engine.CAPTURE.append(dict(relu_inputs=order, grid=grid, C=F))
    return out, dict(u=u, r=r, ts=ts, os=os_, ms=ms, hs=hs, ss=ss, grid=grid, cin=cin, F=F, shape=(B, E, T, Y, X),
                     pad=pad)


def seresnet_backward(P, names, sv, gout, grads):
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
        wa, ba, wb, bb, w1, b1, w2, b2 = (P[n] for n in names["blocks"][k])
        gwa, gba, gwb, gbb, gw1, gb1, gw2, gb2 = (grads[n] for n in names["blocks"][k])
        o, m, h, s = sv["os"][k], sv["ms"][k], sv["hs"][k], sv["ss"][k]
        # r_{k+1} = relu(s o + r_k), s = gate(mean(o)), o = conv_b(t_k) + b_b, t_k = relu(conv_a(r_k) + b_a)
        ds = K.se_bwd_reduce(g, r[k + 1], o, B, N, F)
        dm = K.se_gate_bwd(ds, s, h, m, w1, w2, 1.0 / N, gw1, gb1, gw2, gb2)
        do = K.se_bwd_apply(g, r[k + 1], s, dm, B, N, F)                            # g is now gz = dL/d(s o + r_k)
        _wgrad(ts[k], F, do, F, grid, gwb, gbb, rows)
        gt = _dgrad(do, F, wb, F, F, grid, mask=ts[k])
        _wgrad(r[k], F, gt, F, grid, gwa, gba, rows)
        g = _dgrad(gt, F, wa, F, F, grid, res=g)                                    # dL/d r_k (conv + residual)
    g = K.relu_grad(g, r[0])                                                        # dL/d o_0
    # init layer: o_0 = conv0(u) + b0 ;  du = conv0^T(g) + go (the final residual)
    _wgrad(u, cin, g, F, grid, grads[names["init_w"]], grads[names["init_b"]], rows)
    du = _dgrad(g, F, P[names["init_w"]], cin, PAD_CIN, grid, res=go, out_dtype=torch.float32)
    return K.swin_pre_bwd(du, sv["shape"], pad)


class _SeResNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, meta, *plist):
        P = dict(zip(meta["order"], plist))
        out, sv = seresnet_forward(P, meta["names"], x.to(torch.complex64), meta["nblocks"], meta["pad"])
        ctx.state = (P, sv, meta)
        return out

    @staticmethod
    def backward(ctx, gout):
        P, sv, meta = ctx.state
        grads = {n: torch.zeros_like(p) for n, p in P.items()}
        gx = seresnet_backward(P, meta["names"], sv, gout.to(torch.complex64), grads)
        ctx.state = None
        return (gx, None) + tuple(grads[n] for n in meta["order"])


class SeResNet(nn.Module):
    """se3d:441-515 -- init ConvBlock (no activation), num_resblocks SeResBlocks,
    final pre-activation ConvBlock back to in_chans, plus the input residual."""

    def __init__(self, num_resblocks, in_chans, chans, kernel_size, rr, act_type='relu', use_complex_layers=False,
                 circular_pad=True):
        super().__init__()
        if use_complex_layers:
            raise NotImplementedError("dl_cs HIP SeResNet: COMPLEX: False (configs/config_se.yaml)")
        if kernel_size != 3 or act_type != 'relu' or not circular_pad:
            raise NotImplementedError("dl_cs HIP SeResNet: kernel 3, relu, circular pad (configs/config_se.yaml)")
        if not (1 <= chans <= 1024 and 1 <= rr <= 256):
            raise NotImplementedError("dl_cs HIP SeResNet: 1 <= NUM_FEATURES <= 1024, 1 <= RR <= 256 (dlcs_se_gate)")
        self.use_complex_layers = use_complex_layers
        self.circular_pad = circular_pad
        self.pad_size = (2 * num_resblocks + 2) * (kernel_size - 1) // 2                  # se3d:454
        self.init_layer = ConvBlock(in_chans, chans, kernel_size, act_type='none')
        self.se_res_blocks = nn.ModuleList([SeResBlock(chans, kernel_size, rr, act_type=act_type)
                                            for _ in range(num_resblocks)])
        self.final_layer = ConvBlock(chans, in_chans, kernel_size, act_type=act_type)

    def _names(self):
        c = lambda pre: (f"{pre}.layers.2.conv.weight", f"{pre}.layers.2.conv.bias")
        f = lambda pre: (f"{pre}.fc.weight", f"{pre}.fc.bias")
        blocks = []
        for k in range(len(self.se_res_blocks)):
            b = f"se_res_blocks.{k}"
            blocks.append(c(f"{b}.layers1.0") + c(f"{b}.layers1.1") + f(f"{b}.layers2.layers.1") +
                          f(f"{b}.layers2.layers.3"))
        iw, ib = c("init_layer")
        fw, fb = c("final_layer")
        return dict(init_w=iw, init_b=ib, final_w=fw, final_b=fb, blocks=blocks)

    def forward(self, input):
        if get_compute_dtype() != torch.float32:
            raise NotImplementedError("dl_cs HIP SeResNet: fp32 (the generic conv kernels; no bf16 wgrad at 64 ch)")
        if not input.is_cuda:
            raise RuntimeError("dl_cs HIP SeResNet needs GPU tensors (no CPU fallback in the product path)")
        params = dict(self.named_parameters())
        order = list(params.keys())
        meta = dict(order=order, names=self._names(), nblocks=len(self.se_res_blocks), pad=self.pad_size)
        return _SeResNetFn.apply(input, meta, *[params[n] for n in order])
