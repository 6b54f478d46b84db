"""3D ResNet regularizer of the reference's "dlespirit" unrolled network
(BASELINE config 1, configs/example.yaml), MI355X build.

Same classes, constructor arguments and state_dict keys as the reference
(r3d = dl_cs/models/resnet3d.py:163-317).  The whole network runs as one HIP
autograd node (_TrunkFn) on the generic Conv3d k3 kernels (dlcs_conv3d_k3 /
dlcs_conv3d_k3_wgrad, any channel count padded to 32) in the patch-blocked
channels-last layout of the Swin path.

The reference's pre-activation blocks use nn.ReLU(inplace=True) (r3d:39-55,
:200-208): a ResBlock's ReLU overwrites its input, so its residual adds
relu(input), not input (r3d:232-240), and the final layer's ReLU likewise
(r3d:308).  Every block output is therefore only ever consumed as relu(o), and
the HIP forward stores r = relu(o) straight from the producing conv's epilogue:

    u  = pre(x)                          cat(re, im), circular T pad (r3d:270-282)
    r0 = relu(conv0(u))                  init_layer, act 'none' (r3d:260, :305)
    t  = relu(conv_a(r_k))               ResBlock first ConvBlock + the second's ReLU
    r_{k+1} = relu(conv_b(t) + r_k)      ResBlock (r3d:232-240) + next block's ReLU
    out = conv_f(r_L) + u                final_layer + input (r3d:308)
    x'  = post(out)                      crop, complex (r3d:284-294)

Compute dtype bf16 (swin3D.set_compute_dtype): u, r, t (the gated trunks' o too) and every
F-channel gradient are stored in bf16; the convs accumulate in fp32, add bias and residual in
fp32 and round once.  Weights, biases and their gradients, the final conv's output, the init
dgrad's output and the complex boundary stay fp32, and so do the two residuals that cross the
boundary (the + u of the output and its backward + go: a second, fp32 pre / post_bwd).
"""
import torch
from torch import nn

from . import _ops as K
from .swin3D import ConvBlock, get_compute_dtype

PAD_CIN = 8


class ResBlock(nn.Module):
    """r3d:214-240 -- two pre-activation ConvBlocks and a residual connection."""

    def __init__(self, chans, kernel_size, act_type='relu', is_complex=False):
        super().__init__()
        self.layers = nn.Sequential(
            ConvBlock(chans, chans, kernel_size, act_type=act_type, is_complex=is_complex),
            ConvBlock(chans, chans, kernel_size, act_type=act_type, is_complex=is_complex))

    def forward(self, input):
        raise NotImplementedError("dl_cs: ResBlock runs inside ResNet's fused HIP node")


def _conv(x, cin, w, cout, out_ld, grid, **kw):
    return K.conv3d(x, cin, K.conv_pack(w, x.dtype, 0), cout, out_ld, grid, **kw)


def _dgrad(g, cout_w, w, cin_w, out_ld, grid, **kw):
    """dL/d(conv input) of a conv with weight w [cout_w, cin_w, 3, 3, 3] from g [rows, >= cout_w]."""
    return K.conv3d(g, cout_w, K.conv_pack(w, g.dtype, 1), cin_w, out_ld, grid, **kw)


WGRAD_VOX_BF16 = 8192      # voxels per workgroup range of the bf16 tap-row weight gradient


def _wgrad(x, cin, g, cout, grid, gw, gb, rows):
    dwp = torch.zeros((27, K.pad32(cout), K.pad32(cin)), dtype=torch.float32, device=x.device)
    if x.dtype == torch.bfloat16:
        K.conv3d_wgrad(x, cin, 0, g, cout, grid, dwp, vox_per_block=WGRAD_VOX_BF16)
    else:
        K.conv3d_wgrad(x, cin, 0, g, cout, grid, dwp)
    K.conv_unpack_grad(dwp, gw, cout, cin)
    K.colsum(g, gb, rows=rows, C=cout, ld=g.shape[-1])


def _capture(r, ts, grid, F, box):
    """Test hook: the ReLU decisions [r0, t0, r1, t1, ..., r_L] in the oracle's call order
    (on the padded path in the padded grid's rows, with the box beside it)."""
    from . import engine
    if engine.CAPTURE is not None:
        order = [t for k in range(len(ts)) for t in (r[k], ts[k])] + [r[-1]]
        entry = dict(relu_inputs=order, grid=grid, C=F)
        if box is not None:
            entry["box"] = box
        engine.CAPTURE.append(entry)


# Any grid size.  The kernels take grids whose axes are multiples of 4, so a call whose true
# grid ("box") (B, T + 2 pad, Y, X) is not one runs on the grid rounded up ("padded path").
# The rows outside the box are slack rows; the conv on the padded grid is the reference's
# zero-padded conv on the box as long as every tensor a conv (forward, dgrad, wgrad), colsum,
# the gates' pool / channel mean / stencil or a backward reduce reads is zero there.  box_pre
# and box_post_bwd write zeros there, a masked dgrad and relu_grad give zeros wherever the
# stored post-ReLU tensor is zero, and box_post / box_pre_bwd read the box only; what is left
# are the tensors that a bias (forward) or dmean / da (gate backward) makes non-zero on slack
# rows, which _zero clears: r0, t, r_{k+1} (plain trunk) or conv_b's output o (gated trunk)
# in the forward, the gate backward's dout in the backward.  Without slack box is None and
# the launches are the unpadded ones.
def _pre(x, pad, dtype=torch.float32):
    """x complex64 [B, E, T, Y, X] -> (u, grid, box): grid the (padded) grid of u's rows (of dtype)."""
    B, E, T, Y, X = x.shape
    box = (B, T + 2 * pad, Y, X)
    grid = (B,) + tuple(K.pad4(n) for n in box[1:])
    if grid == box:
        return K.swin_pre(x.contiguous(), dtype, pad, PAD_CIN), grid, None
    if dtype == torch.float32:
        return K.box_pre(x.contiguous(), pad, PAD_CIN, grid), grid, box
    return K.box_pre(x.contiguous(), pad, PAD_CIN, grid, dtype=dtype), grid, box


def _post(o, shape, pad, grid, box):
    return K.swin_post(o, shape, pad) if box is None else K.box_post(o, shape, pad, grid)


def _post_bwd(gout, pad, grid, box, dtype=torch.float32):
    if box is None:
        return K.swin_post_bwd(gout.contiguous(), dtype, pad, PAD_CIN)
    if dtype == torch.float32:
        return K.box_post_bwd(gout.contiguous(), pad, PAD_CIN, grid)
    return K.box_post_bwd(gout.contiguous(), pad, PAD_CIN, grid, dtype=dtype)


def _pre_bwd(du, shape, pad, grid, box):
    return K.swin_pre_bwd(du, shape, pad) if box is None else K.box_pre_bwd(du, shape, pad, grid)


def _zero(t, C, grid, box):
    """t with its slack rows cleared in place (nothing to do without slack)."""
    return t if box is None else K.box_zero(t, C, grid, box)


def _nvox(grid, box):
    """Voxels per batch item that the gates' means run over: the box's, not the padded grid's."""
    g = grid if box is None else box
    return g[1] * g[2] * g[3]


def resnet_forward(P, names, x, nblocks, pad, dtype=torch.float32):
    """x complex64 [B, E, T, Y, X] -> (out complex64, saved).  dtype: the storage of u and of every
    F-channel activation (the convs follow their input; the final conv's output stays fp32)."""
    B, E, T, Y, X = x.shape
    cin = 2 * E
    F = P[names["init_w"]].shape[0]
    u, grid, box = _pre(x, pad, dtype)
    u_res = u if dtype == torch.float32 else _pre(x, pad)[0]     # the input residual is added unrounded
    r = [_zero(_conv(u, cin, P[names["init_w"]], F, F, grid, bias=P[names["init_b"]], relu_out=1), F, grid, box)]
    ts = []
    for k in range(nblocks):
        wa, ba, wb, bb = (P[n] for n in names["blocks"][k])
        t = _zero(_conv(r[-1], F, wa, F, F, grid, bias=ba, relu_out=1), F, grid, box)
        ts.append(t)
        r.append(_zero(_conv(t, F, wb, F, F, grid, bias=bb, res=r[-1], relu_out=1), F, grid, box))
    o = _conv(r[-1], F, P[names["final_w"]], cin, PAD_CIN, grid, bias=P[names["final_b"]], res=u_res,
              out_dtype=torch.float32)
    out = _post(o, (B, E, T, Y, X), pad, grid, box)
    _capture(r, ts, grid, F, box)
    return out, dict(u=u, r=r, ts=ts, grid=grid, box=box, cin=cin, F=F, shape=(B, E, T, Y, X), pad=pad, dtype=dtype)


def resnet_backward(P, names, sv, gout, grads):
    grid, box, cin, F, pad = sv["grid"], sv["box"], sv["cin"], sv["F"], sv["pad"]
    rows = grid[0] * grid[1] * grid[2] * grid[3]
    r, ts, u = sv["r"], sv["ts"], sv["u"]
    go = _post_bwd(gout, pad, grid, box, sv["dtype"])                               # dL/d out (and the + u path)
    go_res = go if sv["dtype"] == torch.float32 else _post_bwd(gout, pad, grid, box)   # the + u path, unrounded
    # final layer: out = conv_f(r_L) + b_f + u
    _wgrad(r[-1], F, go, cin, grid, grads[names["final_w"]], grads[names["final_b"]], rows)
    g = _dgrad(go, cin, P[names["final_w"]], F, F, grid, mask=r[-1])                # dL/d o_L (through relu)
    for k in reversed(range(len(ts))):
        wa, ba, wb, bb = (P[n] for n in names["blocks"][k])
        gwa, gba, gwb, gbb = (grads[n] for n in names["blocks"][k])
        # o_{k+1} = conv_b(t_k) + b_b + r_k ;  t_k = relu(conv_a(r_k) + b_a)
        _wgrad(ts[k], F, g, F, grid, gwb, gbb, rows)
        gt = _dgrad(g, F, wb, F, F, grid, mask=ts[k])
        _wgrad(r[k], F, gt, F, grid, gwa, gba, rows)
        gr = _dgrad(gt, F, wa, F, F, grid, res=g)                                  # dL/d r_k (conv + residual)
        g = K.relu_grad(gr, r[k])                                                  # dL/d o_k
    # init layer: o_0 = conv0(u) + b0 ;  du = conv0^T(g) + go (the final residual)
    _wgrad(u, cin, g, F, grid, grads[names["init_w"]], grads[names["init_b"]], rows)
    du = _dgrad(g, F, P[names["init_w"]], cin, PAD_CIN, grid, res=go_res, out_dtype=torch.float32)
    return _pre_bwd(du, sv["shape"], pad, grid, box)


def gated_forward(P, names, x, nblocks, pad, gate, dtype=torch.float32):
    """The trunk of the gated families (se3d.SeGate, CBAM.CbamGate), which keep conv_b's
    output o_k un-activated and put a gate between it and the residual:

        r_{k+1}, saved = gate.fwd(o_k, r_k, w, grid, F, N)     r_{k+1} = relu(gate(o_k) + r_k)

    with w the block's gate parameters (names["blocks"][k][4:]), N the voxels per batch item
    its means run over (the box's; o_k is zero on slack rows) and saved whatever the
    gate's backward needs besides o_k.  x complex64 [B, E, T, Y, X] -> (out complex64, saved)."""
    B, E, T, Y, X = x.shape
    cin = 2 * E
    F = P[names["init_w"]].shape[0]
    u, grid, box = _pre(x, pad, dtype)
    u_res = u if dtype == torch.float32 else _pre(x, pad)[0]     # the input residual is added unrounded
    r = [_zero(_conv(u, cin, P[names["init_w"]], F, F, grid, bias=P[names["init_b"]], relu_out=1), F, grid, box)]
    ts, os_, gs = [], [], []
    N = _nvox(grid, box)
    for k in range(nblocks):
        wa, ba, wb, bb, *w = (P[n] for n in names["blocks"][k])
        t = _zero(_conv(r[-1], F, wa, F, F, grid, bias=ba, relu_out=1), F, grid, box)
        o = _zero(_conv(t, F, wb, F, F, grid, bias=bb), F, grid, box)
        r_next, saved = gate.fwd(o, r[-1], w, grid, F, N)
        r.append(r_next); ts.append(t); os_.append(o); gs.append(saved)
    o = _conv(r[-1], F, P[names["final_w"]], cin, PAD_CIN, grid, bias=P[names["final_b"]], res=u_res,
              out_dtype=torch.float32)
    out = _post(o, (B, E, T, Y, X), pad, grid, box)
    _capture(r, ts, grid, F, box)
    return out, dict(u=u, r=r, ts=ts, os=os_, gs=gs, grid=grid, box=box, cin=cin, F=F, shape=(B, E, T, Y, X), pad=pad,
                     dtype=dtype)


def gated_backward(P, names, sv, gout, grads, gate):
    """Backward of gated_forward.  Per block

        do = gate.bwd(g, r_{k+1}, o_k, saved, w, gw, grid, F, N)

    takes g = dL/dr_{k+1}, masks it in place into gz = g [r_{k+1} > 0] (the gradient of the
    ReLU's argument, and so also the residual gradient into r_k), accumulates the gate
    parameters' gradients into gw and returns conv_b's output gradient."""
    grid, box, cin, F, pad = sv["grid"], sv["box"], sv["cin"], sv["F"], sv["pad"]
    rows = grid[0] * grid[1] * grid[2] * grid[3]
    N = _nvox(grid, box)
    r, ts, u = sv["r"], sv["ts"], sv["u"]
    go = _post_bwd(gout, pad, grid, box, sv["dtype"])                               # dL/d out (and the + u path)
    go_res = go if sv["dtype"] == torch.float32 else _post_bwd(gout, pad, grid, box)   # the + u path, unrounded
    # final layer: out = conv_f(r_L) + b_f + u
    _wgrad(r[-1], F, go, cin, grid, grads[names["final_w"]], grads[names["final_b"]], rows)
    g = _dgrad(go, cin, P[names["final_w"]], F, F, grid)                            # dL/d r_L
    for k in reversed(range(len(ts))):
        wa, ba, wb, bb, *w = (P[n] for n in names["blocks"][k])
        gwa, gba, gwb, gbb, *gw = (grads[n] for n in names["blocks"][k])
        # r_{k+1} = relu(gate(o) + r_k), o = conv_b(t_k) + b_b, t_k = relu(conv_a(r_k) + b_a)
        do = _zero(gate.bwd(g, r[k + 1], sv["os"][k], sv["gs"][k], w, gw, grid, F, N), F, grid, box)   # g is now gz
        _wgrad(ts[k], F, do, F, grid, gwb, gbb, rows)
        gt = _dgrad(do, F, wb, F, F, grid, mask=ts[k])
        _wgrad(r[k], F, gt, F, grid, gwa, gba, rows)
        g = _dgrad(gt, F, wa, F, F, grid, res=g)                                    # dL/d r_k (conv + residual)
    g = K.relu_grad(g, r[0])                                                        # dL/d o_0
    # init layer: o_0 = conv0(u) + b0 ;  du = conv0^T(g) + go (the final residual)
    _wgrad(u, cin, g, F, grid, grads[names["init_w"]], grads[names["init_b"]], rows)
    du = _dgrad(g, F, P[names["init_w"]], cin, PAD_CIN, grid, res=go_res, out_dtype=torch.float32)
    return _pre_bwd(du, sv["shape"], pad, grid, box)


class _TrunkFn(torch.autograd.Function):
    """One node per regularizer call; meta["trunk"] is the family's (forward, backward) pair."""

    @staticmethod
    def forward(ctx, x, meta, *plist):
        P = dict(zip(meta["order"], plist))
        out, sv = meta["trunk"][0](P, meta["names"], x.to(torch.complex64), meta["nblocks"], meta["pad"],
                                   dtype=meta["dtype"])
        ctx.state = (P, sv, meta)
        return out

    @staticmethod
    def backward(ctx, gout):
        P, sv, meta = ctx.state
        grads = {n: torch.zeros_like(p) for n, p in P.items()}
        gx = meta["trunk"][1](P, meta["names"], sv, gout.to(torch.complex64), grads)
        ctx.state = None
        return (gx, None) + tuple(grads[n] for n in meta["order"])


def _wb(pre):
    return f"{pre}.weight", f"{pre}.bias"


class _TrunkNet(nn.Module):
    """What ResNet, se3d.SeResNet and CBAM.CBAMResNet share: init ConvBlock (no activation),
    num_resblocks blocks, final pre-activation ConvBlock back to in_chans, plus the input
    residual (r3d:243-317).  A family supplies the five names below, its own __init__
    signature (rr is the gated families' hidden width) and _block_keys(b): the parameter keys
    of the block at prefix b, conv_a's and conv_b's weight and bias, then the gate's."""
    NAME = None        # the family, as the messages call it
    CONFIG = None      # the config file they cite
    BLOCK = None       # block class
    BLOCKS = None      # attribute (and state_dict prefix) of the block list
    TRUNK = None       # (forward, backward) for _TrunkFn
    DTYPES = (torch.float32, torch.bfloat16)     # compute dtypes (swin3D.get_compute_dtype) the family runs in

    def __init__(self, num_resblocks, in_chans, chans, kernel_size, act_type, use_complex_layers, circular_pad,
                 rr=None):
        super().__init__()
        head = f"dl_cs HIP {self.NAME}:"
        if use_complex_layers:
            raise NotImplementedError(f"{head} COMPLEX: False ({self.CONFIG})")
        if kernel_size != 3 or act_type != 'relu' or not circular_pad:
            raise NotImplementedError(f"{head} kernel 3, relu, circular pad ({self.CONFIG})")
        if rr is not None and not (1 <= chans <= 1024 and 1 <= rr <= 256):
            raise NotImplementedError(f"{head} 1 <= NUM_FEATURES <= 1024, 1 <= RR <= 256 (dlcs_se_gate)")
        self.use_complex_layers = use_complex_layers
        self.circular_pad = circular_pad
        self.pad_size = (2 * num_resblocks + 2) * (kernel_size - 1) // 2      # r3d:253, se3d:454, CBAM:578
        gate_args = () if rr is None else (rr,)
        self.init_layer = ConvBlock(in_chans, chans, kernel_size, act_type='none')
        setattr(self, self.BLOCKS, nn.ModuleList([self.BLOCK(chans, kernel_size, *gate_args, act_type=act_type)
                                                  for _ in range(num_resblocks)]))
        self.final_layer = ConvBlock(chans, in_chans, kernel_size, act_type=act_type)

    @staticmethod
    def c(pre):
        """Weight and bias keys of the ConvBlock at pre."""
        return _wb(f"{pre}.layers.2.conv")

    def forward(self, input):
        dtype = get_compute_dtype()
        if dtype not in self.DTYPES:
            raise NotImplementedError(f"dl_cs HIP {self.NAME}: compute dtype " +
                                      " or ".join(str(d).replace("torch.", "") for d in self.DTYPES) +
                                      f" (got {dtype}; bf16 stores the activations, weights and gradients stay fp32)")
        if not input.is_cuda:
            raise RuntimeError(f"dl_cs HIP {self.NAME} needs GPU tensors (no CPU fallback in the product path)")
        params = dict(self.named_parameters())
        order = list(params.keys())
        nblocks = len(getattr(self, self.BLOCKS))
        (iw, ib), (fw, fb) = self.c("init_layer"), self.c("final_layer")
        names = dict(init_w=iw, init_b=ib, final_w=fw, final_b=fb,
                     blocks=[self._block_keys(f"{self.BLOCKS}.{k}") for k in range(nblocks)])
        meta = dict(order=order, names=names, nblocks=nblocks, pad=self.pad_size, trunk=self.TRUNK, dtype=dtype)
        return _TrunkFn.apply(input, meta, *[params[n] for n in order])


class ResNet(_TrunkNet):
    """r3d:243-317 -- init ConvBlock (no activation), num_resblocks ResBlocks,
    final pre-activation ConvBlock back to in_chans, plus the input residual."""
    NAME, CONFIG, BLOCK, BLOCKS = "ResNet", "configs/example.yaml", ResBlock, "res_blocks"
    TRUNK = (resnet_forward, resnet_backward)

    def __init__(self, num_resblocks, in_chans, chans, kernel_size, act_type='relu', use_complex_layers=False,
                 circular_pad=True):
        super().__init__(num_resblocks, in_chans, chans, kernel_size, act_type, use_complex_layers, circular_pad)

    def _block_keys(self, b):
        return self.c(f"{b}.layers.0") + self.c(f"{b}.layers.1")

