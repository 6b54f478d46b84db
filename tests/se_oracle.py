"""CPU restatement of the SE-ResNet regularizer (MODEL_TYPE 'SE'), in plain PyTorch,
written from the operator's equations (dl_cs/models/se3d.py docstring).  Same
calling convention as oracle.dlcs_oracle.resnet, so O.pgd(..., reg=...), MaskedRelu
and goldutil.assert_masked_f64 take it unchanged:

    u   = pre(x)                                cat(re, im), circular T pad, pad = 2 L + 2
    r0  = relu(conv0(u))
    t_k = relu(conv_a(r_k));  o_k = conv_b(t_k)
    m_k = mean over (T', Y, X) of o_k
    h_k = relu(W1 m_k + b1);  s_k = sigmoid(W2 h_k + b2)
    r_{k+1} = relu(s_k o_k + r_k)
    out = conv_f(r_L) + u ;  x' = post(out)

`relu` replaces the volume ReLUs, called in the order [r0, t0, r1, t1, ..., r_L]
(the ResNet's); the hidden ReLU of the gate is not one of them (two numbers per
block and batch item, checked by the fixtures to sit away from 0).
"""
import torch
import torch.nn.functional as F


def se_gate(P, pre, o):
    """(mean, hidden, gate) of a block's SeBlock on o [B, F, T', Y, X]."""
    m = o.mean(dim=(2, 3, 4))
    h = F.relu(F.linear(m, P[pre + ".layers.1.fc.weight"], P[pre + ".layers.1.fc.bias"]))
    s = torch.sigmoid(F.linear(h, P[pre + ".layers.3.fc.weight"], P[pre + ".layers.3.fc.bias"]))
    return m, h, s


def seresnet(P, x, num_resblocks=2, relu=F.relu, kernel_size=3, stats=None):
    """x c64 / c128 [B, E, T, Y, X] -> the same shape.  stats (a list): per block,
    (gate, FC1 pre-activation) for the fixtures' spread checks."""
    pad = (2 * num_resblocks + 2) * (kernel_size - 1) // 2
    E = x.shape[1]
    u = torch.cat((x.real, x.imag), dim=1)
    u = F.pad(u, (0, 0, 0, 0, pad, pad), mode="circular")
    conv = lambda h, pre: F.conv3d(h, P[pre + ".layers.2.conv.weight"], P[pre + ".layers.2.conv.bias"], padding=1)
    r = relu(conv(u, "init_layer"))
    for k in range(num_resblocks):
        b = f"se_res_blocks.{k}"
        o = conv(relu(conv(r, b + ".layers1.0")), b + ".layers1.1")
        m, h, s = se_gate(P, b + ".layers2", o)
        if stats is not None:
            w1, b1 = P[b + ".layers2.layers.1.fc.weight"], P[b + ".layers2.layers.1.fc.bias"]
            stats.append((s.detach(), F.linear(m, w1, b1).detach()))
        r = relu(s[:, :, None, None, None] * o + r)
    o = conv(r, "final_layer") + u
    o = o[:, :, pad:o.shape[2] - pad]
    return torch.complex(o[:, :E].contiguous(), o[:, E:].contiguous())


FC_SCALE = 8.0


def scale_fc_weights(sd_or_module, scale=FC_SCALE):
    """Multiply the SE FC weights (keys with '.layers2.' ending in 'fc.weight') by
    `scale` in place: with the plain recipe fill the gates sit in 0.475-0.520 and a
    wrong gate path would hide; x8 spreads them over 0.014-0.968."""
    items = sd_or_module.items() if isinstance(sd_or_module, dict) else sd_or_module.named_parameters()
    n = 0
    with torch.no_grad():
        for k, v in items:
            if ".layers2." in k and k.endswith("fc.weight"):
                v.mul_(scale)
                n += 1
    return n
