"""CPU restatement of the CBAM-ResNet regularizer (MODEL_TYPE 'CBAM'), in plain
PyTorch, written from the operator's equations (dl_cs/models/CBAM.py docstring).  Same
calling convention as se_oracle.seresnet, so O.pgd(..., reg=...), MaskedRelu and
goldutil.assert_masked_f64 take it unchanged:

    u   = pre(x)                                cat(re, im), circular T pad, pad = 2 L + 2
    r0  = relu(conv0(u))
    t_k = relu(conv_a(r_k));  o_k = conv_b(t_k)
    m_k = mean over (T', Y, X) of o_k
    h_k = relu(W1 m_k + b1);  s_k = sigmoid(W2 h_k + b2)
    a_k = mean over channels of s_k o_k
    q_k = b5 + w5 * a_k                         5 x 5 x 5 cross-correlation, zero border
    r_{k+1} = relu(q_k s_k o_k + r_k)
    out = conv_f(r_L) + u ;  x' = post(out)

`relu` replaces the volume ReLUs, called in the order [r0, t0, r1, t1, ..., r_L]
(the ResNet's); the hidden ReLU of the channel gate is not one of them (the fixtures
check that it sits away from 0).
"""
import torch
import torch.nn.functional as F


def ca_gate(P, pre, o):
    """(mean, FC1 pre-activation, gate) of a block's CABlock on o [B, F, T', Y, X]."""
    m = o.mean(dim=(2, 3, 4))
    z = F.linear(m, P[pre + ".layers.0.fc.weight"], P[pre + ".layers.0.fc.bias"])
    s = torch.sigmoid(F.linear(F.relu(z), P[pre + ".layers.2.fc.weight"], P[pre + ".layers.2.fc.bias"]))
    return m, z, s


def sa_map(P, pre, x):
    """The SABlock's map [B, 1, T', Y, X] of x [B, F, T', Y, X]."""
    a = x.mean(dim=1, keepdim=True)
    return F.conv3d(a, P[pre + ".layers.0.conv.weight"], P[pre + ".layers.0.conv.bias"], padding=2)


def cbamresnet(P, x, num_resblocks=2, relu=F.relu, kernel_size=3, stats=None, maps=None):
    """x c64 / c128 [B, E, T, Y, X] -> the same shape.  stats (a list): per block,
    (gate, FC1 pre-activation, spatial map) for the fixtures' spread checks.  maps (a
    list): per block, the spatial map itself with its gradient retained, for a test
    that has to know how well conditioned the sum of that gradient is."""
    pad = (2 * num_resblocks + 2) * (kernel_size - 1) // 2
    E = x.shape[1]
    u = torch.cat((x.real, x.imag), dim=1)
    u = F.pad(u, (0, 0, 0, 0, pad, pad), mode="circular")
    conv = lambda h, pre: F.conv3d(h, P[pre + ".layers.2.conv.weight"], P[pre + ".layers.2.conv.bias"], padding=1)
    r = relu(conv(u, "init_layer"))
    for k in range(num_resblocks):
        b = f"se_res_blocks.{k}"
        o = conv(relu(conv(r, b + ".layers1.0")), b + ".layers1.1")
        m, z, s = ca_gate(P, b + ".CAmodule.0", o)
        so = s[:, :, None, None, None] * o
        q = sa_map(P, b + ".SAmodule.0", so)
        if stats is not None:
            stats.append((s.detach(), z.detach(), q.detach()))
        if maps is not None:
            q.retain_grad()
            maps.append(q)
        r = relu(q * so + r)
    o = conv(r, "final_layer") + u
    o = o[:, :, pad:o.shape[2] - pad]
    return torch.complex(o[:, :E].contiguous(), o[:, E:].contiguous())


FC_SCALE, SA_SCALE, SA_BIAS = 8.0, 32.0, 1.0


def spread_gates(sd_or_module):
    """After the recipe fill, in place: the CA fc.weights x 8, the SA conv weights x 32
    and the SA biases + 1.0.  With the plain fill the channel gates sit in 0.48-0.53 and
    the spatial map near 0.007, which kills the branch and would hide an error in it;
    with these the gates span 0.06-0.95 and the map 0.5-1.7 around 1.  Returns the
    number of tensors changed (4 per block)."""
    items = sd_or_module.items() if isinstance(sd_or_module, dict) else sd_or_module.named_parameters()
    n = 0
    with torch.no_grad():
        for k, v in items:
            if ".CAmodule." in k and k.endswith("fc.weight"):
                v.mul_(FC_SCALE)
            elif ".SAmodule." in k and k.endswith("conv.weight"):
                v.mul_(SA_SCALE)
            elif ".SAmodule." in k and k.endswith("conv.bias"):
                v.add_(SA_BIAS)
            else:
                continue
            n += 1
    return n
