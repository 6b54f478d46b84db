"""Direct unit checks of the layout, LayerNorm and glue kernels (csrc/layout.hip and the
tail of csrc/dit.hip): the small entry points that move activations between the
matrix-core kernels.  Every reference is computed on the CPU with plain torch indexing,
F.pad(mode="circular"), F.layer_norm or F.conv3d, in float64 or exactly; every output
buffer sits between two 64-element sentinel margins that must survive the call.

Tolerances follow from what each kernel does: data movement and dtype casts are compared
with torch.equal (the fp32 -> bf16 cast rounds to nearest even, as torch does), one fp32
multiply-add per element with the same fp32 expression on the CPU, sums with NRMSE < 1e-6
against float64 (the bar of test_gpu_kernels.py::test_layernorm_gather).

  entry point                          test
  -----------------------------------  -----------------------------------------------
  dlcs_swin_pre                        test_swin_pre, test_swin_pre_bwd (adjoint)
  dlcs_swin_pre_bwd                    test_swin_pre_bwd
  dlcs_swin_post                       test_swin_post, test_swin_post_bwd (adjoint)
  dlcs_swin_post_bwd                   test_swin_post_bwd
  dlcs_block_layout                    test_block_layout
  dlcs_permute                         test_permute_model_patterns, test_permute_6d_1d,
                                       test_grid_stride_over_launch_cap
  dlcs_axpby (axpby/cast/scaled_copy)  test_axpby, test_grid_stride_over_launch_cap
  dlcs_relu_grad                       test_relu_grad, test_grid_stride_over_launch_cap
  dlcs_fill_bias                       test_fill_bias
  dlcs_cast_multi_bf16                 test_cast_multi_bf16
  dlcs_gather_rows                     test_gather_rows, test_grid_stride_over_launch_cap
  dlcs_colsum                          test_colsum, test_colsum_unaligned
  dlcs_layernorm_fwd / _bwd            test_layernorm_paths, test_layernorm_null_grads,
                                       test_layernorm_atomic_fallback,
                                       test_layernorm_workspace_short, test_layernorm_refuses_c513
  dlcs_conv3d_thin_im2col              test_thin_im2col, test_thin_conv_end_to_end
  dlcs_conv3d_thin_col2im              test_thin_col2im, test_thin_conv_end_to_end
  dlcs_scale_rows                      test_scale_rows
  dlcs_rows_add                        test_rows_add
  dlcs_dit_vec (ops 0-3)               test_dit_vec
  dlcs_timestep_embedding (odd dim)    test_timestep_embedding_odd_dim
  dlcs_gemm (N = 1, M = 1, K = 1)      test_gemm_degenerate
"""
import math

import pytest
import torch
import torch.nn.functional as F

from goldutil import nrmse

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
PAIRS = [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)]
PAIR_IDS = ["f32-f32", "f32-bf16", "bf16-f32", "bf16-bf16"]
GUARD = 64                      # sentinel elements before and after every output
SENT = -12345.0
N_BIG = 2097152 + 8 * 3 + 5     # just over the 8192 x 256 launch cap of grid_for()


def _K():
    from dl_cs.models import _ops as K
    return K


def _call(name, *args):
    from dl_cs import _lib
    _lib.call(name, *args)


def _err():
    from dl_cs import _lib
    return _lib.DlcsError


def _rnd(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g)


def _perm(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))


class _Out:
    """An output buffer between two GUARD-element sentinel margins.  `t` is the device
    view a kernel writes (init: a tensor or a fill value; else the sentinel); get() checks
    both margins and returns the CPU copy."""

    def __init__(self, shape, dtype=F32, init=None):
        shape = tuple(int(s) for s in shape)
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if torch.is_tensor(init):
            self.t.copy_(init.reshape(shape))
        elif init is not None:
            self.t.fill_(init)

    def get(self):
        b = self.buf.cpu()
        s = torch.full((GUARD,), SENT, dtype=b.dtype)
        assert torch.equal(b[:GUARD], s), "write before the output buffer"
        assert torch.equal(b[b.numel() - GUARD:], s), "write past the output buffer"
        return b[GUARD:b.numel() - GUARD].view(self.t.shape).clone()


def _sent(shape, dtype=F32):
    return torch.full(shape, SENT, dtype=dtype)


def _to_blocked(x):
    """[B, C, D, H, W] (D, H, W multiples of 4) -> blocked rows [B*D*H*W, C] (layout.hip)."""
    B, C, D, H, W = x.shape
    t = x.permute(0, 2, 3, 4, 1).reshape(B, D // 4, 4, H // 4, 4, W // 4, 4, C)
    return t.permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(-1, C)


def _from_blocked(r, B, C, D, H, W):
    t = r.reshape(B, D // 4, H // 4, W // 4, 4, 4, 4, C).permute(0, 1, 4, 2, 5, 3, 6, 7)
    return t.reshape(B, D, H, W, C).permute(0, 4, 1, 2, 3)


def _pad_cols(r, ld):
    return F.pad(r, (0, ld - r.shape[1]))


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


# ============================================================================ 1. boundary
# (B, E, Tn, Y, X, pad, ldc)
_PRE_CASES = [(1, 2, 6, 8, 4, 1, 8), (2, 1, 2, 4, 8, 1, 8), (1, 2, 4, 4, 4, 2, 4), (1, 3, 8, 4, 12, 0, 16),
              (1, 2, 10, 8, 8, 3, 8),
              (1, 1, 4, 4, 4, 4, 8)]            # pad = Tn: every frame appears three times
_pre_params = pytest.mark.parametrize("case", _PRE_CASES, ids=lambda c: "x".join(map(str, c)))
_dt_params = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])


def _crnd(shape, seed, dtype=None):
    re, im = _rnd(shape, seed), _rnd(shape, seed + 1000)
    if dtype is not None:                        # representable in `dtype`
        re, im = re.to(dtype).float(), im.to(dtype).float()
    return torch.complex(re, im)


def _pre_ref(xr, pad, ldc):
    """xr real [B, 2E, T, Y, X] -> circular time pad -> blocked rows [.., ldc], pad channels 0."""
    u = F.pad(xr, (0, 0, 0, 0, pad, pad), mode="circular") if pad else xr
    return _pad_cols(_to_blocked(u), ldc)


def _post_ref(o, shape, pad):
    """o blocked rows [.., ldc] -> real [B, 2E, T, Y, X]: crop [pad, pad + T) of channels < 2E."""
    B, E, T, Y, X = shape
    return _from_blocked(o, B, o.shape[1], T + 2 * pad, Y, X)[:, :2 * E, pad:pad + T]


def _swin_pre(x, dtype, pad, ldc):
    K = _K()
    B, E, T, Y, X = x.shape
    xd = x.to(DEV).contiguous()
    u = _Out((B * (T + 2 * pad) * Y * X, ldc), dtype)
    _call("dlcs_swin_pre", K.code(dtype), K.p(xd), K.p(u.t), B, E, T, Y, X, pad, ldc, K.S())
    return u.get()


def _swin_pre_bwd(gu, shape, pad):
    K = _K()
    B, E, T, Y, X = shape
    gd = gu.to(DEV).contiguous()
    gx = _Out(tuple(shape) + (2,))
    _call("dlcs_swin_pre_bwd", K.code(gd), K.p(gd), K.p(gx.t), B, E, T, Y, X, pad, gu.shape[1], K.S())
    return torch.view_as_complex(gx.get())


def _swin_post(o, shape, pad):
    K = _K()
    B, E, T, Y, X = shape
    od = o.to(DEV).contiguous()
    out = _Out(tuple(shape) + (2,))
    _call("dlcs_swin_post", K.code(od), K.p(od), K.p(out.t), B, E, T, Y, X, pad, o.shape[1], K.S())
    return torch.view_as_complex(out.get())


def _swin_post_bwd(gout, dtype, pad, ldc):
    K = _K()
    B, E, T, Y, X = gout.shape
    gd = gout.to(DEV).contiguous()
    go = _Out((B * (T + 2 * pad) * Y * X, ldc), dtype)
    _call("dlcs_swin_post_bwd", K.code(dtype), K.p(gd), K.p(go.t), B, E, T, Y, X, pad, ldc, K.S())
    return go.get()


def _real2(z):
    return torch.cat([z.real, z.imag], 1)


def _cplx(v, E):
    return torch.complex(v[:, :E].contiguous(), v[:, E:].contiguous())


def _rel_close(a, b, rel):
    return abs(a - b) <= rel * max(abs(a), abs(b))


@_dt_params
@_pre_params
def test_swin_pre(case, dtype):
    B, E, T, Y, X, pad, ldc = case
    x = _crnd((B, E, T, Y, X), 1)
    u = _swin_pre(x, dtype, pad, ldc)
    ref = _pre_ref(_real2(x), pad, ldc)
    assert torch.equal(u, ref.to(dtype))
    assert not u[:, 2 * E:].any()                # channels [2E, ldc) exactly zero


@_dt_params
@_pre_params
def test_swin_pre_bwd(case, dtype):
    """The circular-pad adjoint.  Where every frame appears at most twice the fp32 sum has
    one rounding and equals the fp32 autograd gradient bit for bit."""
    B, E, T, Y, X, pad, ldc = case
    shape = (B, E, T, Y, X)
    gu = _rnd((B * (T + 2 * pad) * Y * X, ldc), 2).to(dtype)     # non-zero in the pad channels too
    gx = _swin_pre_bwd(gu, shape, pad)
    grads = []
    for ft in (torch.float64, F32):
        xr = torch.zeros((B, 2 * E, T, Y, X), dtype=ft, requires_grad=True)
        (_pre_ref(xr, pad, ldc) * gu.to(ft)).sum().backward()
        grads.append(_cplx(xr.grad, E))
    assert nrmse(grads[0].numpy(), gx.numpy()) < 1e-6
    if T + 2 * pad <= 2 * T:
        assert torch.equal(gx, grads[1])
    # <pre(x), g> = <x, pre_bwd(g)> in float64 on the kernels' outputs (x representable in
    # bf16, so that pre itself does not round)
    xq = _crnd(shape, 3, BF16)
    u = _swin_pre(xq, dtype, pad, ldc)
    lhs = float((u.double() * gu.double()).sum())
    rhs = float((_real2(xq).double() * _real2(gx).double()).sum())
    assert _rel_close(lhs, rhs, 1e-6), (lhs, rhs)


@_dt_params
@_pre_params
def test_swin_post(case, dtype):
    B, E, T, Y, X, pad, ldc = case
    shape = (B, E, T, Y, X)
    o = _rnd((B * (T + 2 * pad) * Y * X, ldc), 4).to(dtype)
    out = _swin_post(o, shape, pad)
    assert torch.equal(out, _cplx(_post_ref(o.float(), shape, pad), E))


@_dt_params
@_pre_params
def test_swin_post_bwd(case, dtype):
    B, E, T, Y, X, pad, ldc = case
    shape = (B, E, T, Y, X)
    rows = B * (T + 2 * pad) * Y * X
    gout = _crnd(shape, 5)
    go = _swin_post_bwd(gout, dtype, pad, ldc)
    o = torch.zeros((rows, ldc), dtype=torch.float64, requires_grad=True)
    (_post_ref(o, shape, pad) * _real2(gout).double()).sum().backward()
    assert torch.equal(go, o.grad.float().to(dtype))             # a scatter: no arithmetic
    inside = _from_blocked(go.float(), B, ldc, T + 2 * pad, Y, X)
    assert not inside[:, 2 * E:].any()                           # channels >= 2E
    assert not inside[:, :, :pad].any() and not inside[:, :, pad + T:].any()   # rows outside the crop
    # <post(o), g> = <o, post_bwd(g)> (g representable in bf16, so that post_bwd does not round)
    gq = _crnd(shape, 6, BF16)
    ov = _rnd((rows, ldc), 7).to(dtype)
    out = _swin_post(ov, shape, pad)
    goq = _swin_post_bwd(gq, dtype, pad, ldc)
    lhs = float((_real2(out).double() * _real2(gq).double()).sum())
    rhs = float((ov.double() * goq.double()).sum())
    assert _rel_close(lhs, rhs, 1e-6), (lhs, rhs)


# ============================================================================ 2. block layout
def _block_layout(src, dst_dtype, dims, ld, inverse):
    K = _K()
    B, C, D, H, W = dims
    sd = src.to(DEV).contiguous()
    rows = B * ((D + 3) // 4) * ((H + 3) // 4) * ((W + 3) // 4) * 64
    out = _Out((B, C, D, H, W) if inverse else (rows, ld), dst_dtype)
    _call("dlcs_block_layout", K.code(sd), K.code(dst_dtype), K.p(sd), K.p(out.t), B, C, D, H, W, ld, int(inverse),
          K.S())
    return out.get()


def _to_blocked_pad(x, ld):
    """Zero-pad the grid of [B, C, D, H, W] to multiples of 4, block, zero-pad the columns to ld."""
    _, _, D, H, W = x.shape
    return _pad_cols(_to_blocked(F.pad(x, (0, -W % 4, 0, -H % 4, 0, -D % 4))), ld)


@pytest.mark.parametrize("ti,to", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("dims,ld", [((1, 4, 5, 6, 7), 8), ((2, 3, 4, 4, 4), 3), ((1, 160, 3, 9, 2), 160),
                                     ((1, 1, 1, 1, 1), 8)])
def test_block_layout(dims, ld, ti, to):
    x = _rnd(dims, 10).to(ti)
    ref = _to_blocked_pad(x.float(), ld)
    fwd = _block_layout(x, to, dims, ld, 0)
    assert torch.equal(fwd, ref.to(to))
    real = _to_blocked_pad(torch.ones(dims), ld) != 0            # real voxels and channels
    assert not fwd[~real].any()                                  # pad voxels, columns [C, ld)
    # round trip on values both dtypes hold exactly
    xq = _rnd(dims, 11).to(BF16).to(ti)
    back = _block_layout(_block_layout(xq, to, dims, ld, 0), ti, dims, ld, 1)
    assert torch.equal(back, xq)
    # the crop reads real voxels only
    poisoned = torch.where(real, fwd, torch.full_like(fwd, float("nan")))
    got = _block_layout(poisoned, ti, dims, ld, 1)
    assert not torch.isnan(got).any()
    assert torch.equal(got, x.float().to(to).to(ti))
    # the module-level wrappers reach the same kernel
    from dl_cs.models import _standalone as SA
    assert torch.equal(SA.to_blocked(x.to(DEV), ld, to).cpu(), fwd)
    assert torch.equal(SA.from_blocked(fwd.to(DEV), dims, ti).cpu(), got)


# ============================================================================ 3. elementwise
def _permute(src, dst_shape, strides, dst_dtype, dst0=None):
    K = _K()
    sd = src.to(DEV).contiguous()
    out = _Out(dst_shape, dst_dtype, init=dst0)
    K.permute(sd, tuple(dst_shape), tuple(strides), out=out.t, accumulate=int(dst0 is not None))
    return out.get()


def _permute_ref(src, dst_shape, strides, dst_dtype, dst0=None):
    v = torch.as_strided(src, tuple(dst_shape), tuple(strides)).float()
    if dst0 is not None:
        v = v + dst0.float()
    return v.to(dst_dtype)


def _perm_patterns():
    C, D, cin, Cpe = 8, 8, 4, 3
    B, E, nT, nY, nX = 2, 3, 2, 3, 2
    return {
        # name: (source shape, dst shape, source strides, accumulate)
        "patchgan:102 patch weight": ((C, C, 4, 4, 4), (C, 4, 4, 4, C), (C * 64, 16, 4, 1, 64), 0),
        "patchgan:155 patch wgrad": ((C, 64 * C), (C, C, 4, 4, 4), (64 * C, 1, 16 * C, 4 * C, C), 1),
        "dit_engine:429 patch embed": ((D, Cpe, 32), (D, 32, Cpe), (Cpe * 32, 1, 32), 0),
        "dit_engine:523 final conv": ((cin, D, 27), (27, cin, D), (1, D * 27, 27), 0),
        "dit_engine:565 final wgrad": ((27 * cin, D), (cin, D, 27), (D, 1, cin * D), 1),
        "_standalone:116 tokens": ((B * nT * nY * nX, E), (B, E, nT, nY, nX),
                                   (nT * nY * nX * E, 1, nY * nX * E, nX * E, E), 0),
        "patchgan:102 C=3": ((3, 3, 4, 4, 4), (3, 4, 4, 4, 3), (3 * 64, 16, 4, 1, 64), 0),
    }


@pytest.mark.parametrize("ti,to", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name", list(_perm_patterns()))
def test_permute_model_patterns(name, ti, to):
    sshape, dshape, strides, acc = _perm_patterns()[name]
    src = _rnd(sshape, 20).to(ti)
    dst0 = _rnd(dshape, 21).to(to) if acc else None
    assert torch.equal(_permute(src, dshape, strides, to, dst0), _permute_ref(src, dshape, strides, to, dst0))


@pytest.mark.parametrize("ti,to", PAIRS, ids=PAIR_IDS)
def test_permute_6d_1d(ti, to):
    src = _rnd((2, 3, 2, 5, 3, 2), 22).to(ti)
    order = (4, 0, 5, 2, 1, 3)
    dshape = tuple(src.shape[k] for k in order)
    strides = tuple(src.stride(k) for k in order)
    ref = _permute_ref(src, dshape, strides, to)
    assert torch.equal(ref, src.permute(order).float().to(to))
    assert torch.equal(_permute(src, dshape, strides, to), ref)
    dst0 = _rnd(dshape, 23).to(to)
    assert torch.equal(_permute(src, dshape, strides, to, dst0), _permute_ref(src, dshape, strides, to, dst0))
    v = _rnd((777,), 24).to(ti)
    assert torch.equal(_permute(v, (777,), (1,), to), v.float().to(to))
    assert torch.equal(_permute(v, (259,), (3,), to), v[::3].float().to(to))


@pytest.mark.parametrize("tx,ty", PAIRS, ids=PAIR_IDS)
def test_axpby(tx, ty):
    K = _K()
    for n in (1, 255, 256, 1000):
        x = _rnd((n,), 30 + n).to(tx)
        y0 = _rnd((n,), 31 + n).to(ty)
        xd = x.to(DEV)
        for a, b in ((1.0, 0.0), (-0.5, 0.0), (2.0, 1.0), (0.25, -3.0)):
            # with b = 0 the kernel must not read y: it starts as NaN
            y = _Out((n,), ty, init=y0 if b else float("nan"))
            K.axpby(xd, y.t, a, b)
            got = y.get()
            if b == 0.0:
                assert torch.isfinite(got.float()).all()
                assert torch.equal(got, (a * x.float()).to(ty)), (n, a, b)
            else:
                # the same fp32 expression: two products, one sum, each rounded (measured: the
                # kernel's a x + b y is not contracted into an FMA)
                assert torch.equal(got, (a * x.float() + b * y0.float()).to(ty)), (n, a, b)
    # the wrappers built on it
    x = _rnd((1000,), 32)
    assert torch.equal(K.cast(x.to(DEV), BF16).cpu(), x.to(BF16))
    assert torch.equal(K.cast(x.to(BF16).to(DEV), F32).cpu(), x.to(BF16).float())
    assert torch.equal(K.scaled_copy(x.to(DEV), BF16, -0.5).cpu(), (-0.5 * x).to(BF16))
    assert torch.equal(K.scaled_copy(x.to(DEV), F32, 3.0).cpu(), 3.0 * x)


def _relu_operand(n, seed, shift=0):
    """Activations with exact zeros, -0.0, NaN and negatives at fixed positions."""
    a = _rnd((n,), seed).abs() + 0.125
    k = (torch.arange(n) + shift) % 6
    a[k == 1] = 0.0
    a[k == 2] = -0.0
    a[k == 3] = float("nan")
    a[k == 4] *= -1.0
    return a


@pytest.mark.parametrize("tg,ta", PAIRS, ids=PAIR_IDS)
def test_relu_grad(tg, ta):
    K = _K()
    for n in (1, 7, 8, 9, 2055):
        for shift in (0, 3):
            a = _relu_operand(n, 40 + n, shift).to(ta)
            g0 = _rnd((n,), 41 + n).to(tg)
            g = _Out((n,), tg, init=g0)
            K.relu_grad(g.t, a.to(DEV))
            got = g.get()
            keep = a.float() > 0                                 # NaN, 0.0, -0.0 and negatives: not kept
            ref = torch.where(keep, g0, torch.zeros_like(g0))
            assert torch.equal(_bits(got), _bits(ref)), (n, shift)
            assert torch.equal(_bits(got[keep]), _bits(g0[keep])), (n, shift)


@pytest.mark.parametrize("rows,C,period", [(1, 640, 10), (3, 12, 12), (5, 7, 7)])
def test_fill_bias(rows, C, period):
    K = _K()
    bias = _rnd((period,), 50)
    out = _Out((rows, C))
    K.fill_bias(out.t, bias.to(DEV), rows, C, period)
    assert torch.equal(out.get(), bias[torch.arange(C) % period].expand(rows, C))
    out = _Out((rows, C))
    K.fill_bias(out.t, None, rows, C, period)
    assert torch.equal(out.get(), torch.zeros((rows, C)))


def test_cast_multi_bf16():
    import ctypes
    K = _K()
    assert K.cast_multi_bf16([]) == []
    _call("dlcs_cast_multi_bf16", 0, None, None, None, K.S())    # count 0: nothing to read
    (one,) = K.cast_multi_bf16([_rnd((3, 1025), 60).to(DEV)])
    assert torch.equal(one.cpu(), _rnd((3, 1025), 60).to(BF16))
    sizes = [(0, 1, 1023, 1025, 5000)[(3 * i + i // 5) % 5] for i in range(65)]
    assert set(sizes) == {0, 1, 1023, 1025, 5000} and len(set(sizes[:64])) == 5
    srcs = [_rnd((n,), 61 + i) for i, n in enumerate(sizes)]
    outs = K.cast_multi_bf16([s.to(DEV) for s in srcs])          # 64 + 1: two launches
    assert len(outs) == 65
    for i, (s, o) in enumerate(zip(srcs, outs)):
        assert o.dtype == BF16 and torch.equal(o.cpu(), s.to(BF16)), i
    # guarded destinations, sizes on both sides of the 1024-element launch granule
    ns = [1023, 0, 1025, 1]
    sd = [_rnd((n,), 70 + i).to(DEV) for i, n in enumerate(ns)]
    dst = [_Out((n,), BF16) for n in ns]
    k = len(ns)
    _call("dlcs_cast_multi_bf16", k, (ctypes.c_void_p * k)(*[K.p(t) for t in sd]),
          (ctypes.c_void_p * k)(*[K.p(d.t) for d in dst]), (ctypes.c_int64 * k)(*ns), K.S())
    for s, d in zip(sd, dst):
        assert torch.equal(d.get(), s.cpu().to(BF16))


@pytest.mark.parametrize("ti,to", PAIRS, ids=PAIR_IDS)
def test_gather_rows(ti, to):
    K = _K()
    nsrc, ld_src, C, nrows = 37, 11, 8, 50
    src = _rnd((nsrc, ld_src), 80).to(ti)
    sd = src.to(DEV)
    idx = torch.randint(0, nsrc, (nrows,), generator=torch.Generator().manual_seed(81)).to(torch.int32)
    idx[5] = idx[6] = idx[40] = 3                                 # repeats
    idx[[0, 17, 49]] = -1
    ref = torch.where(idx[:, None] >= 0, src[idx.clamp(min=0).long(), :C].float(), torch.zeros(1)).to(to)
    # C below the source's row length, destination exactly C wide
    out = _Out((nrows, C), to)
    K.gather_rows(sd, idx.to(DEV), nrows, to, C=C, out=out.t)
    assert torch.equal(out.get(), ref)
    # destination wider than C: columns [C, C + 3) keep what they held
    out = _Out((nrows, C + 3), to)
    K.gather_rows(sd, idx.to(DEV), nrows, to, C=C, out=out.t)
    got = out.get()
    assert torch.equal(got[:, :C], ref)
    assert torch.equal(got[:, C:], _sent((nrows, 3), to))
    # idx = None is the identity; full rows
    out = _Out((nsrc, ld_src), to)
    K.gather_rows(sd, None, nsrc, to, out=out.t)
    assert torch.equal(out.get(), src.float().to(to))
    assert torch.equal(K.gather_rows(sd, idx.to(DEV), nrows, to).cpu(),
                       torch.where(idx[:, None] >= 0, src[idx.clamp(min=0).long()].float(), torch.zeros(1)).to(to))


@pytest.mark.parametrize("kernel", ["axpby", "relu_grad", "permute", "gather_rows"])
def test_grid_stride_over_launch_cap(kernel):
    """n = 2,097,181 elements: 29 more than the 8192 x 256 threads a launch is capped at,
    so the last elements are reached only through the grid-stride loop (and relu_grad's
    scalar tail starts past the cap).  fp32, exact."""
    K = _K()
    n = N_BIG
    x = _rnd((n,), 90)
    if kernel == "axpby":
        y0 = _rnd((n,), 91)
        y = _Out((n,), init=y0)
        K.axpby(x.to(DEV), y.t, 2.0, 1.0)
        assert torch.equal(y.get(), 2.0 * x + y0)
    elif kernel == "relu_grad":
        a = _relu_operand(n, 92)
        g = _Out((n,), init=x)
        K.relu_grad(g.t, a.to(DEV))
        assert torch.equal(_bits(g.get()), _bits(torch.where(a > 0, x, torch.zeros_like(x))))
    elif kernel == "permute":
        assert torch.equal(_permute(x, (n,), (1,), F32), x)
    else:
        idx = _perm(n, 93).to(torch.int32)
        out = _Out((n, 1))
        K.gather_rows(x.view(n, 1).to(DEV), idx.to(DEV), n, F32, C=1, out=out.t)
        assert torch.equal(out.get()[:, 0], x[idx.long()])


# ============================================================================ 4. colsum
def _colsum_check(xd, x, rows, C, ld):
    """xd: device operand [rows, ld] whose columns [C, ld) hold 1e30; x its CPU copy."""
    K = _K()
    out0 = _rnd((C,), 101)
    out = _Out((C,), init=out0)                                  # the kernel accumulates
    K.colsum(xd, out.t, rows=rows, C=C, ld=ld)
    ref = out0.double() + x[:, :C].double().sum(0)
    assert nrmse(ref.numpy(), out.get().double().numpy()) < 1e-6


def _colsum_operand(rows, C, ld, dtype):
    x = _rnd((rows, ld), 100)
    x[:, C:] = 1e30                                              # a read of the pad columns shows
    return x.to(dtype)


@_dt_params
@pytest.mark.parametrize("rows,C,ld", [(1, 8, 8), (63, 160, 160), (257, 160, 160), (1000, 4, 8), (300, 12, 16),
                                       (70, 2048, 2048), (40, 2056, 2056), (129, 5, 5)])
def test_colsum(rows, C, ld, dtype):
    """Vector kernel (ld % 8 == 0, C <= 2048) with 1 .. 256 row groups and C % 8 != 0; the
    scalar kernel on C = 2056 and on ld = 5."""
    x = _colsum_operand(rows, C, ld, dtype)
    _colsum_check(x.to(DEV), x, rows, C, ld)


@_dt_params
@pytest.mark.parametrize("rows,C,ld", [(257, 160, 160), (300, 12, 16)])
def test_colsum_unaligned(rows, C, ld, dtype):
    """The same operand 4 bytes into a larger buffer: not 16-byte aligned, the scalar kernel."""
    x = _colsum_operand(rows, C, ld, dtype)
    off = 1 if dtype == F32 else 2
    buf = torch.zeros((rows * ld + 8,), dtype=dtype, device=DEV)
    xd = buf[off:off + rows * ld].view(rows, ld)
    xd.copy_(x)
    assert xd.data_ptr() % 16 == 4
    _colsum_check(xd, x, rows, C, ld)


# ============================================================================ 5. LayerNorm
_LN_C = [32, 64, 65, 128, 160, 256, 257, 384, 512]     # KM = 1, 1, 2, 2, 3, 4, generic x 3
_LN_SHAPES = [(17, C) for C in _LN_C] + [(r, C) for C in (160, 384) for r in (1, 15, 16, 500)]


def _ln_inputs(rows, C, mapped):
    """x [nsrc, C], gamma, beta, dy [rows, C] and the row map: with `mapped`, `rows` output
    rows of which npad are zero-pad rows (-1) and the rest a bijection onto the nsrc source
    rows (the window partition of padded tokens)."""
    if mapped:
        npad = 0 if rows == 1 else max(1, rows // 8)
        nsrc = rows - npad
        idx = torch.full((rows,), -1, dtype=torch.int32)
        idx[_perm(rows, 110)[:nsrc]] = _perm(nsrc, 111).to(torch.int32)
    else:
        nsrc, idx = rows, None
    x = 0.5 + 1.5 * _rnd((nsrc, C), 112)
    gam, bet = 1 + 0.1 * _rnd((C,), 113), 0.1 * _rnd((C,), 114)
    return x, gam, bet, _rnd((rows, C), 115), idx


def _ln_reference(x, gam, bet, dy, idx, eps):
    """float64 F.layer_norm with autograd, as test_layernorm_gather."""
    C = x.shape[1]
    xr = x.double().requires_grad_()
    g_, b_ = gam.double().requires_grad_(), bet.double().requires_grad_()
    if idx is None:
        xs, keep = xr, torch.ones((x.shape[0], 1), dtype=torch.float64)
    else:
        xs, keep = xr[idx.clamp(min=0).long()], (idx >= 0).double()[:, None]
    o = F.layer_norm(xs, (C,), g_, b_, eps)
    (o * dy.double() * keep).sum().backward()
    xs = xs.detach()
    mean = xs.mean(1) * keep[:, 0]
    rstd = (xs.var(1, unbiased=False) + eps).rsqrt() * keep[:, 0]
    return dict(out=o.detach() * keep, mean=mean, rstd=rstd, dx=xr.grad, dg=g_.grad, db=b_.grad)


def _ln_fwd(x, gam, bet, idx, rows, eps, dtype):
    K = _K()
    C = x.shape[1]
    xd, gd, bd = x.to(DEV), gam.to(DEV), bet.to(DEV)
    idd = None if idx is None else idx.to(DEV)
    out, mean, rstd = _Out((rows, C), dtype), _Out((rows,)), _Out((rows,))
    _call("dlcs_layernorm_fwd", K.code(dtype), K.p(xd), K.p(idd), K.p(gd), K.p(bd), float(eps), K.p(out.t),
          K.p(mean.t), K.p(rstd.t), rows, C, K.S())
    return out.get(), mean.get(), rstd.get()


def _ln_bwd(x, gam, dy, idx, mean, rstd, dx, dx_in=None, dg=None, db=None, workspace="full"):
    """dlcs_layernorm_bwd into the _Out buffers dx / dg / db; workspace "full" (NaN-filled:
    it carries nothing in), "short" (one byte less than asked for) or None."""
    from dl_cs import _lib
    K = _K()
    rows, C = dy.shape
    t = [v.to(DEV) for v in (dy, x, gam, mean, rstd)]
    idd = None if idx is None else idx.to(DEV)
    din = None if dx_in is None else dx_in.to(DEV)
    nb = int(_lib.lib().dlcs_layernorm_bwd_workspace_bytes(rows, C))
    ws = torch.full((max(1, nb // 4),), float("nan"), device=DEV)
    wp, wn = (None, 0) if workspace is None else (K.p(ws), nb - (workspace == "short"))
    _call("dlcs_layernorm_bwd", K.p(t[0]), K.p(t[1]), K.p(idd), K.p(t[2]), K.p(t[3]), K.p(t[4]), K.p(din),
          K.p(dx.t), None if dg is None else K.p(dg.t), None if db is None else K.p(db.t), rows, C, wp, wn, K.S())
    torch.cuda.synchronize()


def _ln_close(ref, got):
    return nrmse(ref.numpy(), got.double().numpy()) < 1e-6


@pytest.mark.parametrize("mapped", [False, True], ids=["plain", "src_map"])
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("rows,C", _LN_SHAPES)
def test_layernorm_paths(rows, C, eps, mapped):
    x, gam, bet, dy, idx = _ln_inputs(rows, C, mapped)
    R = _ln_reference(x, gam, bet, dy, idx, eps)
    pad = torch.zeros(rows, dtype=torch.bool) if idx is None else idx < 0
    out, mean, rstd = _ln_fwd(x, gam, bet, idx, rows, eps, F32)
    assert _ln_close(R["out"], out)
    assert _ln_close(R["mean"], mean) and _ln_close(R["rstd"], rstd)
    # zero-pad rows: mean = rstd = 0 and an all-zero row, exactly
    assert not out[pad].any() and not mean[pad].any() and not rstd[pad].any()
    # bf16 output: the fp32 result rounded to nearest, at most 2^-9 relative per element
    outb, meanb, rstdb = _ln_fwd(x, gam, bet, idx, rows, eps, BF16)
    assert nrmse(R["out"].numpy(), outb.double().numpy()) < 2e-3
    assert torch.equal(meanb, mean) and torch.equal(rstdb, rstd) and not outb[pad].any()
    dx0, dg0, db0 = _rnd(x.shape, 116), _rnd((C,), 117), _rnd((C,), 118)
    # (a) dx_in = NULL: dx += dLN/dx on a non-zero dx; dgamma / dbeta accumulate
    dx, dg, db = _Out(x.shape, init=dx0), _Out((C,), init=dg0), _Out((C,), init=db0)
    _ln_bwd(x, gam, dy, idx, mean, rstd, dx, None, dg, db)
    assert _ln_close(dx0.double() + R["dx"], dx.get())
    assert _ln_close(dg0.double() + R["dg"], dg.get())
    assert _ln_close(db0.double() + R["db"], db.get())
    # (b) dx = dx_in + dLN/dx: dx starts as NaN and is not read
    dx, dg, db = _Out(x.shape, init=float("nan")), _Out((C,), init=dg0), _Out((C,), init=db0)
    _ln_bwd(x, gam, dy, idx, mean, rstd, dx, dx0, dg, db)
    assert _ln_close(dx0.double() + R["dx"], dx.get())
    assert _ln_close(dg0.double() + R["dg"], dg.get())
    assert _ln_close(db0.double() + R["db"], db.get())


@pytest.mark.parametrize("rows,C", [(17, 160), (17, 384)])
def test_layernorm_null_grads(rows, C):
    """dgamma = dbeta = NULL, and one of them alone."""
    x, gam, bet, dy, idx = _ln_inputs(rows, C, True)
    R = _ln_reference(x, gam, bet, dy, idx, 1e-5)
    _, mean, rstd = _ln_fwd(x, gam, bet, idx, rows, 1e-5, F32)
    dx = _Out(x.shape, init=0.0)
    _ln_bwd(x, gam, dy, idx, mean, rstd, dx)
    assert _ln_close(R["dx"], dx.get())
    dx, db = _Out(x.shape, init=0.0), _Out((C,), init=0.0)
    _ln_bwd(x, gam, dy, idx, mean, rstd, dx, db=db)
    assert _ln_close(R["dx"], dx.get()) and _ln_close(R["db"], db.get())
    dx, dg = _Out(x.shape, init=0.0), _Out((C,), init=0.0)
    _ln_bwd(x, gam, dy, idx, mean, rstd, dx, dg=dg)
    assert _ln_close(R["dx"], dx.get()) and _ln_close(R["dg"], dg.get())


@pytest.mark.parametrize("rows,C", [(500, 160), (17, 64), (100, 256)])
def test_layernorm_atomic_fallback(rows, C):
    """A NULL workspace: the column partials go to dgamma / dbeta through fp32 atomics."""
    x, gam, bet, dy, idx = _ln_inputs(rows, C, True)
    R = _ln_reference(x, gam, bet, dy, idx, 1e-5)
    _, mean, rstd = _ln_fwd(x, gam, bet, idx, rows, 1e-5, F32)
    got = {}
    for ws in ("full", None):
        dx, dg, db = _Out(x.shape, init=0.0), _Out((C,), init=0.0), _Out((C,), init=0.0)
        _ln_bwd(x, gam, dy, idx, mean, rstd, dx, None, dg, db, workspace=ws)
        got[ws] = (dx.get(), dg.get(), db.get())
    for k, name in enumerate(("dx", "dg", "db")):
        assert _ln_close(R[name], got[None][k]), name
        assert _ln_close(got["full"][k].double(), got[None][k]), name
    assert torch.equal(got["full"][0], got[None][0])             # dx does not depend on the workspace


def test_layernorm_workspace_short():
    rows, C = 17, 160
    x, gam, bet, dy, idx = _ln_inputs(rows, C, False)
    _, mean, rstd = _ln_fwd(x, gam, bet, idx, rows, 1e-5, F32)
    dx, dg, db = _Out(x.shape), _Out((C,)), _Out((C,))
    with pytest.raises(_err(), match="100003"):                  # DLCS_ERR_WORKSPACE
        _ln_bwd(x, gam, dy, idx, mean, rstd, dx, None, dg, db, workspace="short")
    assert torch.equal(dx.get(), _sent(x.shape)) and torch.equal(dg.get(), _sent((C,)))
    assert torch.equal(db.get(), _sent((C,)))


def test_layernorm_refuses_c513():
    rows, C = 4, 513
    x, gam, bet, dy, idx = _ln_inputs(rows, C, False)
    with pytest.raises(_err(), match="100001"):                  # DLCS_ERR_INVALID_ARG
        _ln_fwd(x, gam, bet, idx, rows, 1e-5, F32)
    dx = _Out(x.shape)
    with pytest.raises(_err(), match="100001"):
        _ln_bwd(x, gam, dy, idx, torch.zeros(rows), torch.ones(rows), dx, None, _Out((C,)), _Out((C,)))
    assert torch.equal(dx.get(), _sent(x.shape))


# ============================================================================ 6. DiT glue
def _tap_shift(rows, grid, tap, sign):
    """rows [V, C] blocked on grid (B, D, H, W) -> [V, C] whose row v is rows[v + sign * off(tap)],
    off(tap) = (kd - 1, kh - 1, kw - 1), tap = 9 kd + 3 kh + kw; zero outside the grid."""
    B, D, H, W = grid
    C = rows.shape[1]
    xp = F.pad(_from_blocked(rows, B, C, D, H, W), (1, 1, 1, 1, 1, 1))
    dt, dy, dx = (sign * (tap // 9 - 1), sign * ((tap // 3) % 3 - 1), sign * (tap % 3 - 1))
    return _to_blocked(xp[:, :, 1 + dt:1 + dt + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W])


def _im2col(src, C, grid, sign, ld_dst):
    K = _K()
    B, D, H, W = grid
    sd = src.to(DEV).contiguous()
    dst = _Out((B * D * H * W, ld_dst))
    _call("dlcs_conv3d_thin_im2col", K.p(sd), src.shape[1], C, K.p(dst.t), ld_dst, int(sign), B, D, H, W, K.S())
    return dst.get()


def _col2im(P, C, grid, sign, ld_out, bias=None, out0=None):
    K = _K()
    B, D, H, W = grid
    pd = P.to(DEV).contiguous()
    bd = None if bias is None else bias.to(DEV)
    out = _Out((B * D * H * W, ld_out), init=out0)
    _call("dlcs_conv3d_thin_col2im", K.p(pd), P.shape[1], C, K.p(out.t), ld_out, K.p(bd), int(sign),
          int(out0 is not None), B, D, H, W, K.S())
    return out.get()


_THIN_GRIDS = [(1, 4, 4, 4), (2, 4, 8, 4), (1, 8, 4, 12)]
_thin_params = pytest.mark.parametrize("grid", _THIN_GRIDS, ids=lambda g: "x".join(map(str, g)))


@_thin_params
@pytest.mark.parametrize("C", [1, 4, 8])
def test_thin_im2col(C, grid):
    V = math.prod(grid)
    src = _rnd((V, C + 3), 120)                                  # ld_src > C: the pad columns are never copied
    for sign in (1, -1):
        ref = torch.cat([_tap_shift(src[:, :C], grid, tap, sign) for tap in range(27)], 1)
        for ld_dst in (27 * C, 27 * C + 5):
            got = _im2col(src, C, grid, sign, ld_dst)
            assert torch.equal(got[:, :27 * C], ref), (sign, ld_dst)
            assert not got[:, 27 * C:].any()                     # columns [27 C, ld_dst) exactly zero


def test_thin_unsupported_grid():
    """A grid that is not a multiple of 4 is DLCS_ERR_UNSUPPORTED_SIZE, nothing written."""
    K = _K()
    grid, C = (1, 4, 6, 4), 4
    V = math.prod(grid)
    src, P = torch.zeros((V, C), device=DEV), torch.zeros((V, 27 * C), device=DEV)
    dst, out = _Out((V, 27 * C)), _Out((V, C))
    with pytest.raises(_err(), match="100002"):
        _call("dlcs_conv3d_thin_im2col", K.p(src), C, C, K.p(dst.t), 27 * C, 1, *grid, K.S())
    with pytest.raises(_err(), match="100002"):
        _call("dlcs_conv3d_thin_col2im", K.p(P), 27 * C, C, K.p(out.t), C, None, 1, 0, *grid, K.S())
    assert torch.equal(dst.get(), _sent((V, 27 * C))) and torch.equal(out.get(), _sent((V, C)))


@_thin_params
@pytest.mark.parametrize("C", [1, 4, 8])
def test_thin_col2im(C, grid):
    V = math.prod(grid)
    P = _rnd((V, 27 * C + 5), 121)                               # ld_p > 27 C: the pad columns are never read
    bias = _rnd((C,), 122)
    for sign in (1, -1):
        taps = sum(_tap_shift(P[:, tap * C:(tap + 1) * C].double(), grid, tap, sign) for tap in range(27))
        for b in (None, bias):
            ref = taps if b is None else taps + b.double()
            for ld_out in (C, C + 3):
                got = _col2im(P, C, grid, sign, ld_out, b)
                assert nrmse(ref.numpy(), got[:, :C].double().numpy()) < 1e-6, (sign, ld_out)
                assert not got[:, C:].any()                      # zeroed when not accumulating
                out0 = _rnd((V, ld_out), 123)
                got = _col2im(P, C, grid, sign, ld_out, b, out0)
                assert nrmse((ref + out0[:, :C].double()).numpy(), got[:, :C].double().numpy()) < 1e-6
                assert torch.equal(got[:, C:], out0[:, C:])      # untouched when accumulating


@_thin_params
def test_thin_conv_end_to_end(grid):
    """The sign convention of include/dlcs.h and dit_engine: im2col(sign = +1) times a
    [cout, 27 C] weight in [tap][ci] order is F.conv3d(padding=1) (cross-correlation), and
    col2im(sign = +1) of a thin GEMM output P[v][tap * cout + co] = sum_d r[v][d] w[co, d, tap]
    is the same convolution; sign = -1 gives their adjoints (the input gradients)."""
    B, D, H, W = grid
    V, c4, hid = math.prod(grid), 4, 16
    # thin input: cin = 4 -> hid, weight packed [co][tap][ci] (dit_engine.py: Wsfe)
    x = _rnd((B, c4, D, H, W), 130)
    w = _rnd((hid, c4, 3, 3, 3), 131) / (27 * c4) ** 0.5
    col = _im2col(_pad_cols(_to_blocked(x), 8), c4, grid, +1, 27 * c4)
    Wsfe = torch.as_strided(w, (hid, 27, c4), (c4 * 27, 1, 27)).reshape(hid, 27 * c4)
    ref = _to_blocked(F.conv3d(x.double(), w.double(), padding=1))
    assert nrmse(ref.numpy(), (col.double() @ Wsfe.double().t()).numpy()) < 1e-12
    # thin output: hid -> cout = 4, weight [tap * cout + co][d] (dit_engine.py: Wf2)
    r = _rnd((B, hid, D, H, W), 132)
    wf = _rnd((c4, hid, 3, 3, 3), 133) / (27 * hid) ** 0.5
    bias = _rnd((c4,), 134)
    Wf2 = torch.as_strided(wf, (27, c4, hid), (1, hid * 27, 27)).reshape(27 * c4, hid)
    P = (_to_blocked(r).double() @ Wf2.double().t()).float()
    got = _col2im(P, c4, grid, +1, 8, bias)
    ref = _to_blocked(F.conv3d(r.double(), wf.double(), bias.double(), padding=1))
    assert nrmse(ref.numpy(), got[:, :c4].double().numpy()) < 1e-6
    # adjointness of the pair the engine uses for a conv and its input gradient
    Pr = _rnd((V, 27 * c4), 135)
    xb = _pad_cols(_to_blocked(x), 8)
    lhs = float((_im2col(xb, c4, grid, +1, 27 * c4).double() * Pr.double()).sum())
    rhs = float((xb[:, :c4].double() * _col2im(Pr, c4, grid, -1, c4).double()).sum())
    assert _rel_close(lhs, rhs, 1e-6), (lhs, rhs)
    lhs = float((_im2col(xb, c4, grid, -1, 27 * c4).double() * Pr.double()).sum())
    rhs = float((xb[:, :c4].double() * _col2im(Pr, c4, grid, +1, c4).double()).sum())
    assert _rel_close(lhs, rhs, 1e-6), (lhs, rhs)


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("N,Kd", [(48, 40), (5, 1), (1, 300)])
def test_scale_rows(N, Kd, with_bias):
    K = _K()
    W, b, gate = _rnd((N, Kd), 140), _rnd((N,), 141), _rnd((N,), 142)
    Wd, bd, gd = W.to(DEV), b.to(DEV) if with_bias else None, gate.to(DEV)
    Wo, bo = _Out((N, Kd)), _Out((N,))
    _call("dlcs_scale_rows", K.p(Wd), K.p(bd), K.p(gd), K.p(Wo.t), K.p(bo.t), N, Kd, K.S())
    assert torch.equal(Wo.get(), gate[:, None] * W)
    assert torch.equal(bo.get(), gate * b if with_bias else _sent((N,)))


@pytest.mark.parametrize("nrows,C", [(7, 384), (1, 1)])
def test_rows_add(nrows, C):
    """dst[idx[r]] += src[r]: duplicates accumulate, negative indices are skipped."""
    K = _K()
    ndst = 5
    src, dst0 = _rnd((nrows, C), 150), _rnd((ndst, C), 151)
    idx = torch.tensor([3, 0, 3, -1, 4, 3, -1][:nrows], dtype=torch.int32)
    dst = _Out((ndst, C), init=dst0)
    sd, idd = src.to(DEV), idx.to(DEV)
    _call("dlcs_rows_add", K.p(dst.t), K.p(idd), K.p(sd), nrows, C, K.S())
    keep = idx >= 0
    ref = dst0.double().index_add_(0, idx[keep].long(), src[keep].double())
    assert nrmse(ref.numpy(), dst.get().double().numpy()) < 1e-6
    assert torch.equal(dst.get()[[1, 2]], dst0[[1, 2]])           # rows no index names
    dst0 = _rnd((nrows, C), 152)
    dst = _Out((nrows, C), init=dst0)
    _call("dlcs_rows_add", K.p(dst.t), None, K.p(sd), nrows, C, K.S())
    assert torch.equal(dst.get(), dst0 + src)                    # idx = NULL: one fp32 add per element


@pytest.mark.parametrize("n", [1, 1000])
def test_dit_vec(n):
    K = _K()
    a, b = _rnd((n,), 160), _rnd((n,), 161)
    ad, bd = a.to(DEV), b.to(DEV)

    def run(op, second):
        y = _Out((n,))
        _call("dlcs_dit_vec", op, K.p(ad), K.p(second), K.p(y.t), n, K.S())
        return y.get()
    assert torch.equal(run(2, None), 1.0 + a)                    # modulate's 1 + scale
    assert torch.equal(run(3, bd), a + b)
    assert nrmse(F.silu(a.double()).numpy(), run(0, None).double().numpy()) < 2e-6
    bb = b.double().requires_grad_()
    F.silu(bb).backward(a.double())
    assert nrmse(bb.grad.numpy(), run(1, bd).double().numpy()) < 2e-6


def test_timestep_embedding_odd_dim():
    from oracle import dit_oracle as DO
    K = _K()
    t = torch.tensor([0.0, 1.0, 37.0, 613.0, 999.0])
    td = t.to(DEV)
    dim = 255
    te = _Out((5, dim))
    _call("dlcs_timestep_embedding", K.p(td), 5, dim, 10000.0, K.p(te.t), K.S())
    got = te.get()
    assert not got[:, dim - 1].any()                             # the odd last column is exactly zero
    assert (got - DO.timestep_embedding(t, dim)).abs().max() < 2e-4      # sin/cos of t f up to 999


# ============================================================================ 7. degenerate GEMMs
@pytest.mark.parametrize("dtype,tol", [(F32, 1e-6), (BF16, 1e-2)], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,N,K_,a_t,b_t,bias,acc", [
    (300, 1, 160, 0, 0, True, 0),       # patchgan head: logits = a3 wh^T + bh
    (1, 160, 300, 1, 1, False, 1),      # head weight gradient: g^T a3 accumulated
    (300, 160, 1, 0, 1, False, 0),      # head input gradient: g wh
    (1, 1, 1, 0, 0, False, 0)])
def test_gemm_degenerate(M, N, K_, a_t, b_t, bias, acc, dtype, tol):
    """dlcs_gemm at the N = 1, M = 1 and K = 1 shapes of models/patchgan.py (leading
    dimensions as there: each operand dense), vs float64 on the rounded operands."""
    K = _K()
    A = _rnd((K_, M) if a_t else (M, K_), 170)
    B = _rnd((K_, N) if b_t else (N, K_), 171)
    bv = _rnd((N,), 172) if bias else None
    C0 = _rnd((M, N), 173) if acc else None
    Am, Bm = (A.t() if a_t else A), (B.t() if b_t else B)
    ref = Am.to(dtype).double() @ Bm.to(dtype).double().t()
    if bias:
        ref = ref + bv.double()
    if acc:
        ref = ref + C0.double()
    for cdt in ((F32,) if acc or dtype == F32 else (F32, dtype)):
        C = _Out((M, N), cdt, init=C0)
        K.gemm(A.to(DEV, dtype), B.to(DEV, dtype), C.t, M, N, K_, A.shape[1], B.shape[1], N, a_trans=a_t, b_trans=b_t,
               bias=None if bv is None else bv.to(DEV), accumulate=acc, splitk=max(1, min(64, K_ // 256)) if acc else 1)
        assert nrmse(ref.numpy(), C.get().double().numpy()) < max(tol, 1e-6), cdt
