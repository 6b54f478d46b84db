"""Direct tests of the box kernels (box.hip; dlcs.h "A box inside a padded grid"), in the
style of test_gpu_glue_kernels.py: every output lies between sentinel margins, the
references are torch constructions on the CPU.

  dlcs_box_pre / _pre_bwd        test_box_pre, test_box_pre_bwd (adjoint)
  dlcs_box_post / _post_bwd      test_box_post, test_box_post_bwd (adjoint)
  all four without slack         test_box_equals_swin_without_slack (bitwise dlcs_swin_*)
  dlcs_box_zero                  test_box_zero, test_box_zero_no_slack, test_box_zero_refusals
  refusals of the four           test_box_prepost_refusals

The four layout kernels copy values (the backward of pre sums at most three of them in a
fixed order), so all comparisons but the adjoint identities are bitwise.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
GUARD = 64
SENT = -12345.0
UNSUPPORTED = 100002

# (B, E, T, Y, X, pad); the last has no slack
CASES = [(2, 1, 5, 6, 7, 4), (1, 2, 7, 3, 9, 6), (1, 1, 8, 8, 8, 4)]
LDC = 8
_cases = pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))


def _K():
    from dl_cs.models import _ops as K
    return K


def _raw(name, *args):
    """The entry point's status, unchecked."""
    from dl_cs import _lib
    return getattr(_lib.lib(), name)(*args)


def _call(name, *args):
    from dl_cs import _lib
    _lib.call(name, *args)


def _pad4(n):
    return (n + 3) // 4 * 4


def _rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _crnd(shape, seed):
    return torch.complex(_rnd(shape, seed), _rnd(shape, seed + 1000))


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Out:
    """A sentinel-filled output buffer between two GUARD-element sentinel margins."""

    def __init__(self, shape, init=None):
        shape = tuple(int(s) for s in shape)
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=F32, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if init is not None:
            self.t.copy_(init.reshape(shape))

    def get(self):
        b = self.buf.cpu()
        s = torch.full((GUARD,), SENT)
        assert torch.equal(b[:GUARD], s), "write before the output buffer"
        assert torch.equal(b[b.numel() - GUARD:], s), "write past the output buffer"
        return b[GUARD:b.numel() - GUARD].view(self.t.shape).clone()


def _to_blocked(x):
    """[B, C, D, H, W] (D, H, W multiples of 4) -> blocked rows [B D H W, C]."""
    B, C, D, H, W = x.shape
    t = x.permute(0, 2, 3, 4, 1).reshape(B, D // 4, 4, H // 4, 4, W // 4, 4, C)
    return t.permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(-1, C)


def _from_blocked(r, B, D, H, W):
    C = r.shape[1]
    t = r.reshape(B, D // 4, H // 4, W // 4, 4, 4, 4, C).permute(0, 1, 4, 2, 5, 3, 6, 7)
    return t.reshape(B, D, H, W, C).permute(0, 4, 1, 2, 3)


def _geom(case):
    B, E, T, Y, X, pad = case
    D = T + 2 * pad
    return (B, E, T, Y, X), pad, (D, Y, X), (_pad4(D), _pad4(Y), _pad4(X))


def _extend(v, padded):
    """[B, C, D, H, W] zero-extended to the padded grid."""
    D, H, W = v.shape[2:]
    return F.pad(v, (0, padded[2] - W, 0, padded[1] - H, 0, padded[0] - D))


def _pre_ref(x, pad, padded):
    """cat re / im, circular time pad, zero-extend, block, pad the columns to LDC."""
    xr = torch.cat([x.real, x.imag], 1)
    u = F.pad(xr, (0, 0, 0, 0, pad, pad), mode="circular")
    r = _to_blocked(_extend(u, padded))
    return F.pad(r, (0, LDC - r.shape[1]))


def _post_bwd_ref(gout, pad, padded):
    """cat re / im, zero time pad, zero-extend, block, pad the columns to LDC."""
    gr = torch.cat([gout.real, gout.imag], 1)
    r = _to_blocked(_extend(F.pad(gr, (0, 0, 0, 0, pad, pad)), padded))
    return F.pad(r, (0, LDC - r.shape[1]))


def _post_ref(o, shape, pad, padded):
    B, E, T, Y, X = shape
    v = _from_blocked(o, B, *padded)[:, :2 * E, pad:pad + T, :Y, :X]
    return torch.complex(v[:, :E].contiguous(), v[:, E:].contiguous())


def _box_scatter(name, x, pad, padded):
    """dlcs_box_pre / dlcs_box_post_bwd into a sentinel-filled [rows, LDC]."""
    K = _K()
    B, E, T, Y, X = x.shape
    xd = x.to(DEV).contiguous()
    u = _Out((B * padded[0] * padded[1] * padded[2], LDC))
    _call(name, K.p(xd), K.p(u.t), B, E, T, Y, X, pad, *padded, LDC, K.S())
    return u.get()


def _box_gather(name, o, shape, pad, padded):
    """dlcs_box_pre_bwd / dlcs_box_post from rows [.., ld] into a sentinel-filled complex tensor."""
    K = _K()
    B, E, T, Y, X = shape
    od = o.to(DEV).contiguous()
    out = _Out(tuple(shape) + (2,))
    _call(name, K.p(od), K.p(out.t), B, E, T, Y, X, pad, *padded, o.shape[1], K.S())
    return torch.view_as_complex(out.get())


def _rows_operand(case, seed):
    """Random rows [rows of the padded grid, LDC]: slack rows and columns >= 2E hold values
    that a kernel reading them would carry into its output."""
    shape, pad, box, padded = _geom(case)
    return _rnd((shape[0] * padded[0] * padded[1] * padded[2], LDC), seed)


@_cases
def test_box_pre(case):
    shape, pad, box, padded = _geom(case)
    x = _crnd(shape, 11)
    u = _box_scatter("dlcs_box_pre", x, pad, padded)
    assert not bool((u == SENT).any()), "a row of the padded grid was not written"
    assert torch.equal(_bits(u), _bits(_pre_ref(x, pad, padded)))       # +0.0 on slack rows and columns >= 2E


@_cases
def test_box_post_bwd(case):
    shape, pad, box, padded = _geom(case)
    gout = _crnd(shape, 21)
    go = _box_scatter("dlcs_box_post_bwd", gout, pad, padded)
    assert not bool((go == SENT).any()), "a row of the padded grid was not written"
    assert torch.equal(_bits(go), _bits(_post_bwd_ref(gout, pad, padded)))
    # adjoint of post: <post o, g> = <o, post_bwd g> over all rows and columns
    o = _rows_operand(case, 22)
    out = _box_gather("dlcs_box_post", o, shape, pad, padded)
    lhs = float((out.to(torch.complex128) * gout.to(torch.complex128).conj()).real.sum())
    rhs = float((o.double() * go.double()).sum())
    # both sides are float64 sums of the same exact products, in different orders
    assert abs(lhs - rhs) <= 1e-12 * float((o.double() * go.double()).abs().sum())


@_cases
def test_box_post(case):
    shape, pad, box, padded = _geom(case)
    o = _rows_operand(case, 31)
    out = _box_gather("dlcs_box_post", o, shape, pad, padded)
    ref = _post_ref(o, shape, pad, padded)
    assert torch.equal(_bits(torch.view_as_real(out)), _bits(torch.view_as_real(ref)))


@_cases
def test_box_pre_bwd(case):
    """The adjoint of pre, <pre x, u> = <x, pre_bwd u>, with u random on every row: slack rows
    and columns >= 2E pair with pre's zeros, so a pre_bwd that read them would break it."""
    shape, pad, box, padded = _geom(case)
    x = _crnd(shape, 41)
    u = _rows_operand(case, 42)
    pre = _box_scatter("dlcs_box_pre", x, pad, padded)
    gx = _box_gather("dlcs_box_pre_bwd", u, shape, pad, padded)
    lhs = float((pre.double() * u.double()).sum())
    rhs = float((x.to(torch.complex128) * gx.to(torch.complex128).conj()).real.sum())
    # pre_bwd sums up to 3 fp32 terms per element: relative 2 x 2^-24 of the terms' magnitude
    scale = float((pre.double().abs() * u.double().abs()).sum())
    assert abs(lhs - rhs) <= 2 * 2.0 ** -24 * scale
    # and the values themselves: the float64 sum of the frames t + pad + k T, cropped to the box
    B, E, T, Y, X = shape
    v = _from_blocked(u, B, *padded)[:, :2 * E, :box[0], :Y, :X].double()
    acc = torch.zeros((B, 2 * E, T, Y, X), dtype=torch.float64)
    for tp in range(box[0]):
        acc[:, :, (tp - pad) % T] += v[:, :, tp]
    ref = torch.complex(acc[:, :E], acc[:, E:])
    assert float((gx.to(torch.complex128) - ref).abs().max()) <= 2 * 2.0 ** -24 * float(v.abs().max()) * 3


def test_box_equals_swin_without_slack():
    """(1, 1, 8, 8, 8, pad 4): the padded grid is the box; the same bits as dlcs_swin_*."""
    K = _K()
    case = CASES[-1]
    shape, pad, box, padded = _geom(case)
    assert box == padded
    x = _crnd(shape, 51)
    o = _rows_operand(case, 52)
    xd, od = x.to(DEV), o.to(DEV)
    pairs = [(_box_scatter("dlcs_box_pre", x, pad, padded), K.swin_pre(xd, F32, pad, LDC)),
             (_box_scatter("dlcs_box_post_bwd", x, pad, padded), K.swin_post_bwd(xd, F32, pad, LDC)),
             (torch.view_as_real(_box_gather("dlcs_box_post", o, shape, pad, padded)),
              torch.view_as_real(K.swin_post(od, shape, pad))),
             (torch.view_as_real(_box_gather("dlcs_box_pre_bwd", o, shape, pad, padded)),
              torch.view_as_real(K.swin_pre_bwd(od, shape, pad)))]
    for got, swin in pairs:
        assert torch.equal(_bits(got), _bits(swin.cpu()))


def test_box_prepost_refusals():
    K = _K()
    shape, pad, box, padded = _geom(CASES[0])
    B, E, T, Y, X = shape
    x = _crnd(shape, 61).to(DEV)
    rows = B * padded[0] * padded[1] * padded[2]
    bad = [(padded[0] + 1, padded[1], padded[2]),          # not a multiple of 4
           (padded[0], padded[1] - 4, padded[2]),          # H > Hp
           (padded[0] - 4, padded[1], padded[2])]          # D > Dp
    for name, gather in (("dlcs_box_pre", False), ("dlcs_box_post_bwd", False), ("dlcs_box_post", True),
                         ("dlcs_box_pre_bwd", True)):
        for g in bad:
            u = _Out((rows + 64 * B * padded[1] * padded[2], LDC))
            out = _Out(tuple(shape) + (2,))
            a, b = (u.t, out.t) if gather else (x, u.t)
            assert _raw(name, K.p(a), K.p(b), B, E, T, Y, X, pad, *g, LDC, K.S()) == UNSUPPORTED, (name, g)
            assert bool((u.get() == SENT).all()) and bool((out.get() == SENT).all()), (name, g)


# ---------------------------------------------------------------------------- box_zero
# (box D, H, W), (padded Dp, Hp, Wp)
ZERO_GRIDS = [((5, 6, 7), (8, 8, 8)), ((4, 4, 3), (4, 4, 4)), ((1, 1, 1), (4, 4, 4))]


def _slack_rows(B, box, padded):
    """Boolean [rows]: the blocked rows outside the box."""
    inside = torch.zeros((B, 1) + tuple(padded))
    inside[:, :, :box[0], :box[1], :box[2]] = 1
    return _to_blocked(inside)[:, 0] == 0


def _box_zero(buf, ld, C, B, padded, box):
    K = _K()
    return _raw("dlcs_box_zero", K.p(buf), ld, C, B, *padded, *box, K.S())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("grids", ZERO_GRIDS, ids=lambda g: "x".join(map(str, g[0])) + "in" + "x".join(map(str, g[1])))
@pytest.mark.parametrize("dld", [0, 3, 4])
@pytest.mark.parametrize("C", [1, 6, 8, 64])
def test_box_zero(C, dld, grids, B):
    box, padded = grids
    ld = C + dld
    rows = B * padded[0] * padded[1] * padded[2]
    before = _rnd((rows, ld), 71)                          # valid rows and columns >= C keep these bits
    before[::7] = SENT
    x = _Out((rows, ld), init=before)
    assert _box_zero(x.t, ld, C, B, padded, box) == 0
    after = x.get()
    slack = _slack_rows(B, box, padded)
    assert int(slack.sum()) == B * (math.prod(padded) - math.prod(box))
    expect = before.clone()
    expect[slack, :C] = 0.0                                # +0.0: bit pattern 0
    assert torch.equal(_bits(after), _bits(expect))


def test_box_zero_unaligned_base():
    """C and ld multiples of 4 but the base pointer 4 B off a 16-B boundary: the scalar path."""
    box, padded = ZERO_GRIDS[0]
    C = ld = 8
    rows = math.prod(padded)
    before = _rnd((rows * ld + 1,), 72)
    buf = _Out((rows * ld + 1,), init=before)
    view = buf.t[1:]
    assert view.data_ptr() % 16 == 4
    assert _box_zero(view, ld, C, 1, padded, box) == 0
    expect = before.clone()
    e = expect[1:].view(rows, ld)
    e[_slack_rows(1, box, padded)] = 0.0
    assert torch.equal(_bits(buf.get()), _bits(expect))


def test_box_zero_no_slack():
    padded = (4, 8, 4)
    rows = 2 * math.prod(padded)
    x = _Out((rows, 8))
    assert _box_zero(x.t, 8, 8, 2, padded, padded) == 0
    assert bool((x.get() == SENT).all()), "written without slack"


def test_box_zero_refusals():
    x = _Out((3 * 8 * 8 * 8 + 64 * 64, 8))
    cases = [(1, (8, 8, 6), (5, 6, 5)),                    # Wp not a multiple of 4
             (1, (7, 8, 8), (5, 6, 7)),                    # Dp not a multiple of 4
             (1, (4, 8, 8), (5, 6, 7)),                    # D > Dp
             (1, (8, 4, 8), (5, 6, 7)),                    # H > Hp
             (1, (8, 8, 4), (5, 6, 7)),                    # W > Wp
             (65536, (8, 8, 8), (5, 6, 7))]                # B > 65535
    for B, padded, box in cases:
        assert _box_zero(x.t, 8, 8, B, padded, box) == UNSUPPORTED, (B, padded, box)
        assert bool((x.get() == SENT).all()), (B, padded, box)
