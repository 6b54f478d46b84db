"""The five dlcs_lr_* kernels (lowrank.hip) and the four autograd Functions over them
against the float64 oracle (tests/dslr_oracle.py).

Bound: every output element is a sum of at most E b^2 = 512 fp32 products (project_r;
T <= 20 for project_l, 4 r <= 32 for compose), so its rounding error is about
sqrt(512) 2^-24 = 1.4e-6 of the operand scale, plus the fp32 window (one rounding).  The
project's fp32 bar NRMSE <= 1e-5 covers that with margin and is what every case uses.
"""
import pytest
import torch

import dslr_oracle as D
from goldutil import nrmse
from oracle import recipe

pytestmark = pytest.mark.gpu

TOL = 1e-5
# name: b, E, T, Y, X, r  (A, B, C: the issue's cases; odd T / r take the 8-B paths, even the 16-B ones)
CASES = {
    "A": (4, 2, 8, 12, 20, 3),
    "B": (4, 2, 5, 9, 13, 3),
    "C": (4, 1, 3, 11, 14, 2),
    "b8": (8, 2, 6, 16, 24, 4),
    "b16": (16, 2, 20, 32, 48, 8),
}
_CACHE = {}


def case(name):
    """Inputs, the module on the GPU and the float64 oracle results, computed once."""
    if name in _CACHE:
        return _CACHE[name]
    from dl_cs.mri import lowrank
    b, E, T, Y, X, r = CASES[name]
    g = D.Geo(b, E, T, Y, X)
    op = lowrank.ArrayToBlocks(b, [1, E, T, Y, X], True).cuda()
    seed = 900 + 10 * list(CASES).index(name)
    x = recipe.crandn(seed, (E, T, Y, X))
    B = recipe.crandn(seed + 1, (g.N, E * b * b, T))
    L = recipe.crandn(seed + 2, (g.N, E * b * b, r))
    R = recipe.crandn(seed + 3, (g.N, T, r))
    x64, B64, L64, R64 = (t.to(torch.complex128) for t in (x, B, L, R))
    ref = {}
    for d in (False, True):
        ref["extract", d] = D.extract(g, x64, d)
        ref["combine", d] = D.combine(g, B64, d)
        ref["compose", d] = D.compose(g, L64, R64, d)
        ref["project_l", d] = D.project_l(g, x64, R64, d)
        ref["project_r", d] = D.project_r(g, x64, L64, d)
    c = dict(g=g, op=op, r=r, x=x.cuda(), B=B.cuda(), L=L.cuda(), R=R.cuda(), x64=x64, B64=B64, L64=L64, R64=R64, ref=ref)
    _CACHE[name] = c
    return c


def run(c, what, d):
    from dl_cs.mri import lowrank as lr
    op = c["op"]
    return {"extract": lambda: lr._extract_raw(op, c["x"], d),
            "combine": lambda: lr._combine_raw(op, c["B"], d),
            "compose": lambda: lr._compose_raw(op, c["L"], c["R"], d),
            "project_l": lambda: lr._project_l_raw(op, c["x"], c["R"], d),
            "project_r": lambda: lr._project_r_raw(op, c["x"], c["L"], d)}[what]()


OPS = ("extract", "combine", "compose", "project_l", "project_r")


@pytest.mark.parametrize("name", list(CASES))
def test_geometry_and_weights(name):
    c = case(name)
    g, op = c["g"], c["op"]
    assert (op.num_blocks_y, op.num_blocks_x, op.pad_y, op.pad_x) == (g.nby, g.nbx, g.py, g.px)
    assert op.weights2d.is_cuda and op.win1d.is_cuda
    assert nrmse(g.weights.numpy(), op.weights2d.cpu().numpy()) < 1e-6


@pytest.mark.parametrize("divide", [False, True])
@pytest.mark.parametrize("what", OPS)
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_vs_oracle(name, what, divide):
    c = case(name)
    out = run(c, what, divide)
    ref = c["ref"][what, divide]
    assert tuple(out.shape) == tuple(ref.shape)
    assert torch.isfinite(torch.view_as_real(out)).all()
    err = nrmse(ref.numpy(), out.cpu().numpy())
    print(f"{name} {what} divide={int(divide)}: NRMSE {err:.3g}")
    assert err <= TOL


@pytest.mark.parametrize("name", list(CASES))
def test_adjoint_identities(name):
    """<extract x, B> = <x, combine_0 B> and <combine_1 B, x> = <B, extract_1 x>."""
    c = case(name)
    for d in (False, True):
        ex = run(c, "extract", d).to(torch.complex128)
        co = run(c, "combine", d).to(torch.complex128)
        lhs = torch.sum(ex.conj() * c["B"].to(torch.complex128))
        rhs = torch.sum(c["x"].to(torch.complex128).conj() * co)
        rel = float((lhs - rhs).abs() / lhs.abs())
        print(f"{name} divide={int(d)}: adjoint mismatch {rel:.3g}")
        assert rel <= 1e-5


@pytest.mark.parametrize("name", list(CASES))
def test_fused_equals_unfused(name):
    """compose = combine(L R^H); the projections = the products with extract(image)."""
    c = case(name)
    bt = lambda m: m.conj().transpose(1, 2)
    for d in (False, True):
        blocks = torch.bmm(c["L"], bt(c["R"])).contiguous()
        from dl_cs.mri import lowrank as lr
        assert nrmse(lr._combine_raw(c["op"], blocks, d).cpu().numpy(), run(c, "compose", d).cpu().numpy()) <= TOL
        ex = run(c, "extract", d)
        assert nrmse(torch.bmm(ex, c["R"]).cpu().numpy(), run(c, "project_l", d).cpu().numpy()) <= TOL
        assert nrmse(torch.bmm(bt(ex), c["L"]).cpu().numpy(), run(c, "project_r", d).cpu().numpy()) <= TOL


def test_zero_weight_row_is_zero():
    """Case C: the zero left pad gives the first row weight 0; combine and compose with
    divide return exactly 0 there (0 / 1e-8), and everything stays finite."""
    c = case("C")
    assert float(c["op"].weights2d[0].abs().max()) == 0.0
    for what in ("combine", "compose"):
        out = run(c, what, True)
        assert torch.isfinite(torch.view_as_real(out)).all()
        assert float(out[:, :, 0, :].abs().max()) == 0.0
    for what in ("extract", "project_l", "project_r"):
        assert torch.isfinite(torch.view_as_real(run(c, what, True))).all()


@pytest.mark.parametrize("name", ["B", "b16"])
def test_bitwise_reproducible(name):
    c = case(name)
    for what in OPS:
        a, b = run(c, what, True), run(c, what, True)
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b)), what


def _grads(fn, args, w):
    args = [a.clone().requires_grad_() for a in args]
    out = fn(*args)
    torch.sum((out * w.conj()).real).backward()
    return [a.grad for a in args]


@pytest.mark.parametrize("name", ["A", "B", "C", "b8"])
def test_autograd_vs_oracle(name):
    """torch.autograd through the four Functions (extract, combine, compose, project) against
    autograd through the float64 oracle, loss = Re <out, W>."""
    from dl_cs.mri import lowrank as lr
    c = case(name)
    g, op = c["g"], c["op"]
    x5, x5_64 = c["x"][None], c["x64"][None]
    todo = [
        ("extract", lambda x: op.extract(x), lambda x: D.extract(g, x[0]), [x5], [x5_64]),
        ("combine", lambda B: op.combine(B), lambda B: D.combine(g, B)[None], [c["B"]], [c["B64"]]),
        ("extract_adjoint", lambda B: op.extract_adjoint(B), lambda B: D.combine(g, B, False)[None], [c["B"]], [c["B64"]]),
        ("combine_adjoint", lambda x: op.combine_adjoint(x), lambda x: D.extract(g, x[0], True), [x5], [x5_64]),
        ("compose", lambda L, R: lr.compose(L, R, op), lambda L, R: D.compose(g, L, R)[None],
         [c["L"], c["R"]], [c["L64"], c["R64"]]),
        ("project_l", lambda x, R: lr.project_l(x, R, op), lambda x, R: D.project_l(g, x[0], R),
         [x5, c["R"]], [x5_64, c["R64"]]),
        ("project_r", lambda x, L: lr.project_r(x, L, op), lambda x, L: D.project_r(g, x[0], L),
         [x5, c["L"]], [x5_64, c["L64"]]),
        ("project_l_div", lambda x, R: lr.project_l(x, R, op, divide=True), lambda x, R: D.project_l(g, x[0], R, True),
         [x5, c["R"]], [x5_64, c["R64"]]),
    ]
    for label, f_hip, f_ref, a_hip, a_ref in todo:
        shape = f_ref(*a_ref).shape
        w = recipe.crandn(77, tuple(shape))
        got = _grads(f_hip, a_hip, w.cuda())
        want = _grads(f_ref, a_ref, w.to(torch.complex128))
        for k, (gh, gr) in enumerate(zip(got, want)):
            err = nrmse(gr.numpy(), gh.cpu().numpy())
            print(f"{name} {label} grad {k}: NRMSE {err:.3g}")
            assert err <= TOL, (label, k, err)


def test_double_backward_of_compose():
    """compose's backward is itself differentiable (the projections are Functions), which
    torch.utils.checkpoint and CG-through-autograd rely on."""
    from dl_cs.mri import lowrank as lr
    c = case("B")
    L, R = c["L"].clone().requires_grad_(), c["R"].clone().requires_grad_()
    out = lr.compose(L, R, c["op"])
    gL, = torch.autograd.grad(torch.sum(out.abs() ** 2), L, create_graph=True)
    torch.sum(gL.abs() ** 2).backward()
    assert torch.isfinite(torch.view_as_real(R.grad)).all() and float(R.grad.abs().max()) > 0


def test_unsupported_shapes_raise():
    from dl_cs.mri import lowrank as lr
    x = torch.zeros((1, 1, 4, 12, 12), dtype=torch.complex64, device="cuda")
    op6 = lr.ArrayToBlocks(6, [1, 1, 4, 12, 12], True).cuda()
    with pytest.raises(NotImplementedError):
        op6.extract(x)
    op4 = lr.ArrayToBlocks(4, [1, 1, 4, 12, 12], True).cuda()
    N = op4.num_blocks
    with pytest.raises(NotImplementedError):                       # rank 9
        lr.compose(torch.zeros((N, 16, 9), dtype=torch.complex64, device="cuda"),
                   torch.zeros((N, 4, 9), dtype=torch.complex64, device="cuda"), op4)
    opT = lr.ArrayToBlocks(4, [1, 1, 33, 12, 12], True).cuda()
    with pytest.raises(NotImplementedError):                       # T = 33
        opT.extract(torch.zeros((1, 1, 33, 12, 12), dtype=torch.complex64, device="cuda"))
    opE = lr.ArrayToBlocks(4, [1, 3, 4, 12, 12], True).cuda()
    with pytest.raises(NotImplementedError):                       # E = 3
        opE.extract(torch.zeros((1, 3, 4, 12, 12), dtype=torch.complex64, device="cuda"))


def test_host_operator_with_gpu_tensors_raises():
    """An operator whose window and weights are still on the host must not reach a kernel
    with GPU data (the kernels read them through raw pointers): every path raises."""
    from dl_cs import _lib
    from dl_cs.mri import lowrank as lr
    c = case("B")
    b, E, T, Y, X, r = CASES["B"]
    host = lr.ArrayToBlocks(b, [1, E, T, Y, X], True)
    for fn in (lambda: host.extract(c["x"][None]), lambda: host.combine(c["B"]),
               lambda: host.extract_adjoint(c["B"]), lambda: host.combine_adjoint(c["x"][None]),
               lambda: lr.compose(c["L"], c["R"], host), lambda: lr.project_l(c["x"][None], c["R"], host),
               lambda: lr.project_r(c["x"][None], c["L"], host)):
        with pytest.raises(_lib.DlcsError):
            fn()
    dec = lr.Decompose(b, r, [1, E, T, Y, X], True)                 # its operator stays on the host
    L, R = dec(c["x"][None])
    assert L.is_cuda and R.is_cuda
    with pytest.raises(_lib.DlcsError):
        dec((L, R), adjoint=True)
    assert tuple(dec((L.cpu(), R.cpu()), adjoint=True).shape) == (1, E, T, Y, X)


def test_other_dtypes_raise():
    from dl_cs import _lib
    c = case("B")
    with pytest.raises(_lib.DlcsError):
        c["op"].extract(c["x"][None].to(torch.complex128))
