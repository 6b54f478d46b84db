"""The DSLR family in compute dtype bf16 (resnet2d._PlaneFn on the plane conv, csrc/conv2d.hip)
against tests/golden/dslr.npz and the float64 oracle tests/dslr_oracle.py, with the helpers
of test_gpu_dslr.py.

Bars.  Predictions: NRMSE against the reference's fixture < 1e-2, the bf16 budget of every
bf16 test here.  Gradients: the rule of test_gpu_trunk_bf16.py -- the CPU oracle under
torch.autocast("cpu", bfloat16) on the same weights, input and cotangent defines the error
a bf16-operand evaluation carries against float64, and the HIP path stays within 1.5 x of
it per class (correction net(x) - x, dx, median and max over the parameter tensors).  The
autocast oracle is dslr_oracle with its _trunk wrapped (monkeypatch): autocast around the
call, .float() on the result; everything outside the two CNNs stays at the oracle's dtype.
"""
import json
import math

import pytest
import torch

import dslr_oracle as D
import test_gpu_dslr as T
from oracle import recipe

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
_CACHE = {}


@pytest.fixture(autouse=True)
def _fp32_after():
    yield
    from dl_cs.models import swin3D
    swin3D.set_compute_dtype(torch.float32)


def _bf16():
    from dl_cs.models import swin3D
    swin3D.set_compute_dtype(BF16)


def _autocast_trunk(monkeypatch):
    """dslr_oracle._trunk under CPU autocast to bf16, its result back in fp32."""
    plain = D._trunk

    def trunk(*a, **kw):
        with torch.autocast("cpu", dtype=BF16):
            o = plain(*a, **kw)
        return o.float()
    monkeypatch.setattr(D, "_trunk", trunk)


def _rel(a, b):
    a, b = torch.as_tensor(a).to(torch.complex128), torch.as_tensor(b).to(torch.complex128)
    return float((a - b).abs().pow(2).sum().sqrt() / b.abs().pow(2).sum().sqrt())


def _med_max(grads, ref):
    pr = sorted(_rel(grads[k], ref[k]) for k in ref if ref[k].abs().sum() > 0)
    return pr[len(pr) // 2], pr[-1]


# ---------------------------------------------------------------------------- 1: the two CNNs alone
def _net(kind, size, nb):
    """test_gpu_dslr._net_case's networks at a block size / sequence length and nb resblocks."""
    from dl_cs.models import resnet1d, resnet2d
    if kind == "2d":
        net = resnet2d.ResNet(num_resblocks=nb, in_chans=12, chans=8, kernel_size=3)
        x = recipe.crandn(31, (77, 6, size, size))
        f = lambda P, v: D.resnet2d(P, "", v, nb)
    else:
        net = resnet1d.ResNet(num_resblocks=nb, in_chans=6, chans=8, kernel_size=3, circular_pad=True)
        x = recipe.crandn(32, (77, 3, size))
        f = lambda P, v: D.resnet1d(P, "", v, nb)
    recipe.fill_module(net, 33)
    return net, x, f


# test_resnet_alone's shapes (77 planes of 4 x 4; 77 sequences, T + 2 pad = 12 + 12), and one of each that
# the fp32 path refuses: b = 6, and T + 2 pad = 6 + 8 = 14 (one resblock; a circular pad cannot exceed T)
ALONE = [("2d", 4, 2), ("2d", 6, 2), ("1d", 12, 2), ("1d", 6, 1)]


@pytest.mark.parametrize("kind,size,nb", ALONE)
def test_resnet_alone_bf16(monkeypatch, kind, size, nb):
    net, x, f = _net(kind, size, nb)
    w = recipe.crandn(34, tuple(x.shape))
    net = net.cuda()
    if size == 6:
        with pytest.raises(NotImplementedError):                  # compute dtype fp32: the multiple-of-4 grid
            net(x.cuda())
    _bf16()
    xg = x.cuda().requires_grad_()
    out = net(xg)
    torch.sum((out * w.cuda().conj()).real).backward()
    hip = (out.detach().cpu(), xg.grad.cpu(), {n: p.grad.detach().cpu() for n, p in net.named_parameters()})
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}

    def oracle(dt, cd):
        P = {k: v.to(dt).clone().requires_grad_() for k, v in sd.items()}
        xi = x.to(cd).clone().requires_grad_()
        o = f(P, xi)
        torch.sum((o * w.to(cd).conj()).real).backward()
        return o.detach(), xi.grad, {k: p.grad for k, p in P.items()}

    ref = oracle(torch.float64, torch.complex128)
    _autocast_trunk(monkeypatch)
    amp = oracle(torch.float32, torch.complex64)

    def classes(y, dx, gp):
        return (_rel(y - x, ref[0] - x), _rel(dx, ref[1])) + _med_max(gp, ref[2]) + (_rel(y, ref[0]),)

    h, a = classes(*hip), classes(*amp)
    for name, hv, av in zip(("correction", "dx", "median param", "max param", "rel(y)"), h, a):
        print(f"resnet{kind} {size} {name}: HIP bf16 {hv:.3g}  autocast oracle {av:.3g}")
    assert tuple(out.shape) == tuple(x.shape) and h[4] < 1e-2
    for hv, av in zip(h[:4], a[:4]):
        assert hv <= 1.5 * av, (h, a)


# ---------------------------------------------------------------------------- 2: the five networks
def _bf16_step(g, arch, **over):
    model = T._model(arch, **over)
    if over.get("GRAD_CHECKPOINT"):
        model.train()
    _bf16()
    return T._run(model, g, arch)


def _first(g, arch):
    """The bf16 step of a network at the fixture's case A: computed once, shared, left unchanged."""
    if arch not in _CACHE:
        _CACHE[arch] = _bf16_step(g, arch)
    return _CACHE[arch]


@pytest.mark.parametrize("arch", D.ARCHS)
def test_network_fwd_bwd_bf16(golden, monkeypatch, arch):
    g = golden("dslr")
    pred, loss, grads = _first(g, arch)
    e = D.nrmse(g[f"{arch}_pred"], pred[0].numpy())
    print(f"{arch} bf16: output NRMSE vs the reference {e:.3g}, loss {loss:.6g}")
    assert e < 1e-2
    assert sorted(grads) == [str(k) for k in g[f"{arch}_grad_names"]]
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())
    _, (_, _, o64) = T._oracle(g, arch)
    _autocast_trunk(monkeypatch)
    pa, _, oa = D.oracle_run(g, arch, torch.float32)
    (hm, hx), (am, ax) = _med_max(grads, o64), _med_max(oa, o64)
    print(f"{arch} bf16 gradients vs float64: HIP median {hm:.3g} max {hx:.3g}; autocast oracle median {am:.3g} "
          f"max {ax:.3g} (its prediction vs the fixture {D.nrmse(g[f'{arch}_pred'], pa.numpy()):.3g})")
    assert hm <= 1.5 * am and hx <= 1.5 * ax


# ---------------------------------------------------------------------------- 3: storage
@pytest.mark.parametrize("kind,size,nb", [ALONE[1], ALONE[3]])
def test_saved_activations_are_bf16(monkeypatch, kind, size, nb):
    from dl_cs.models import resnet2d
    saved = []
    plain = resnet2d.plane_forward

    def capture(*a, **kw):
        out, sv = plain(*a, **kw)
        saved.append(sv)
        return out, sv
    monkeypatch.setattr(resnet2d, "plane_forward", capture)
    net, x, _ = _net(kind, size, nb)
    _bf16()
    net.cuda()(x.cuda().requires_grad_())
    (sv,) = saved
    Tp = size + 2 * (2 * nb + 2)
    rows = 77 * (size * size if kind == "2d" else Tp)
    assert sv["planes"] == ((77, size, size, 3) if kind == "2d" else (77, 1, Tp, 1))       # no padding of N, b or T'
    acts = [sv["u"]] + sv["r"] + sv["ts"]
    assert len(sv["r"]) == nb + 1 and len(sv["ts"]) == nb
    for t, C in zip(acts, [sv["C"]] + [sv["F"]] * (2 * nb + 1)):
        assert t.dtype == BF16 and t.shape[0] == rows and t.shape[1] == (C + 7) // 8 * 8 and t.stride() == (t.shape[1], 1)


# ---------------------------------------------------------------------------- 4: repeatability
def test_bf16_step_is_repeatable(golden):
    g = golden("dslr")
    p0, _, g0 = _first(g, "modl-v1")
    p1, _, g1 = _bf16_step(g, "modl-v1")
    assert torch.equal(torch.view_as_real(p0), torch.view_as_real(p1))
    assert sorted(g0) == sorted(g1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


# ---------------------------------------------------------------------------- 5, 6
@pytest.mark.parametrize("arch", ["cg-v1", "modl-v2"])
def test_grad_checkpoint_same_gradients_bf16(golden, arch):
    """The checkpointed recompute runs the same launches on the same inputs, and the gradients
    have to agree to 1e-6, the bar of test_gpu_dslr.py's fp32 test at the same two networks.

    modl-v2 needs dslr._DenseGrad for it: an output of a checkpointed segment that nothing reads
    (L and R of its four-tensor state) gets a contiguous zero gradient first, the single backward
    pass hands on the strided view that the CNN input's permute leaves, and torch's reductions in
    the CG backward then add in another order.  Without it the two modes differed by 3.5e-7 in
    the gradient reaching the last unroll's 2-D CNN, and -- a few fp32 ulps moving bf16-stored
    gradient elements by 2^-8 -- by up to 3.3e-4 per parameter tensor.  With it every CNN node
    receives and returns the same bits in both modes."""
    g = golden("dslr")
    p1, _, g1 = _bf16_step(g, arch, GRAD_CHECKPOINT=True)
    model = T._model(arch, GRAD_CHECKPOINT=False)
    model.train()
    _bf16()
    p0, _, g0 = T._run(model, g, arch)
    assert D.nrmse(p0.numpy(), p1.numpy()) <= 1e-6
    assert sorted(g0) == sorted(g1)
    for k in g0:
        assert D.nrmse(g0[k].numpy(), g1[k].numpy()) <= 1e-6, k


def test_share_weights_bf16(golden):
    g = golden("dslr")
    pred, _, grads = _bf16_step(g, "cg-v2", SHARE_WEIGHTS=True)
    _, (p64, _, o64) = T._oracle(g, "cg-v2", share=True)
    assert D.nrmse(p64.numpy(), pred[0].numpy()) < 1e-2
    assert sorted(grads) == sorted(o64) and all(bool(torch.isfinite(v).all()) for v in grads.values())


# ---------------------------------------------------------------------------- 7: the fp32 path
@pytest.mark.parametrize("arch", D.ARCHS)
def test_fp32_path_unchanged(golden, monkeypatch, arch):
    """Compute dtype fp32 calls none of the plane-conv wrappers, and test_network_fwd_bwd's
    assertions hold as before."""
    from dl_cs.models import _ops as K

    def refuse(*a, **kw):
        raise AssertionError("plane conv called in compute dtype fp32")
    for name in ("conv2d", "conv2d_pack", "conv2d_wgrad", "conv2d_unpack_grad"):
        monkeypatch.setattr(K, name, refuse)
    T.test_network_fwd_bwd(golden, arch)


# ---------------------------------------------------------------------------- 8: train_lr.py --dtype bf16
def test_train_lr_script_bf16(tmp_path):
    out = tmp_path / "out"
    cfg = tmp_path / "dslr.yaml"
    cfg.write_text(T.LR_CFG.format(out=str(out), arch="modslr-v1"))
    tr = T._script("train_lr")
    tr.main(["--config-file", str(cfg), "--data", "synthetic", "--synthetic-slices", "2",
             "--synthetic-shape", "4", "2", "8", "16", "24", "--dtype", "bf16"])
    from dl_cs.models import swin3D
    assert swin3D.get_compute_dtype() == BF16
    recs = [json.loads(line) for line in (out / "exp" / "metrics.jsonl").read_text().splitlines()]
    train = [r for r in recs if "Train/complex_l1" in r]
    val = [r for r in recs if "Validate/complex_l1" in r]
    assert len(train) == 2 and len(val) == 1
    assert all(math.isfinite(r["Train/complex_l1"]) for r in train) and math.isfinite(val[0]["Validate/complex_l1"])
