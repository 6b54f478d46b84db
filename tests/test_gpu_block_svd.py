"""dlcs_lr_decompose (csrc/lowrank.hip): the truncated SVD of every block on the GPU, and the
switch that reaches it -- lowrank.Decompose(svd='device'), CinePreprocess(lr_svd='device'),
scripts/train_lr.py and scripts/reconstruct_lr.py with --svd device.

The reference in every test is torch.linalg.svd of dslr_oracle.extract in complex128
(tests/block_svd_cases.py).  Bars: the truncation L R^H to NRMSE 1e-5 (the project's fp32
bar), the singular values to 1e-5 sigma_1, ||L_k||^2 = ||R_k||^2 = S_k to 2e-5 max S, the
phase-aligned vectors [L_k; R_k] of the well-separated components to 1e-5.
"""
import pytest
import torch

import block_svd_cases as BC
import dslr_oracle as D
import test_gpu_dslr as T
from oracle import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _op(b, E, Tt, Y, X):
    from dl_cs.mri import lowrank
    return lowrank.ArrayToBlocks(b, [1, E, Tt, Y, X], True).to(DEV)


def _decompose(b, r, img):
    """(L, R, S, info) on the CPU of img [E, T, Y, X] (a CPU tensor)."""
    from dl_cs.mri import lowrank
    op = _op(b, *img.shape)
    out = lowrank.decompose_blocks(img.to(DEV), op, r, return_s=True, return_info=True)
    M = img.shape[0] * b * b
    assert [tuple(t.shape) for t in out] == [(op.num_blocks, M, r), (op.num_blocks, img.shape[1], r),
                                              (op.num_blocks, r), (op.num_blocks,)]
    assert [t.dtype for t in out] == [torch.complex64, torch.complex64, torch.float32, torch.int32]
    return tuple(t.cpu() for t in out)


@pytest.fixture(scope="module")
def results():
    """The kernel's output per (shape, image), computed once."""
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            b, E, Tt, Y, X, r = BC.CASES[name]
            cache[name, kind] = _decompose(b, r, BC.image(name, kind))
        return cache[name, kind]
    return get


@pytest.mark.parametrize("kind", BC.KINDS)
@pytest.mark.parametrize("name", list(BC.CASES))
def test_truncation(results, name, kind):
    r = BC.CASES[name][5]
    BC.check_truncation(BC.reference(name, kind), r, *results(name, kind), label=f"{name}/{kind}")


@pytest.mark.parametrize("name", list(BC.CASES))
def test_vectors(results, name):
    r = BC.CASES[name][5]
    L, R, S, info = results(name, "lowrank")
    err, mask = BC.vector_errors(BC.reference(name, "lowrank"), r, L, R)
    share = 1.0 - float(mask.double().mean())
    worst = float(err[mask].max())
    print(f"{name}: aligned-vector error {worst:.3g} over {int(mask.sum())} components, {100 * share:.1f} % left out")
    assert share <= BC.MAX_LEFT_OUT
    assert worst <= 1e-5


@pytest.mark.parametrize("name", list(BC.CASES))
def test_phase_convention(results, name):
    """The entry of R_k of largest magnitude is real and positive."""
    for kind in BC.KINDS:
        L, R, S, info = results(name, kind)
        mag = R.abs()                                             # [N, T, r]
        top = mag.max(dim=1, keepdim=True).values
        written = (top > 0).squeeze(1)                            # [N, r]
        assert bool(written.any())
        ok = (mag >= (1 - 1e-5) * top) & (R.imag.abs() <= 1e-5 * mag) & (R.real > 0)
        assert bool(ok.any(dim=1)[written].all())
        # a component is zero in L exactly when it is zero in R
        assert torch.equal((L.abs().amax(dim=1) > 0), written)


def test_zero_image():
    b, E, Tt, Y, X, r = BC.CASES["A"]
    L, R, S, info = _decompose(b, r, torch.zeros(E, Tt, Y, X, dtype=torch.complex64))
    assert not L.abs().any() and not R.abs().any() and not S.any()
    assert int(info.max()) <= 1


def test_one_corner():
    """Zero except one block-sized corner: the blocks that do not touch it come out exactly zero."""
    b, E, Tt, Y, X, r = BC.CASES["A"]
    img = torch.zeros(E, Tt, Y, X, dtype=torch.complex64)
    img[:, :, :b, :b] = recipe.crandn(790, (E, Tt, b, b))
    ref = BC.svd64(b, img)
    L, R, S, info = _decompose(b, r, img)
    dead = ref[1][:, 0] == 0
    assert 0 < int(dead.sum()) < dead.numel()
    assert not L[dead].abs().any() and not R[dead].abs().any() and not S[dead].any()
    BC.check_truncation(ref, r, L, R, S, info, label="one corner")


def test_rank_one():
    """All frames equal: one component, the other two zeros (or below 1e-5 sqrt(sigma_1))."""
    b, E, Tt, Y, X, r = BC.CASES["A"]
    img = recipe.crandn(791, (E, 1, Y, X)).expand(E, Tt, Y, X).contiguous()
    ref = BC.svd64(b, img)
    L, R, S, info = _decompose(b, r, img)
    bound = 1e-5 * ref[1][:, 0].sqrt()[:, None, None]
    assert bool((L[:, :, 1:].abs() <= bound).all()) and bool((R[:, :, 1:].abs() <= bound).all())
    BC.check_truncation(ref, r, L, R, S, info, label="rank one")


@pytest.mark.parametrize("name", ["B", "b16"])
def test_bitwise_repeat(results, name):
    b, E, Tt, Y, X, r = BC.CASES[name]
    again = _decompose(b, r, BC.image(name, "gauss"))
    for a, c in zip(results(name, "gauss"), again):
        assert torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(c) if c.is_complex() else c)


def test_limits():
    """Outside the range: NotImplementedError from the wrapper, DLCS_ERR_UNSUPPORTED_SIZE from the
    entry point, which writes nothing; DlcsError for tensors the kernel cannot take."""
    from dl_cs import _lib
    from dl_cs.models import _ops as K
    p = _lib.ptr
    win = torch.ones(32, device=DEV)
    for b, E, Tt, r in ((32, 1, 8, 2), (4, 1, 33, 2), (4, 1, 12, 9), (4, 1, 3, 4), (4, 3, 8, 2), (4, 1, 8, 0)):
        Y = X = 8
        img = recipe.crandn(795, (E, Tt, Y, X)).to(DEV)
        if r >= 1:
            with pytest.raises(NotImplementedError):
                K.lr_decompose(img, win[:b].contiguous(), b, r)
        N = K.lr_num_blocks(Y, X, b)
        L = torch.full((N, E * b * b, max(r, 1)), 7.0, dtype=torch.complex64, device=DEV)
        R = torch.full((N, Tt, max(r, 1)), 7.0, dtype=torch.complex64, device=DEV)
        S = torch.full((N, max(r, 1)), 7.0, device=DEV)
        info = torch.full((N,), 7, dtype=torch.int32, device=DEV)
        status = _lib.lib().dlcs_lr_decompose(p(img), p(win), p(L), p(R), p(S), p(info), E, Tt, Y, X, b, r, _lib.stream())
        torch.cuda.synchronize()
        assert status == 100002, (b, E, Tt, r, status)
        assert bool((L == 7).all()) and bool((R == 7).all()) and bool((S == 7).all()) and bool((info == 7).all())
    b, E, Tt, Y, X, r = BC.CASES["A"]
    op = _op(b, E, Tt, Y, X)
    good = BC.image("A", "gauss")
    from dl_cs.mri import lowrank
    with pytest.raises(_lib.DlcsError):                           # a CPU image
        lowrank.decompose_blocks(good, op, r)
    with pytest.raises(_lib.DlcsError):                           # complex128
        lowrank.decompose_blocks(good.to(DEV).to(torch.complex128), op, r)
    wide = recipe.crandn(796, (E, Tt, Y, 2 * X)).to(DEV)[..., ::2]
    assert not wide.is_contiguous()
    with pytest.raises(_lib.DlcsError):                           # not contiguous
        K.lr_decompose(wide, op.win1d, b, r)
    with pytest.raises(_lib.DlcsError):                           # the operator left on the host
        lowrank.decompose_blocks(good.to(DEV), lowrank.ArrayToBlocks(b, [1, E, Tt, Y, X], True), r)


def test_decompose_module(golden):
    """Decompose(svd='device') at dslr_oracle's case A: the assertions of
    test_lowrank.py::test_decompose against the reference-made goldens, every tensor on the GPU."""
    from dl_cs import _lib
    from dl_cs.mri import lowrank
    g = golden("dslr")
    b, E, Tt, Y, X = D.GEO_CASES["A"]
    dec = lowrank.Decompose(b, D.DEC_RANK, [1, E, Tt, Y, X], True, svd="device")
    img = D.lowrank_image()[None]
    L, R = dec(img.to(DEV))
    assert L.is_cuda and R.is_cuda
    assert tuple(L.shape) == (dec.block_op.num_blocks, E * b * b, D.DEC_RANK)
    assert tuple(R.shape) == (dec.block_op.num_blocks, Tt, D.DEC_RANK)
    assert D.nrmse(g["dec_S"], (L.abs() ** 2).sum(1).cpu().numpy()) <= 1e-5
    assert D.nrmse(g["dec_S"], (R.abs() ** 2).sum(1).cpu().numpy()) <= 1e-5
    out = dec((L, R), adjoint=True)
    assert out.is_cuda and tuple(out.shape) == (1, E, Tt, Y, X)
    assert D.nrmse(g["dec_img"], out[0].cpu().numpy()) <= 1e-5
    assert D.nrmse(img.numpy(), out.cpu().numpy()) < 0.05
    assert D.nrmse(out.cpu().numpy(), dec.compose(L, R).cpu().numpy()) == 0
    with pytest.raises(_lib.DlcsError):
        dec(img)


def test_preprocess_device_svd():
    """CinePreprocess(lr_decom=True, lr_svd='device', device=cuda) at the configuration of
    test_preprocess_lr_decom_cpu: the factors from the kernel, the other six items unchanged."""
    import types
    from dl_cs.data.preprocess import CinePreprocess
    from dl_cs.mri import lowrank
    N = types.SimpleNamespace
    cfg = N(AUG_TRAIN=N(UNDERSAMPLE=N(ACCELERATIONS=(4, 6), PARTIAL_KX=0.25, PARTIAL_KY=0.25), CROP_READOUT=0, ZPAD_PE=0),
            MODEL=N(PARAMETERS=N(SLWIN_INIT=True, DSLR=N(BLOCK_SIZE=4, NUM_BASIS=2, OVERLAPPING=True))))
    C, Tt, Y, X, E = 3, 6, 12, 10, 2
    k = recipe.crandn(1, (C, Tt, Y, X)).numpy()
    maps = recipe.sense_maps(2, 1, E, C, Y, X)[0].numpy()
    target = recipe.crandn(3, (E, Tt, Y, X)).numpy()
    host = CinePreprocess(cfg, lr_decom=True, use_seed=True, device=DEV)(k, maps, target, "slice.h5")
    dev = CinePreprocess(cfg, lr_decom=True, use_seed=True, device=DEV, lr_svd="device")(k, maps, target, "slice.h5")
    assert len(host) == 8 and len(dev) == 8
    for i in (0, 1, 2, 5, 6, 7):
        assert dev[i].is_cuda and torch.equal(host[i], dev[i])
    L, R, init = dev[3], dev[4], dev[5]
    assert L.is_cuda and R.is_cuda
    op = lowrank.ArrayToBlocks(4, [1, E, Tt, Y, X], True)
    assert tuple(L.shape) == (op.num_blocks, E * 16, 2) and tuple(R.shape) == (op.num_blocks, Tt, 2)
    ref = BC.svd64(4, init.cpu())
    e = D.nrmse(BC.truncation(ref, 2).numpy(), torch.bmm(L, R.conj().transpose(1, 2)).cpu().numpy())
    print(f"preprocess, device SVD: L R^H against the float64 truncation: NRMSE {e:.3g}")
    assert e <= 1e-5


def test_reconstruct_lr_device_svd(tmp_path):
    """scripts/reconstruct_lr.py --svd device on the scan and model of test_gpu_reconstruct_lr.py."""
    import numpy as np
    import test_gpu_reconstruct_lr as TR
    from dl_cs import checkpoint
    from dl_cs.config import load_cfg
    from dl_cs.fileio import cfl
    from dl_cs.mri import lowrank, transforms as Tr
    from dl_cs.models import swin3D
    rl = T._script("reconstruct_lr")
    TR._write_scan(tmp_path)
    (tmp_path / "dslr.yaml").write_text(T.LR_CFG.format(out=str(tmp_path / "out"), arch="modslr-v1"))
    config = load_cfg(str(tmp_path / "dslr.yaml"))
    model = D.fill(rl.train_lr.build_model(config), 91)
    checkpoint.save(str(tmp_path / "m.ckpt"), model)
    try:
        rl.main(TR._args(rl, tmp_path, "--svd", "device"))
        im = cfl.read(str(tmp_path / "im.dl"), order='F')
        assert im.shape == (TR.X, TR.Y, TR.S, 1, TR.E, 1, 1, TR.PH)
        assert np.isfinite(im).all() and np.abs(im).max() > 0

        dev = torch.device("cuda", 0)
        model = model.eval().to(dev)
        data = rl.CflDataset(str(tmp_path / "ks"), str(tmp_path / "maps"))
        tf, tf_host = rl.LrTransform(config, dev, svd="device"), rl.LrTransform(config, dev)
        op = lowrank.ArrayToBlocks(4, [1, TR.E, TR.PH, TR.Y, TR.X], overlapping=True).to(dev)
        direct = []
        with torch.no_grad():
            for i in range(len(data)):
                ks, mp, mask, L0, R0, scale = tf(*data[i])
                assert L0.is_cuda and R0.is_cuda
                Lh, Rh = tf_host(*data[i])[3:5]
                e = D.nrmse(torch.bmm(Lh, D.bt(Rh)).cpu().numpy(), torch.bmm(L0, D.bt(R0)).cpu().numpy())
                print(f"slice {i}: L R^H of the device factors against the host factors': NRMSE {e:.3g}")
                assert e <= 1e-5
                pred = model(y=ks[None], A=Tr.SenseModel(mp[None], weights=mask[None]), BlockOp=op, L0=L0, R0=R0)
                direct.append((scale * pred)[0].cpu().numpy())
        got = np.transpose(im[:, :, :, 0, :, 0, 0, :], (2, 3, 4, 1, 0))
        e = D.nrmse(np.stack(direct), got)
        print(f"reconstruct_lr --svd device vs the direct call: NRMSE {e:.3g}")
        assert e <= 1e-6
    finally:
        swin3D.set_compute_dtype(torch.float32)


def test_train_lr_device_svd(tmp_path, monkeypatch):
    """scripts/train_lr.py --svd device: one optimiser step with the factors from the kernel."""
    import json
    import math
    from dl_cs import checkpoint
    from dl_cs.config import load_cfg
    from dl_cs.models import _ops as K
    out = tmp_path / "out"
    cfg = tmp_path / "dslr.yaml"
    cfg.write_text(T.LR_CFG.format(out=str(out), arch="modslr-v1"))
    calls = []
    raw = K.lr_decompose
    monkeypatch.setattr(K, "lr_decompose", lambda *a, **k: (calls.append(1), raw(*a, **k))[1])
    tr = T._script("train_lr")
    tr.main(["--config-file", str(cfg), "--data", "synthetic", "--synthetic-slices", "2",
             "--synthetic-shape", "4", "2", "8", "16", "24", "--svd", "device", "--max-steps", "1"])
    assert calls                                                  # the kernel made the factors
    recs = [json.loads(line) for line in (out / "exp" / "metrics.jsonl").read_text().splitlines()]
    train = [r for r in recs if "Train/complex_l1" in r]
    assert len(train) == 1 and math.isfinite(train[0]["Train/complex_l1"])
    ck = torch.load(out / "last.ckpt", weights_only=True)
    assert ck["global_step"] == 1
    torch.manual_seed(load_cfg(str(cfg)).SEED)                    # the trainer's initial parameters
    init = tr.build_model(load_cfg(str(cfg))).state_dict()
    sd = checkpoint.model_state_dict(ck)
    changed = [k for k in init if k in sd and not torch.equal(init[k], sd[k].cpu())]
    assert set(init) <= set(sd) and changed
