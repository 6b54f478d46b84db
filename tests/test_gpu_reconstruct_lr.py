"""scripts/reconstruct_lr.py: CFL k-space in, CFL images out with a DSLR checkpoint.

A small scan (kx 24, ky 16, 2 slices, 4 coils, 1 echo, 8 phases, 2 maps) and a modslr-v1
model filled by the recipe: the output has the reference's layout [x, y, sl, 1, emap, ec, 1,
ph] and equals the same model called directly on the same transform's tensors, times the
scale; --dtype bf16 stays within the bf16 budget (1e-2) of the fp32 output.  The argument
parser and the CFL dimension bookkeeping are checked without a GPU.
"""
import numpy as np
import pytest
import torch

import dslr_oracle as D
import test_gpu_dslr as T

X, Y, S, C, E, PH = 24, 16, 2, 4, 2, 8


@pytest.fixture(autouse=True)
def _fp32_after():
    yield
    from dl_cs.models import swin3D
    swin3D.set_compute_dtype(torch.float32)


def _write_scan(tmp_path):
    from dl_cs.data.dataset import SyntheticCineDataset
    from dl_cs.fileio import cfl
    ds = SyntheticCineDataset(S, lambda k, m, t, f: (k, m), coils=C, emaps=E, frames=PH, ny=Y, nx=X, seed=5)
    ks = np.stack([ds[i][0] for i in range(S)])                  # [sl, C, T, Y, X]
    maps = np.stack([ds[i][1] for i in range(S)])                # [sl, E, C, 1, Y, X]
    ks[:, :, :, ::3] = 0                                         # undersample ky
    cfl.write(str(tmp_path / "ks"), ks.transpose(4, 3, 0, 1, 2).reshape(X, Y, S, C, 1, 1, 1, PH), order='F')
    cfl.write(str(tmp_path / "maps"), maps[:, :, :, 0].transpose(4, 3, 0, 2, 1), order='F')


def _args(rl, tmp_path, *extra):
    return rl.create_arg_parser().parse_args(["--directory", str(tmp_path), "--ckpt", str(tmp_path / "m.ckpt"),
                                              "--config-file", str(tmp_path / "dslr.yaml"), "--device", "0", *extra])


@pytest.mark.gpu
def test_reconstruct_lr(tmp_path):
    from dl_cs import checkpoint
    from dl_cs.config import load_cfg
    from dl_cs.fileio import cfl
    from dl_cs.mri import lowrank, transforms as Tr
    from dl_cs.models import swin3D
    rl = T._script("reconstruct_lr")
    _write_scan(tmp_path)
    (tmp_path / "dslr.yaml").write_text(T.LR_CFG.format(out=str(tmp_path / "out"), arch="modslr-v1"))
    config = load_cfg(str(tmp_path / "dslr.yaml"))
    model = D.fill(rl.train_lr.build_model(config), 91)          # recipe.fill_module, the MoDL penalties kept
    checkpoint.save(str(tmp_path / "m.ckpt"), model)

    rl.main(_args(rl, tmp_path))
    im = cfl.read(str(tmp_path / "im.dl"), order='F')
    assert im.shape == (X, Y, S, 1, E, 1, 1, PH)
    assert np.isfinite(im).all() and np.abs(im).max() > 0

    # the same model on the same transform's tensors, times the scale
    swin3D.set_compute_dtype(torch.float32)
    dev = torch.device("cuda", 0)
    model = model.eval().to(dev)
    data = rl.CflDataset(str(tmp_path / "ks"), str(tmp_path / "maps"))
    tf = rl.LrTransform(config, dev)
    op = lowrank.ArrayToBlocks(4, [1, E, PH, Y, X], overlapping=True).to(dev)
    direct = []
    with torch.no_grad():
        for i in range(len(data)):
            ks, mp, mask, L0, R0, scale = tf(*data[i])
            assert tuple(L0.shape) == (op.num_blocks, E * 16, 3) and tuple(R0.shape) == (op.num_blocks, PH, 3)
            pred = model(y=ks[None], A=Tr.SenseModel(mp[None], weights=mask[None]), BlockOp=op, L0=L0, R0=R0)
            direct.append((scale * pred)[0].cpu().numpy())
    direct = np.stack(direct)                                    # [sl, em, ph, y, x]
    got = np.transpose(im[:, :, :, 0, :, 0, 0, :], (2, 3, 4, 1, 0))
    e = D.nrmse(direct, got)
    print(f"reconstruct_lr fp32 vs the direct call: NRMSE {e:.3g}")
    assert e <= 1e-6

    rl.main(_args(rl, tmp_path, "--dtype", "bf16", "--out", "im.bf16"))
    assert swin3D.get_compute_dtype() == torch.bfloat16
    im16 = cfl.read(str(tmp_path / "im.bf16"), order='F')
    e16 = D.nrmse(im, im16)
    print(f"reconstruct_lr bf16 vs fp32: NRMSE {e16:.3g}")
    assert im16.shape == im.shape and 0 < e16 <= 1e-2

    with pytest.raises(NotImplementedError):
        rl.main(_args(rl, tmp_path, "--batch-size", "2"))
    with pytest.raises(NotImplementedError):
        rl.main(_args(rl, tmp_path, "--multi-gpu"))


def test_reconstruct_lr_parser_and_cfl_dims(tmp_path):
    """No GPU: the reference's command line plus --dtype; the examples are echo major; write is
    the inverse of read."""
    from dl_cs.fileio import cfl
    rl = T._script("reconstruct_lr")
    a = rl.create_arg_parser().parse_args(["--directory", "d", "--ckpt", "c", "--config-file", "f"])
    assert (a.kspace, a.maps, a.out, a.batch_size, a.device, a.multi_gpu, a.verbose, a.dtype) == \
        ("ks", "maps", "im.dl", 1, -1, False, False, "fp32")
    a = rl.create_arg_parser().parse_args(["--directory", "d", "--ckpt", "c", "--config-file", "f", "--kspace", "k", "--maps",
                                           "m", "--out", "o", "--batch-size", "3", "--device", "1", "--multi-gpu",
                                           "--verbose", "--dtype", "bf16"])
    assert (a.kspace, a.maps, a.out, a.batch_size, a.device, a.multi_gpu, a.verbose, a.dtype) == \
        ("k", "m", "o", 3, 1, True, True, "bf16")
    for bad in (["--batch-size", "2"], ["--multi-gpu"]):          # refused before anything is loaded
        with pytest.raises(NotImplementedError):
            rl.main(rl.create_arg_parser().parse_args(["--directory", "d", "--ckpt", "c", "--config-file", "f"] + bad))

    Ec, x, y, s, c, ph, em = 2, 5, 4, 3, 2, 3, 2
    rng = np.random.default_rng(7)
    ks = (rng.standard_normal((x, y, s, c, 1, Ec, 1, ph)) + 1j * rng.standard_normal((x, y, s, c, 1, Ec, 1, ph))).astype(np.complex64)
    maps = (rng.standard_normal((x, y, s, c, em)) + 1j * rng.standard_normal((x, y, s, c, em))).astype(np.complex64)
    cfl.write(str(tmp_path / "ks"), ks, order='F')
    cfl.write(str(tmp_path / "maps"), maps, order='F')
    data = rl.CflDataset(str(tmp_path / "ks"), str(tmp_path / "maps"))
    assert len(data) == Ec * s and data.examples == [(sl, ec) for ec in range(Ec) for sl in range(s)]
    for i, (sl, ec) in enumerate(data.examples):
        k, m = data[i]
        assert k.shape == (c, ph, y, x) and m.shape == (em, c, 1, y, x)
        assert np.array_equal(k, ks[:, :, sl, :, 0, ec, 0, :].transpose(2, 3, 1, 0))
        assert np.array_equal(m[:, :, 0], maps[:, :, sl].transpose(3, 2, 1, 0))
    # one echo: images in example order [sl, em, ph, y, x] come back as [x, y, sl, 1, em, 1, 1, ph]
    cfl.write(str(tmp_path / "k1"), ks[:, :, :, :, :, :1], order='F')
    one = rl.CflDataset(str(tmp_path / "k1"), str(tmp_path / "maps"))
    images = (rng.standard_normal((s, em, ph, y, x)) + 1j * rng.standard_normal((s, em, ph, y, x))).astype(np.complex64)
    one.write(str(tmp_path / "im"), images)
    im = cfl.read(str(tmp_path / "im"), order='F')
    assert im.shape == (x, y, s, 1, em, 1, 1, ph)
    assert np.array_equal(np.transpose(im[:, :, :, 0, :, 0, 0, :], (2, 3, 4, 1, 0)), images)
