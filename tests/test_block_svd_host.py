"""The block SVD switch without a GPU: the command lines, the constructors, the binding,
and the preconditions of tests/block_svd_cases.py on the float64 reference alone."""
import pytest
import torch

import block_svd_cases as BC
import test_gpu_dslr as T


def test_parsers_accept_svd():
    rl = T._script("reconstruct_lr")
    base = ["--directory", "d", "--ckpt", "c", "--config-file", "f"]
    a = rl.create_arg_parser().parse_args(base)
    assert a.svd == "host"
    assert (a.kspace, a.maps, a.out, a.batch_size, a.device, a.multi_gpu, a.verbose, a.dtype) == \
        ("ks", "maps", "im.dl", 1, -1, False, False, "fp32")
    assert rl.create_arg_parser().parse_args(base + ["--svd", "device"]).svd == "device"
    with pytest.raises(SystemExit):
        rl.create_arg_parser().parse_args(base + ["--svd", "lapack"])
    tr = T._script("train_lr")
    assert tr.create_arg_parser().parse_args(["--config-file", "f"]).svd == "host"
    assert tr.create_arg_parser().parse_args(["--config-file", "f", "--svd", "device"]).svd == "device"


def test_decompose_constructs_without_gpu():
    from dl_cs import _lib
    from dl_cs.mri import lowrank
    dec = lowrank.Decompose(4, 2, [1, 2, 5, 12, 20], True, svd="device")
    assert dec.svd == "device" and dec.block_op.win1d.device.type == "cpu"
    assert sorted(dec.state_dict()) == sorted(lowrank.Decompose(4, 2, [1, 2, 5, 12, 20], True).state_dict())
    with pytest.raises(_lib.DlcsError):                           # the kernel takes a GPU image
        dec(torch.zeros(1, 2, 5, 12, 20, dtype=torch.complex64))
    with pytest.raises(AssertionError):
        lowrank.Decompose(4, 2, [1, 2, 5, 12, 20], True, device="cuda")
    with pytest.raises(AssertionError):
        lowrank.Decompose(4, 2, [1, 2, 5, 12, 20], True, device="cuda", svd="device")
    assert lowrank.Decompose(4, 2, [1, 2, 5, 12, 20], True).svd == "host"


def test_binding_declares_decompose():
    from dl_cs import _lib
    assert len(_lib.SIGNATURES["dlcs_lr_decompose"]) == 13


def test_ops_range_before_any_device_check():
    """Outside the range the wrapper raises NotImplementedError whatever the tensors are."""
    from dl_cs.models import _ops
    win = torch.ones(4)
    for b, T_, r in ((32, 8, 2), (4, 33, 2), (4, 9, 9), (4, 3, 4)):
        with pytest.raises(NotImplementedError):
            _ops.lr_decompose(torch.zeros(1, T_, 8, 8, dtype=torch.complex64), win, b, r)


@pytest.mark.parametrize("name", list(BC.CASES))
def test_case_preconditions(name):
    b, E, T_, Y, X, r = BC.CASES[name]
    share = BC.left_out_share(name)
    U, S, Vh = BC.reference(name, "lowrank")
    full = int((S[:, r - 1] > 1e-6 * S[:, 0].max()).sum())
    print(f"{name}: {S.shape[0]} blocks, {100 * share:.1f} % of the components left out, {full} blocks of rank >= {r}")
    assert share <= BC.MAX_LEFT_OUT
    assert full >= 1
