"""dlcs_fft_plan (host only, no GPU): which of the three plan cases every line
length 1..1024 takes -- 2-3-5-smooth Stockham passes, extra passes of 7 / 11 / 13,
or Bluestein at the smallest 2-3-5-smooth padded length >= 2n - 1."""
import ctypes
import os

import pytest

UNSUPPORTED_SIZE = 100002  # DLCS_ERR_UNSUPPORTED_SIZE (include/dlcs.h)


def _lib():
    from dl_cs import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libdlcs_hip.so not built")
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.dlcs_fft_plan.argtypes = [ctypes.c_int64, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.dlcs_fft_plan.restype = ctypes.c_int
    return L


def _plan(L, n):
    kind, padded = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.dlcs_fft_plan(n, ctypes.byref(kind), ctypes.byref(padded))
    return rc, kind.value, padded.value


def _strip(n, radices):
    for r in radices:
        while n % r == 0:
            n //= r
    return n


def _smooth(n):
    return _strip(n, (2, 3, 5)) == 1


def _expected_kind(n):
    rest = _strip(n, (4, 2, 3, 5))
    if rest == 1:
        return 0
    return 1 if _strip(rest, (7, 11, 13)) == 1 else 2


def test_every_length_takes_the_stated_case():
    L = _lib()
    counts = [0, 0, 0]
    for n in range(1, 1025):
        rc, kind, padded = _plan(L, n)
        assert rc == 0, n
        assert kind == _expected_kind(n), n
        counts[kind] += 1
        if kind == 2:
            assert padded >= 2 * n - 1, n
            assert _smooth(padded), (n, padded)
            assert not any(_smooth(m) for m in range(2 * n - 1, padded)), (n, padded)
            assert padded <= 2048, (n, padded)
        else:
            assert padded == n, n
    assert all(counts), counts


@pytest.mark.parametrize("n, kind, padded", [
    (192, 0, 192), (224, 1, 224), (1001, 1, 1001), (17, 2, 36), (246, 2, 500), (1021, 2, 2048)])
def test_spot_values(n, kind, padded):
    assert _plan(_lib(), n) == (0, kind, padded)


@pytest.mark.parametrize("n", [0, 1025, -3, 1 << 40])
def test_outside_range_is_unsupported(n):
    L = _lib()
    assert _plan(L, n)[0] == UNSUPPORTED_SIZE
    # never touches the outputs it cannot fill, and takes NULL outputs
    assert L.dlcs_fft_plan(n, None, None) == UNSUPPORTED_SIZE
    assert L.dlcs_fft_plan(224, None, None) == 0
