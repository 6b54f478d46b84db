"""Micro-benchmark of the dense SENSE operator at any in-plane matrix: forward,
adjoint and the fused PGD normal-op + DC update (1 x 2 maps x 8 coils x 20
frames, 10 % element mask, DLCS_SENSE_ROWS=0), the timing loop of
tools/sense_bench.py with (Y, X) from the command line.  Per size and operator:
median us per op over --reps windows of --iters calls (min and max beside it),
the share of 8 TB/s on algorithmic bytes (each operand read or written once),
the ratio to the first size given, and a digest of the output bits (the same
library on the same size must print the same digest).

    python tools/sense_sizes_bench.py 240x200 224x208 246x204 [--iters 200] [--reps 5]

A size the library refuses is reported as such and skipped.  dlcs_fft_plan's
(kind, padded length) per axis is printed where the library has it."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

os.environ.setdefault("DLCS_DIAG", "1")         # DLCS_SENSE_ROWS is a diagnostic switch
os.environ["DLCS_SENSE_ROWS"] = "0"

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dl-swin-gan_amd"))
import torch  # noqa: E402
from dl_cs import _lib  # noqa: E402
from dl_cs.mri import transforms as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="+", help="YxX, e.g. 240x200")
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"
dev = "cuda"
B, E, C, Tt = 1, 2, 8, 20
HBM_GBS = 8000.0


def plan(n):
    if not _lib.has_symbol("dlcs_fft_plan"):
        return None
    kind, padded = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.call("dlcs_fft_plan", n, ctypes.byref(kind), ctypes.byref(padded))
    return kind.value, padded.value


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.iters


def digest(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]


first = {}
for size in args.sizes:
    Y, X = (int(v) for v in size.lower().split("x"))
    g = torch.Generator(device=dev).manual_seed(0)
    cr = lambda *s: torch.complex(torch.randn(s, device=dev, generator=g), torch.randn(s, device=dev, generator=g))  # noqa: E731
    maps = cr(B, E, C, 1, Y, X)
    mask = (torch.rand((B, 1, Tt, Y, X), device=dev, generator=g) < 0.1).float()
    x, y = cr(B, E, Tt, Y, X), cr(B, C, Tt, Y, X)
    A = T.SenseModel(maps, weights=mask)
    img, ksp = B * E * Tt * Y * X * 8, B * C * Tt * Y * X * 8
    mb, wb = B * E * C * Y * X * 8, B * Tt * Y * X * 4
    with torch.no_grad():
        try:
            aty = A(y, adjoint=True)
        except _lib.DlcsError as e:
            print(json.dumps({"size": size, "skipped": str(e)}), flush=True)
            continue
        ops = [("forward", lambda: A(x), img + mb + wb + ksp),
               ("adjoint", lambda: A(y, adjoint=True), ksp + mb + wb + img),
               ("normal_dc", lambda: A.normal_dc(x, aty, -2.0), 3 * img + mb + wb)]
        for name, fn, nbytes in ops:
            for _ in range(10):
                out = fn()
            torch.cuda.synchronize()
            us = sorted(window(fn) for _ in range(args.reps))
            med = statistics.median(us)
            first.setdefault(name, med)
            print(json.dumps({"size": size, "plan_y": plan(Y), "plan_x": plan(X), "op": name,
                              "us": round(med, 1), "us_min": round(us[0], 1), "us_max": round(us[-1], 1),
                              "bytes": nbytes, "pct_of_8TBs": round(nbytes / med / 1e3 / HBM_GBS * 100, 2),
                              "ratio_to_first": round(med / first[name], 3), "digest": digest(out)}), flush=True)
