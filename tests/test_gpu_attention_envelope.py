"""The whole contract of dlcs_window_attn_fwd / dlcs_window_attn_bwd (csrc/attention.hip,
attention_f32.inc, attention_h3.inc): every head dim 4 .. 32, any head count, windows other
than (7, 8, 8), the three mask modes, fp32 and bf16, the launches that fall back on the LDS
limit, the refusals and the write promises of include/dlcs.h.

Every call goes through dl_cs._lib.call into buffers between two 64-element sentinel margins
(test_gpu_glue_kernels._Out); out, lse and dqkv start as NaN, so an element the kernel skips,
or a write outside the buffer, fails the test.  References are float64 on the CPU on the
operands the kernel receives (goldutil.attn_reference; bf16 operands rounded first, scale * q
rounded to bf16 for the bf16 kernels as in test_gpu_kernels.py).

Bars are the existing ones: fp32 NRMSE < 1e-5 (test_window_attention_f32_kernels), bf16 1e-2
forward and 2e-2 backward (test_window_attention_bf16_kernels; the bf16 log-sum-exp, fp32
arithmetic on bf16 operands, is held to the fp32 bar, see _bars), the fp16-split
(h3) kernels max(1e-6, 4 x torch's own fp32 distance from float64) (test_window_attention_h3_floor).

  kernel family                          reached by                              test
  -------------------------------------  --------------------------------------  ---------------------------------
  generic fp32 forward                   fp32, head dim != 20                    test_attn_head_dims,
    attn_fwd_kernel<float>                                                       test_attn_table_gradient_wide_span,
                                                                                 test_attn_write_contract,
                                                                                 test_attn_window_isolation,
                                                                                 test_swin_block_other_geometry
  generic fp32 backward                  fp32, head dim != 20; N = 200: two key  the same; test_attn_head_dims
    attn_bwd_kernel<float>               groups (dQ atomics across groups)       [f32-N200]
  bf16 forward                           bf16, any head dim                      test_attn_head_dims, _wide_span,
    attn_fwd_v2_kernel                                                           _write_contract, _window_isolation
  bf16 backward                          bf16, any head dim                      the same
    attn_bwd_kv_kernel, attn_bwd_q_kernel
  h3 forward                             fp32, head dim 20, LDS image fits       _wide_span [h3], _write_contract
    attn_fwd_h3_kernel                                                           [h3], _window_isolation [h3]
  h3 backward                            fp32, head dim 20, LDS images fit       the same
    attn_bwd_kv_h3_kernel, attn_bwd_q_h3_kernel
  f32-MFMA forward                       fp32, head dim 20, window0 (8, 8, 9),   test_attn_f32_mfma_by_lds_limit,
    attn_fwd_f32_kernel<20, MM, RAGGED>  N = 544 / 530: the h3 image is 175 KB   _wide_span [f32mfma],
                                                                                 _write_contract [f32mfma],
                                                                                 test_attn_refuses_oversize (fwd)
  f32-MFMA backward                      the same sizes: the h3 dK / dV kernel   the same; _refuses_oversize: at
    attn_bwd_kv_f32_kernel<20, MM>,      needs 193 KB, this one 157 776 B        N = 576 it needs 163 932 B and
    attn_bwd_q_f32_kernel<20, MM>                                                the call is refused

  refusals (head dim 36 / 6, N = 1025, misaligned qkv)                           test_attn_refusals
  which tiles leave the table-gradient bins, which launch fits the LDS           test_attn_geometry_mirror
"""
from types import SimpleNamespace

import pytest
import torch

from goldutil import attn_fwd_dtype, attn_reference, nrmse
from test_gpu_glue_kernels import _Out

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
MODES = ["labels", "mask", "plain"]
UNSUPPORTED = "100002"            # DLCS_ERR_UNSUPPORTED_SIZE (include/dlcs.h)
LDS_LIMIT = 160 * 1024
K_BINS, K_H3_BINS = 128, 112      # attention.hip kBins, attention_h3.inc kH3Bins
W788, W889 = (7, 8, 8), (8, 8, 9)


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


# ============================================================================ geometry mirror
def _rel_term(t, w0):
    """attention.hip rel_term: token t of the constructed window -> its relative-position term."""
    _, wh, ww = w0
    d, h, w = t // (wh * ww), (t // ww) % wh, t % ww
    return (d * (2 * wh - 1) + h) * (2 * ww - 1) + w


def _nrel(w0):
    return (2 * w0[0] - 1) * (2 * w0[1] - 1) * (2 * w0[2] - 1)


def _tile_spans(w0, N):
    """The `span` every backward kernel computes for each 32 x 32 (query block, key block)
    tile: (f_hi - f_lo of the query block) + (f_hi - f_lo of the key block) + 1."""
    rng = []
    for b in range((N + 31) // 32):
        f = [_rel_term(t, w0) for t in range(b * 32, min(N, b * 32 + 32))]
        rng.append(max(f) - min(f))
    return [q + k + 1 for q in rng for k in rng]


def _span_counts(w0, N):
    """(nrel, tiles, tiles with span > 128, tiles with span in (112, 128])"""
    s = _tile_spans(w0, N)
    return (_nrel(w0), len(s), sum(x > K_BINS for x in s), sum(K_H3_BINS < x <= K_BINS for x in s))


def _lds_bytes(w0, N):
    """LDS bytes of the head-dim-20 fp32 launches (fwd_h3_smem, fwd_f32_smem<20>, bwd_kv_h3_smem
    + the static bins / bwd_q_h3_smem, bwd_kv_f32_smem<20> / bwd_q_f32_smem<20>)."""
    Np, nrel = (N + 31) // 32 * 32, _nrel(w0)
    nrp, nb = (nrel + 3) // 4 * 4, (N + 31) // 32
    h3_bins = 2 * 7 * 2 * (K_H3_BINS + 1) * 4
    return SimpleNamespace(
        fwd_h3=2 * Np * 32 * 2 + 2 * 32 * (Np + 8) * 2 + nrp * 8 + Np * 8 + nb * 4 + 16,
        fwd_f32=Np * 46 * 4 + nrel * 8 + Np * 8 + nb * 4,
        bwd_h3=max(4 * Np * 32 * 2 + 2 * nrp * 4 + 5 * Np * 4 + nb * 12 + 32 + h3_bins,
                   4 * Np * 32 * 2 + 2 * nrp * 4 + 2 * Np * 4 + nb * 4 + 32),
        bwd_f32=max(2 * Np * 22 * 4 + 3 * nrel * 4 + 4 * Np * 4 + 7 * 2 * (K_BINS + 1) * 4 + nb * 12,
                    2 * Np * 22 * 4 + 2 * nrel * 4 + 2 * Np * 4 + nb * 4))


# window0, N -> (nrel, tiles, span > 128, span in (112, 128])
GEOMETRY = {
    ((2, 7, 7), 98): (507, 16, 7, 0),       # ragged, both branches
    ((4, 4, 4), 64): (343, 4, 4, 0),        # every tile on the fallback
    ((2, 6, 6), 72): (363, 9, 3, 3),        # separates the h3 kernel's 112 from 128
    (W788, 100): (2925, 16, 0, 0),          # control: every tile in the bins
    (W889, 530): (3825, 289, 168, 91),      # the f32-MFMA sizes (LDS limit)
    (W889, 544): (3825, 289, 168, 112),
}


def test_attn_geometry_mirror():
    """Pure host arithmetic, asserted before any launch: how many tiles of each tested geometry
    leave the table-gradient bins (span > 128; > 112 in the h3 kernel), and which head-dim-20
    launches fit the 160 KB of LDS.  A change of geometry or of an LDS layout that stops a test
    below from reaching its branch fails here.

    window0 (8, 8, 9), Np = 544: h3 forward 175 348 B, f32-MFMA forward 135 116 B, h3 backward
    193 660 B, f32-MFMA backward 157 776 B; Np = 576: f32-MFMA forward 141 264 B, f32-MFMA
    backward 163 932 B > 163 840.  (8, 8, 8), Np = 512: h3 forward 163 280 B (still fits)."""
    for (w0, N), want in GEOMETRY.items():
        assert _span_counts(w0, N) == want, (w0, N, _span_counts(w0, N))
    for N in (530, 544):
        b = _lds_bytes(W889, N)
        assert (b.fwd_h3, b.fwd_f32, b.bwd_h3, b.bwd_f32) == (175348, 135116, 193660, 157776)
        assert b.fwd_h3 > LDS_LIMIT >= b.fwd_f32 and b.bwd_h3 > LDS_LIMIT >= b.bwd_f32
    b = _lds_bytes(W889, 576)
    assert (b.fwd_f32, b.bwd_f32) == (141264, 163932)
    assert b.fwd_h3 > LDS_LIMIT >= b.fwd_f32 and b.bwd_h3 > LDS_LIMIT and b.bwd_f32 > LDS_LIMIT
    assert _lds_bytes((8, 8, 8), 512).fwd_h3 == 163280
    for N in (64, 72, 98, 100, 200):                   # the small cases stay on the h3 kernels
        b = _lds_bytes(W788, N)
        assert b.fwd_h3 <= LDS_LIMIT and b.bwd_h3 <= LDS_LIMIT


# ============================================================================ problems, launches
def _problem(seed, dtype, nwin, N, heads, hd, window, mode, mask_nw=2):
    C = heads * hd
    p = SimpleNamespace(dtype=dtype, nwin=nwin, N=N, heads=heads, hd=hd, C=C, window=tuple(window), mode=mode,
                        scale=hd ** -0.5, nrel=_nrel(window))
    p.qkv = (_rnd((nwin * N, 3 * C), seed) * 1.5).to(dtype)
    p.table = _rnd((p.nrel, heads), seed + 1) * 0.3
    p.labels = (_rnd((nwin * N,), seed + 2).abs() * 2).int().clamp(max=3) if mode == "labels" else None
    p.mask = torch.where(_rnd((mask_nw, N, N), seed + 3) > 0.8, -100.0, 0.0) if mode == "mask" else None
    p.dout = _rnd((nwin * N, C), seed + 4).to(dtype)
    return p


def _window_of(p, w):
    """Window w of problem p as a problem of its own (contiguous rows, its labels / mask slice)."""
    r = slice(w * p.N, (w + 1) * p.N)
    s = SimpleNamespace(**vars(p))
    s.nwin = 1
    s.qkv, s.dout = p.qkv[r].contiguous(), p.dout[r].contiguous()
    s.labels = p.labels[r].contiguous() if p.labels is not None else None
    s.mask = p.mask[w % p.mask.shape[0]][None].contiguous() if p.mask is not None else None
    return s


def _reference(p):
    """float64 (out, lse, dq, dk, dv, dtable) on the operands as the kernel receives them."""
    o, g, dt, lse = attn_reference(p.qkv, p.table, p.labels, p.mask, p.nwin, p.N, p.heads, p.hd, p.window,
                                   p.scale, p.dout, round_q=p.dtype == BF16, with_lse=True)
    C = p.C
    return (o, lse, g[:, :C], g[:, C:2 * C], g[:, 2 * C:], dt)


def _torch_f32(p):
    o, lse, g, dt = attn_fwd_dtype(p.qkv, p.table, p.labels, p.mask, p.nwin, p.N, p.heads, p.hd, p.window,
                                   p.scale, F32, p.dout)
    C = p.C
    return (o, lse, g[:, :C], g[:, C:2 * C], g[:, 2 * C:], dt)


class _Launch:
    """The device operands of a problem and its guarded outputs: out, lse and dqkv start as
    NaN, dtable as `dtable0` (default zeros)."""

    def __init__(self, p, dtable0=None):
        K = _K()
        self.p = p
        self.qkv, self.table, self.dout = p.qkv.to(DEV), p.table.to(DEV), p.dout.to(DEV)
        self.labels = p.labels.to(DEV) if p.labels is not None else None
        self.mask = p.mask.to(DEV).contiguous() if p.mask is not None else None
        self.mask_nw = p.mask.shape[0] if p.mask is not None else 0
        rows = p.nwin * p.N
        self.out = _Out((rows, p.C), p.dtype, init=NAN)
        self.lse = _Out((p.nwin, p.heads, p.N), F32, init=NAN)
        self.dqkv = _Out((rows, 3 * p.C), F32, init=NAN)
        self.dtable = _Out((p.nrel, p.heads), F32, init=0.0 if dtable0 is None else dtable0)
        self.code = K.code(p.dtype)

    def fwd(self, qkv=None):
        K, p = _K(), self.p
        _call("dlcs_window_attn_fwd", self.code, K.p(self.qkv if qkv is None else qkv), K.p(self.out.t),
              K.p(self.lse.t), K.p(self.table), K.p(self.labels), K.p(self.mask), self.mask_nw, p.nwin, p.N,
              p.heads, p.hd, p.window[0], p.window[1], p.window[2], float(p.scale), K.S())

    def bwd(self, qkv=None):
        """The backward on the output and log-sum-exp the forward left in the guarded buffers."""
        K, p = _K(), self.p
        _call("dlcs_window_attn_bwd", self.code, K.p(self.qkv if qkv is None else qkv), K.p(self.out.t),
              K.p(self.dout), K.p(self.lse.t), K.p(self.table), K.p(self.labels), K.p(self.mask), self.mask_nw,
              K.p(self.dqkv.t), K.p(self.dtable.t), p.nwin, p.N, p.heads, p.hd, p.window[0], p.window[1],
              p.window[2], float(p.scale), K.S())

    def results(self):
        """(out, lse, dq, dk, dv, dtable) on the CPU; checks every margin."""
        torch.cuda.synchronize()
        C = self.p.C
        g = self.dqkv.get()
        return (self.out.get(), self.lse.get(), g[:, :C], g[:, C:2 * C], g[:, 2 * C:], self.dtable.get())


NAMES = ("out", "lse", "dq", "dk", "dv", "dtable")


def _bars(dtype):
    """(out, lse, dq, dk, dv, dtable).  The bf16 log-sum-exp is held to the fp32 bar: the scores
    are fp32 sums of exact products of bf16 operands and the row sum is taken in fp32 before P
    is rounded, so it carries fp32 error only -- and one padded key let into a row moves it by
    about 1 / N, which the 1e-2 bar on the bf16 output cannot see."""
    return (1e-2, 1e-5, 2e-2, 2e-2, 2e-2, 2e-2) if dtype == BF16 else (1e-5,) * 6


def _compare(label, got, ref, bars, names=NAMES):
    """Every element finite (the NaN pre-fill overwritten) and each tensor within its bar."""
    bad = []
    for name, g, r, bar in zip(names, got, ref, bars):
        assert g.shape == r.shape, (name, g.shape, r.shape)
        assert torch.isfinite(g).all(), f"{label} {name}: elements not written"
        e = nrmse(r.numpy(), g.double().numpy())
        print(f"{label} {name}: NRMSE {e:.3g} (bar {bar:.3g})")
        if not e < bar:
            bad.append((name, e, bar))
    assert not bad, (label, bad)


def _run_and_compare(p, label, h3_floor=False):
    ref = _reference(p)
    L = _Launch(p)
    L.fwd()
    L.bwd()
    got = L.results()
    bars = _bars(p.dtype)
    if h3_floor:                                  # the rule of test_window_attention_h3_floor
        f32 = _torch_f32(p)
        e32 = [nrmse(r.numpy(), f.double().numpy()) for r, f in zip(ref, f32)]
        print(f"{label} torch fp32 vs float64: " + ", ".join(f"{n} {e:.3g}" for n, e in zip(NAMES, e32)))
        bars = tuple(max(1e-6, 4 * e) for e in e32)
    _compare(label, got, ref, bars)
    return got, ref


# ============================================================================ 1. head dims, head counts
_HEADS_HD = [(1, 4), (3, 16), (5, 24), (2, 32), (8, 12)]
_HD_CASES = [pytest.param(dt, hh, N, m, id=f"{tag}-h{hh[0]}x{hh[1]}-N{N}-{m}")
             for dt, tag, lst in ((F32, "f32", _HEADS_HD), (BF16, "bf16", _HEADS_HD + [(3, 28)]))
             for hh in lst for N in (64, 100) for m in MODES]
_HD_CASES.append(pytest.param(F32, (3, 16), 200, "labels", id="f32-N200"))


@pytest.mark.parametrize("dtype,heads_hd,N,mode", _HD_CASES)
def test_attn_head_dims(dtype, heads_hd, N, mode):
    """Every head dim the entry points accept besides 20, head counts 1 .. 8, window (7, 8, 8) at
    N = 64 (two full blocks) and 100 (ragged): fp32 runs attn_fwd_kernel<float> /
    attn_bwd_kernel<float>, bf16 the v2 forward and the kv / q backward with partly filled
    4-element runs.  f32-N200: the generic backward's two key groups of 160 keys (dQ summed
    across workgroups with atomics into the buffer the entry point zeroes).  out, lse, dQ, dK,
    dV and dtable vs float64: fp32 NRMSE < 1e-5; bf16 1e-2 forward (lse 1e-5), 2e-2 backward."""
    heads, hd = heads_hd
    p = _problem(300 + 7 * hd + heads + N, dtype, 3, N, heads, hd, W788, mode)
    _run_and_compare(p, f"head dims {dtype} {heads}x{hd} N={N} {mode}")


# ============================================================================ 2. wide-span tiles
# family -> dtype, heads, head dim
FAMILY = {"generic": (F32, 3, 16), "bf16": (BF16, 3, 20), "h3": (F32, 3, 20), "f32mfma": (F32, 2, 20)}
_SMALL_GEO = [((2, 7, 7), 98), ((4, 4, 4), 64), ((2, 6, 6), 72), (W788, 100)]
_SPAN_CASES = [pytest.param(f, w0, N, m, id=f"{f}-{'x'.join(map(str, w0))}-N{N}-{m}")
               for f in ("generic", "bf16", "h3") for (w0, N) in _SMALL_GEO for m in MODES]
_SPAN_CASES += [pytest.param("f32mfma", W889, 544, m, id=f"f32mfma-8x8x9-N544-{m}") for m in MODES]


@pytest.mark.parametrize("family,window,N,mode", _SPAN_CASES)
def test_attn_table_gradient_wide_span(family, window, N, mode):
    """The table gradient where a 32 x 32 tile's relative-position indices span more than the
    per-wave bins (128; 112 in the h3 kernel) and the kernels fall back to LDS atomics on the
    workgroup's column -- every window narrower or wider than 8 does that; (7, 8, 8) is the
    control.  Tile counts per geometry: GEOMETRY, asserted here and in test_attn_geometry_mirror.
    The f32-MFMA backward is reached by the LDS limit (window0 (8, 8, 9), N = 544: 168 of its
    289 tiles span more than 128).  dtable, and out, lse, dQ, dK, dV, vs float64 at the bars
    of test_attn_head_dims; h3: max(1e-6, 4 x torch fp32), both printed."""
    nrel, tiles, wide, mid = _span_counts(window, N)
    assert (nrel, tiles, wide, mid) == GEOMETRY[(tuple(window), N)]
    if tuple(window) != W788:
        assert wide > 0, "no tile on the fallback branch"
    dtype, heads, hd = FAMILY[family]
    lds = _lds_bytes(window, N)
    if family == "h3":
        assert lds.fwd_h3 <= LDS_LIMIT and lds.bwd_h3 <= LDS_LIMIT
    if family == "f32mfma":
        assert lds.bwd_h3 > LDS_LIMIT >= lds.bwd_f32
    nwin = 2 if family == "f32mfma" else 3
    p = _problem(500 + N + hd, dtype, nwin, N, heads, hd, window, mode)
    _run_and_compare(p, f"wide span {family} {window} N={N} {mode}", h3_floor=family == "h3")


# ============================================================================ 3. the LDS limit
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", [544, 530])
def test_attn_f32_mfma_by_lds_limit(N, mode):
    """Head dim 20, window0 (8, 8, 9) (nrel 3825), Np = 544: the h3 forward's image is 175 348 B
    and the h3 dK / dV kernel's 193 660 B (with its static bins), both over the 163 840 B limit,
    so the call runs attn_fwd_f32_kernel<20, MM, RAGGED, 1> (135 116 B) and the f32-MFMA backward
    (157 776 B): N = 544 the non-ragged, N = 530 the ragged instantiation, each mask mode.
    Forward and backward vs float64, NRMSE < 1e-5."""
    b = _lds_bytes(W889, N)
    assert b.fwd_h3 > LDS_LIMIT >= b.fwd_f32 and b.bwd_h3 > LDS_LIMIT >= b.bwd_f32
    p = _problem(700 + N, F32, 2, N, 2, 20, W889, mode)
    _run_and_compare(p, f"f32-MFMA by LDS limit N={N} {mode}")


def _all_nan(t):
    return bool(torch.isnan(t).all())


def test_attn_refuses_oversize():
    """N = 576 with window0 (8, 8, 9): the forward still runs (f32-MFMA, 141 264 B), the f32-MFMA
    backward would need 163 932 B > 163 840 and the call returns DLCS_ERR_UNSUPPORTED_SIZE
    without touching dqkv or dtable."""
    b = _lds_bytes(W889, 576)
    assert b.fwd_f32 <= LDS_LIMIT < b.bwd_f32 and b.bwd_h3 > LDS_LIMIT
    p = _problem(760, F32, 2, 576, 2, 20, W889, "labels")
    ref = _reference(p)
    fill = _rnd((p.nrel, p.heads), 761)
    L = _Launch(p, dtable0=fill)
    L.fwd()
    with pytest.raises(_err(), match=UNSUPPORTED):
        L.bwd()
    out, lse, dq, dk, dv, dt = L.results()
    _compare("oversize forward", (out, lse), ref[:2], (1e-5, 1e-5), NAMES[:2])
    assert _all_nan(dq) and _all_nan(dk) and _all_nan(dv), "a refused backward wrote dqkv"
    assert torch.equal(dt, fill), "a refused backward wrote dtable"


# ============================================================================ 4. writes, refusals
# family -> window0, N, nwin (ragged)
_RAGGED = {"generic": (W788, 100, 3), "bf16": (W788, 100, 3), "h3": (W788, 100, 3), "f32mfma": (W889, 530, 2)}


@pytest.mark.parametrize("family", list(FAMILY))
def test_attn_write_contract(family):
    """include/dlcs.h: dqkv "every element written (no zeroing needed)", dtable "accumulated".
    One ragged case per kernel family into NaN-filled, guarded out / lse / dqkv: every element
    finite and correct, margins intact; the backward called twice into one dtable that starts
    as a random tensor: (dtable - start) / 2 is the float64 gradient at the family's bar."""
    dtype, heads, hd = FAMILY[family]
    window, N, nwin = _RAGGED[family]
    p = _problem(800 + hd + N, dtype, nwin, N, heads, hd, window, "labels")
    ref = _reference(p)
    start = _rnd((p.nrel, heads), 801) * 0.5
    L = _Launch(p, dtable0=start)
    L.fwd()
    L.bwd()
    first = L.dqkv.get()
    L.dqkv.t.fill_(NAN)
    L.bwd()
    got = L.results()
    assert torch.isfinite(first).all(), "dqkv elements not written by the first call"
    grad = (got[5].double() - start.double()) / 2
    _compare(f"write contract {family}", got[:5] + (grad,), ref, _bars(dtype))


_REFUSALS = {
    # name: heads, hd, N, element offset of qkv
    "head_dim_36": (2, 36, 64, 0),
    "head_dim_6": (2, 6, 64, 0),
    "N_1025": (1, 4, 1025, 0),
    "qkv_misaligned": (2, 16, 64, 1),
}


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", list(_REFUSALS))
def test_attn_refusals(case, dtype):
    """head_dim > 32, head_dim % 4 != 0, N > 1024 and a qkv pointer that is not 16-byte aligned:
    forward and backward return DLCS_ERR_UNSUPPORTED_SIZE and write nothing."""
    heads, hd, N, off = _REFUSALS[case]
    p = _problem(900, dtype, 1, N, heads, hd, W788 if N <= 448 else (8, 12, 12), "plain")
    fill = _rnd((p.nrel, heads), 901)
    L = _Launch(p, dtable0=fill)
    qkv = L.qkv
    if off:
        buf = torch.zeros(qkv.numel() + 8, dtype=dtype, device=DEV)
        qkv = buf[off:off + qkv.numel()].view(qkv.shape).copy_(qkv)
        assert qkv.data_ptr() % 16 != 0
    with pytest.raises(_err(), match=UNSUPPORTED):
        L.fwd(qkv)
    with pytest.raises(_err(), match=UNSUPPORTED):
        L.bwd(qkv)
    out, lse, dq, dk, dv, dt = L.results()
    for name, t in zip(NAMES[:5], (out, lse, dq, dk, dv)):
        assert _all_nan(t), f"a refused call wrote {name}"
    assert torch.equal(dt, fill), "a refused call wrote dtable"


# ============================================================================ 5. window isolation
_ISO = {"bf16": (BF16, 3, 12), "generic": (F32, 3, 16), "h3": (F32, 3, 20)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", list(_ISO))
def test_attn_window_isolation(family, mode):
    """Three ragged windows (N = 100) in one call, then each window alone (nwin = 1, contiguous
    copy of its rows, its own labels / mask slice): out, lse, dK, dV and dQ of the joint run are
    bit-identical to the single runs -- a workgroup's arithmetic does not depend on its
    neighbours, so a key or query past N read from the next window shows here, where no NRMSE
    bar in bf16 would see it.  The generic fp32 backward sums dQ with atomics: NRMSE < 1e-6."""
    dtype, heads, hd = _ISO[family]
    p = _problem(1000 + hd, dtype, 3, 100, heads, hd, W788, mode)
    J = _Launch(p)
    J.fwd()
    J.bwd()
    joint = J.results()
    for n, t in zip(NAMES[:5], joint[:5]):
        assert torch.isfinite(t).all(), n
    for w in range(p.nwin):
        S = _Launch(_window_of(p, w))
        S.fwd()
        S.bwd()
        solo = S.results()
        r = slice(w * p.N, (w + 1) * p.N)
        parts = (joint[0][r], joint[1][w:w + 1], joint[2][r], joint[3][r], joint[4][r])
        for name, a, b in zip(NAMES[:5], parts, solo[:5]):
            assert torch.isfinite(b).all(), (name, w)
            if name == "dq" and family == "generic":
                e = nrmse(b.double().numpy(), a.double().numpy())
                assert e < 1e-6, (name, w, e)
            else:
                assert torch.equal(a, b), f"{family} {mode} window {w}: {name} differs from the window run alone"


# ============================================================================ 6. a block off 160 / 8 / (7, 8, 8)
def test_swin_block_other_geometry():
    """SwinTransformerBlock3D(64, 4, window (2, 7, 7), shift (1, 3, 3)) on a (4, 14, 14) token
    grid, fp32, forward and backward against the float64 block of oracle/dlcs_oracle.py on the
    same weights: the labels of window_tables, the [:N, :N] slicing of the bias index and the
    generic fp32 attention kernels (head dim 16) together in a real shifted geometry.  Bars of
    test_gpu_swin.py::test_swin_block_module: 1e-5 on y and dx, 1e-4 on parameter gradients."""
    from dl_cs.models import swin3D
    from dl_cs.models import video_swin_transformer_mri_downsample as vst
    from oracle import dlcs_oracle as O
    from oracle import recipe, windex
    dim, heads, window, shift, grid = 64, 4, (2, 7, 7), (1, 3, 3), (4, 14, 14)
    old = swin3D.get_compute_dtype()
    swin3D.set_compute_dtype(F32)
    try:
        blk = vst.SwinTransformerBlock3D(dim, heads, window_size=window, shift_size=shift, qkv_bias=True)
        blk.eval()
        recipe.fill_module(blk, 41)
        blk = blk.to(DEV)
        ws, ss = windex.get_window_size(grid, window, shift)
        assert (ws, ss) == (window, shift)
        m = vst.compute_mask(*windex.padded_grid(*grid, ws), ws, ss, DEV)
        x0, dy = recipe.randn(42, (1,) + grid + (dim,)), recipe.randn(43, (1,) + grid + (dim,))
        x = x0.to(DEV).requires_grad_()
        y = blk(x, m)
        (y * dy.to(DEV)).sum().backward()
    finally:
        swin3D.set_compute_dtype(old)
    P = {k: v.detach().cpu().double().requires_grad_() for k, v in blk.named_parameters()}
    m64 = torch.from_numpy(windex.compute_mask(*windex.padded_grid(*grid, ws), ws, ss)).double()
    assert torch.equal(m.cpu().double(), m64)
    x64 = x0.double().requires_grad_()
    y64 = O.swin_block(P, "", x64, shift, m64, heads, window)
    (y64 * dy.double()).sum().backward()
    assert nrmse(y64.detach().numpy(), y.detach().double().cpu().numpy()) < 1e-5
    assert nrmse(x64.grad.numpy(), x.grad.double().cpu().numpy()) < 1e-5
    named = dict(blk.named_parameters())
    assert set(named) == set(P) and len(P) == 13
    for n, v in P.items():
        e = nrmse(v.grad.numpy(), named[n].grad.double().cpu().numpy())
        print(f"block (2,7,7) grad {n}: NRMSE {e:.3g}")
        assert e < 1e-4, (n, e)
