// Live-frame windows of the weight gradients: which work units a window [t_lo, t_hi) of
// non-zero g frames leaves, how they are numbered and how ranges are cut over them.  Plain
// C++ that also compiles for the device, so tools/wgrad_live_check.cpp walks the same code on
// the host.
//
// The 160 -> 160 kernel's unit is a half patch (2 frames x 4 x 4 voxels); units are walked
// patch-major, ((b nT + t_blk) nY + py) nX + px, half th = 0, 1.  Half-slab hs = 2 t_blk + th
// holds frames [2 hs, 2 hs + 2); the live ones of every batch item are [hs_lo, hs_hi) =
// [t_lo / 2, ceil(t_hi / 2)).  Per live slab either both halves are live, or only the second
// (the first live slab, hs_lo odd), or only the first (the last live slab, hs_hi odd).
#pragma once

#if defined(__HIPCC__)
#define WGL_HD __host__ __device__ __forceinline__
#else
#define WGL_HD inline
#endif

struct WgLiveGeom { int nT, nY, nX, hs_lo, hs_hi; };     // 0 <= hs_lo < hs_hi <= 2 nT
struct WgLiveIter { int ip, ipt, ipy, ipx, th; };        // flat patch index, its slab / y / x, the half

// the window of frames as half-slabs; empty -> hs_lo >= hs_hi
WGL_HD void wgl_halfslabs(int D, int t_lo, int t_hi, int* hs_lo, int* hs_hi) {
    if (t_lo < 0) t_lo = 0;
    if (t_hi > D) t_hi = D;
    *hs_lo = t_lo >> 1;
    *hs_hi = t_lo < t_hi ? (t_hi + 1) >> 1 : *hs_lo;
}

// Whole 4-frame slabs [s0, s1) of every batch item whose frames, widened by `halo` frames per
// side, meet the window (the thin weight gradient gathers g through a one-frame tap halo, so a
// patch is dead only if its halo is); empty -> s0 >= s1
WGL_HD void wgl_slabs(int D, int t_lo, int t_hi, int halo, int* s0, int* s1) {
    if (t_lo < 0) t_lo = 0;
    if (t_hi > D) t_hi = D;
    const int lo = t_lo - halo;
    *s0 = (lo > 0 ? lo : 0) >> 2;
    const int hi = (t_hi + halo + 3) >> 2;
    *s1 = t_lo < t_hi ? (hi < (D >> 2) ? hi : (D >> 2)) : *s0;
}

// live patch number u -> flat patch index; per = live patches of a batch item, item = all its
// patches, first = patches of its dead slabs below the window
WGL_HD int wgl_live_patch(int u, int per, int item, int first) {
    const int bi = u / per;
    return bi * item + first + (u - bi * per);
}

WGL_HD int wgl_units_per_item(const WgLiveGeom& g) { return (g.hs_hi - g.hs_lo) * g.nY * g.nX; }

// range r of nr over n units [u0, u1): sizes differ by at most one, the first n % nr one larger
// (the launch passes base = n / nr and rem = n % nr, the kernels cut with them)
WGL_HD void wgl_range(int base, int rem, int r, int* u0, int* u1) {
    *u0 = r * base + (r < rem ? r : rem);
    *u1 = *u0 + base + (r < rem ? 1 : 0);
}

// live unit number u (< B units_per_item) -> its patch and half
WGL_HD WgLiveIter wgl_seek(const WgLiveGeom& g, int u) {
    const int nYX = g.nY * g.nX, per = (g.hs_hi - g.hs_lo) * nYX;
    const int bi = u / per;
    int r = u - bi * per;
    const int t0 = g.hs_lo >> 1;
    const int nfirst = ((2 * t0 + 2 < g.hs_hi ? 2 * t0 + 2 : g.hs_hi) - g.hs_lo) * nYX;    // units of slab t0
    int t, pin, th;
    if (r < nfirst) {
        t = t0;
        if (nfirst == 2 * nYX) { pin = r >> 1; th = r & 1; }
        else { pin = r; th = g.hs_lo & 1; }
    } else {
        r -= nfirst;
        t = t0 + 1 + r / (2 * nYX);
        r -= (t - t0 - 1) * 2 * nYX;
        if (2 * t + 1 < g.hs_hi) { pin = r >> 1; th = r & 1; }
        else { pin = r; th = 0; }                   // the last slab's first half alone
    }
    WgLiveIter it;
    it.ip = (bi * g.nT + t) * nYX + pin;
    it.ipt = t;
    it.ipy = pin / g.nX;
    it.ipx = pin - it.ipy * g.nX;
    it.th = th;
    return it;
}

// the next live unit: the patch's second half if live, else the first live half of the next
// patch, skipping the dead slabs at the end of this batch item and the start of the next
WGL_HD void wgl_advance(const WgLiveGeom& g, WgLiveIter& it) {
    if (it.th == 0 && 2 * it.ipt + 1 < g.hs_hi) { it.th = 1; return; }
    ++it.ip;
    if (++it.ipx == g.nX) {
        it.ipx = 0;
        if (++it.ipy == g.nY) {
            it.ipy = 0;
            if (2 * ++it.ipt >= g.hs_hi) {
                const int t0 = g.hs_lo >> 1;
                it.ip += (g.nT - it.ipt + t0) * g.nY * g.nX;
                it.ipt = t0;
            }
        }
    }
    it.th = 2 * it.ipt >= g.hs_lo ? 0 : 1;
}
