// Host walk of the weight gradients' live-frame mapping (csrc/wgrad_live.h), as the kernels use
// it: per range seek to its first live unit, then advance unit by unit.  For a sweep of
// (B, nT, nY, nX, t_lo, t_hi, ranges) the walk must give exactly the live half patches, each
// once and in patch-major order, with consistent (t, y, x) coordinates, no dead half, and
// range sizes that differ by at most one unit; the whole-patch walk of the thin weight gradient
// likewise.  Prints "ok: <n> cases"; tests/test_wgrad_live_map.py builds and runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "wgrad_live.h"

static long g_cases = 0;

#define CHECK(c)                                                                                         \
    do {                                                                                                 \
        if (!(c)) {                                                                                      \
            std::printf("FAIL %s:%d %s (B %d nT %d nY %d nX %d window [%d, %d) nr %d)\n", __FILE__, __LINE__, \
                        #c, B, nT, nY, nX, t_lo, t_hi, nr);                                             \
            std::exit(1);                                                                                \
        }                                                                                                \
    } while (0)

struct Unit { int ip, th; };

static void half_units(int B, int nT, int nY, int nX, int t_lo, int t_hi, int want) {
    int nr = want;
    const int D = 4 * nT;
    int hs_lo, hs_hi;
    wgl_halfslabs(D, t_lo, t_hi, &hs_lo, &hs_hi);
    // the definition: a half is live iff its two frames intersect the window
    std::vector<Unit> ref;
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < nT; ++t)
            for (int p = 0; p < nY * nX; ++p)
                for (int th = 0; th < 2; ++th) {
                    const int f0 = 4 * t + 2 * th;
                    if (std::max(f0, t_lo) < std::min(f0 + 2, std::min(t_hi, D)))
                        ref.push_back({(b * nT + t) * nY * nX + p, th});
                }
    if (ref.empty()) {
        CHECK(hs_lo >= hs_hi);
        return;
    }
    CHECK(hs_lo < hs_hi && hs_lo >= 0 && hs_hi <= 2 * nT);
    const WgLiveGeom g{nT, nY, nX, hs_lo, hs_hi};
    const int n = B * wgl_units_per_item(g);
    CHECK(n == (int)ref.size());
    nr = std::min(want, n);
    int next = 0, smin = n, smax = 0;
    for (int r = 0; r < nr; ++r) {
        int u0, u1;
        wgl_range(n / nr, n % nr, r, &u0, &u1);
        CHECK(u0 == next && u1 > u0 && u1 <= n);
        next = u1;
        smin = std::min(smin, u1 - u0);
        smax = std::max(smax, u1 - u0);
        WgLiveIter it = wgl_seek(g, u0);
        for (int u = u0; u < u1; ++u) {
            CHECK(it.ip == ref.at(u).ip && it.th == ref.at(u).th);
            const int rr = it.ip % (nT * nY * nX);
            CHECK(it.ipt == rr / (nY * nX) && it.ipy == rr / nX % nY && it.ipx == rr % nX);
            wgl_advance(g, it);
        }
    }
    CHECK(next == n && smax - smin <= 1);
    ++g_cases;
}

static void whole_patches(int B, int nT, int nY, int nX, int t_lo, int t_hi, int halo, int want) {
    int nr = want;
    const int D = 4 * nT;
    int s0, s1;
    wgl_slabs(D, t_lo, t_hi, halo, &s0, &s1);
    // the definition: a patch is live iff its frames, widened by the halo, meet the window
    std::vector<int> ref;
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < nT; ++t)
            for (int p = 0; p < nY * nX; ++p)
                if (std::max(4 * t - halo, std::max(t_lo, 0)) < std::min(4 * t + 4 + halo, std::min(t_hi, D)))
                    ref.push_back((b * nT + t) * nY * nX + p);
    if (ref.empty()) {
        CHECK(s0 >= s1);
        return;
    }
    CHECK(s0 < s1 && s0 >= 0 && s1 <= nT);
    const int per = (s1 - s0) * nY * nX, n = B * per;
    CHECK(n == (int)ref.size());
    nr = std::min(want, n);
    int next = 0;
    for (int r = 0; r < nr; ++r) {
        int u0, u1;
        wgl_range(n / nr, n % nr, r, &u0, &u1);
        CHECK(u0 == next && u1 > u0);
        next = u1;
        for (int u = u0; u < u1; ++u) CHECK(wgl_live_patch(u, per, nT * nY * nX, s0 * nY * nX) == ref.at(u));
    }
    CHECK(next == n);
    ++g_cases;
}

int main() {
    const int grids[][2] = {{1, 1}, {2, 2}, {2, 3}, {3, 5}};
    const int wants[] = {1, 2, 3, 5, 8, 9, 12, 28};
    for (int B = 1; B <= 3; ++B)
        for (int nT = 1; nT <= 7; ++nT)
            for (const auto& yx : grids)
                for (int t_lo = -1; t_lo <= 4 * nT; ++t_lo)
                    for (int t_hi = t_lo; t_hi <= 4 * nT + 1; ++t_hi)
                        for (int want : wants) {
                            half_units(B, nT, yx[0], yx[1], t_lo, t_hi, want);
                            whole_patches(B, nT, yx[0], yx[1], t_lo, t_hi, 0, want);
                            whole_patches(B, nT, yx[0], yx[1], t_lo, t_hi, 1, want);
                        }
    std::printf("ok: %ld cases\n", g_cases);
    return 0;
}
