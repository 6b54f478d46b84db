// Stand-alone host check of the plane conv's index arithmetic (csrc/conv2d_geom.h and the
// loops of csrc/conv2d.hip restated on the host): walks every tile of the forward kernel and
// every pixel range of the weight gradient over a grid of geometries, touching byte maps sized
// like the real buffers with bounds-checked accesses, and checks that every pixel is staged
// and written exactly once.  Meant to be built with -fsanitize=address,undefined
// (tests/test_conv2d_geom.py); no GPU, nothing loaded into Python.
//   c++ -std=c++17 -fsanitize=address,undefined -I dl-swin-gan_amd/csrc tools/conv2d_geom_check.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "conv2d_geom.h"

int main() {
    long checked = 0;
    for (int KH : {3, 1})
    for (long N : {1L, 2L, 5L, 77L})
    for (long H = 1; H <= (KH == 3 ? 17 : 6); ++H)
    for (long W = 1; W <= (KH == 3 ? 17 : 258); W += (KH == 3 ? 1 : 7)) {
        Conv2dGeom g;
        int st = conv2d_geom(N, H, W, KH, &g);
        bool big = KH == 3 ? (H > 16 || W > 16) : W > 256;
        if (big != (st == DLCS_ERR_UNSUPPORTED_SIZE)) { printf("limit mismatch\n"); return 1; }
        if (st) continue;
        if (g.PP < 1 || g.PP * g.PH * g.PW > C2_MTILE || g.PP * g.HR * g.HC > C2_HALO) { printf("tile too big\n"); return 1; }
        std::vector<char> in(g.rows, 0), out(g.rows, 0), lds(C2_HALO);
        const int ppix = g.PH * g.PW, hpl = g.HR * g.HC;
        for (long t = 0; t < g.ntiles; ++t) {
            long plane0 = t * g.PP, left = g.nplanes - plane0;
            int np = left < g.PP ? (int)left : g.PP;
            long row0 = plane0 * ppix;
            for (int hr = 0; hr < np * hpl; ++hr) {
                int pl = hr / hpl, rem = hr - pl * hpl, hy = rem / g.HC, hx = rem - hy * g.HC;
                int y = KH == 3 ? hy - 1 : 0, x = hx - 1;
                lds.at(hr) = 1;
                if (y >= 0 && y < g.PH && x >= 0 && x < g.PW) in.at(row0 + (long)pl * ppix + y * g.PW + x) = 1;
            }
            for (int m = 0; m < C2_MTILE; ++m) {
                int mm = m < np * ppix ? m : 0;
                int pl = mm / ppix, rem = mm - pl * ppix, y = rem / g.PW, x = rem - y * g.PW;
                int hb = pl * hpl + y * g.HC + x;
                for (int tap = 0; tap < KH * 3; ++tap) (void)lds.at(hb + (tap / 3) * g.HC + tap % 3);
                if (m < np * ppix) out.at(row0 + m) += 1;
            }
        }
        for (long r = 0; r < g.rows; ++r) if (in[r] != 1 || out[r] != 1) { printf("coverage\n"); return 1; }
        for (long ppb : {0L, 1L, 64L, 100L, 128L, 4096L}) {
            long ppr = conv2d_wgrad_ppr(ppb), nr = conv2d_wgrad_ranges(g.rows, ppr);
            std::vector<char> seen(g.rows, 0);
            for (long rg = 0; rg < nr; ++rg) {
                long p0 = rg * ppr, p1 = p0 + ppr < g.rows ? p0 + ppr : g.rows;
                for (long pb = p0; pb < p1; pb += C2_WG_PIX) for (int vl = 0; vl < C2_WG_PIX; ++vl) {
                    long p = pb + vl; if (p >= p1) continue;
                    seen.at(p) += 1;
                    for (int tap = 0; tap < KH * 3; ++tap) {
                        int dy = KH == 3 ? tap / 3 - 1 : 0, dx = tap % 3 - 1;
                        int rem = (int)(p % ppix), y = rem / g.PW + dy, x = rem % g.PW + dx;
                        if (y >= 0 && y < g.PH && x >= 0 && x < g.PW) (void)in.at(p + dy * g.PW + dx);
                    }
                }
            }
            for (long r = 0; r < g.rows; ++r) if (seen[r] != 1) { printf("range coverage\n"); return 1; }
            if (conv2d_wgrad_ws(nr, KH, 256, 256) < (size_t)nr * KH * 3 * 256 * 256 * 4) { printf("ws\n"); return 1; }
        }
        ++checked;
    }
    Conv2dGeom g;
    if (conv2d_geom((int64_t)1 << 40, 16, 16, 3, &g) != DLCS_ERR_UNSUPPORTED_SIZE) return 1;
    if (conv2d_geom(INT64_MAX, INT64_MAX, 4, 1, &g) != DLCS_ERR_UNSUPPORTED_SIZE) return 1;
    if (conv2d_geom(0, 4, 4, 3, &g) != DLCS_ERR_INVALID_ARG || conv2d_geom(1, 4, 4, 2, &g) != DLCS_ERR_INVALID_ARG) return 1;
    printf("ok: %ld geometries\n", checked);
    return 0;
}
