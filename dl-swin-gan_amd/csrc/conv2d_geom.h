// Host-side index arithmetic of the plane conv (conv2d.hip): tile geometry, limits and the
// weight gradient's ranges and workspace size.  Plain C++ (no HIP), so it also compiles into a
// stand-alone host program.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/dlcs.h"

constexpr int C2_MTILE = 256;      // pixels of a workgroup's M tile (4 waves x 2 x 32)
constexpr int C2_PLANES = 16;      // planes of a tile at most
constexpr int C2_HALO = 640;       // halo rows of a tile in LDS at most
constexpr int C2_MAX_HW = 16;      // KH = 3: H, W <= 16 (a plane is one tile at most)
constexpr int C2_MAX_W1 = 256;     // KH = 1: W <= 256 (a sequence is one tile at most)
constexpr int C2_MAX_CH = 256;     // cin, cout
constexpr int C2_WG_PIX = 64;      // pixels of one k-stage of the weight gradient
constexpr int C2_WG_CO = 128;      // cout_pad columns of one weight-gradient workgroup

struct Conv2dGeom {
    long nplanes;   // independent planes: N (KH = 3) or N * H sequences (KH = 1)
    long rows;      // N * H * W
    int PH, PW;     // a plane: H x W, or 1 x W
    int HR, HC;     // its zero-filled halo: (PH + 2) x (PW + 2), or 1 x (PW + 2)
    int PP;         // planes per tile
    long ntiles;
};

static inline int conv2d_geom(int64_t N, int64_t H, int64_t W, int KH, Conv2dGeom* g) {
    if (KH != 3 && KH != 1) return DLCS_ERR_INVALID_ARG;
    if (N < 1 || H < 1 || W < 1) return DLCS_ERR_INVALID_ARG;
    if (KH == 3 && (H > C2_MAX_HW || W > C2_MAX_HW)) return DLCS_ERR_UNSUPPORTED_SIZE;
    if (KH == 1 && W > C2_MAX_W1) return DLCS_ERR_UNSUPPORTED_SIZE;
    const int64_t lim = (int64_t)1 << 31;
    if (N >= lim || H >= lim) return DLCS_ERR_UNSUPPORTED_SIZE;
    if (N * H >= lim || N * H * W >= lim) return DLCS_ERR_UNSUPPORTED_SIZE;     // < 2^62: no overflow
    g->nplanes = KH == 3 ? (long)N : (long)(N * H);
    g->rows = (long)(N * H * W);
    g->PH = KH == 3 ? (int)H : 1;
    g->PW = (int)W;
    g->HR = KH == 3 ? g->PH + 2 : 1;
    g->HC = g->PW + 2;
    int pp = C2_MTILE / (g->PH * g->PW);
    if (pp > C2_PLANES) pp = C2_PLANES;
    while (pp > 1 && pp * g->HR * g->HC > C2_HALO) --pp;      // one plane: <= 18 x 18 or 258 rows
    g->PP = pp;
    g->ntiles = (g->nplanes + pp - 1) / pp;
    return 0;
}

static inline bool conv2d_channels_ok(int64_t c, int64_t c_pad) {
    return c >= 1 && c <= C2_MAX_CH && c_pad >= c && c_pad % 32 == 0 && c_pad <= C2_MAX_CH;
}

// pixel range of a weight-gradient workgroup (a multiple of the k-stage) and their number
static inline long conv2d_wgrad_ppr(int64_t pix_per_block) {
    long p = pix_per_block <= 0 ? 4096 : (long)pix_per_block;
    if (p > ((long)1 << 30)) p = (long)1 << 30;
    return (p + C2_WG_PIX - 1) / C2_WG_PIX * C2_WG_PIX;
}
static inline long conv2d_wgrad_ranges(long rows, long ppr) { return (rows + ppr - 1) / ppr; }
// workspace: one dW slab [KH 3][cout_pad][cin_pad] per range, then one row of column sums per range
static inline size_t conv2d_wgrad_slab_floats(long nrange, int KH, int64_t cout_pad, int64_t cin_pad) {
    return (size_t)nrange * (size_t)(KH * 3) * (size_t)cout_pad * (size_t)cin_pad;
}
static inline size_t conv2d_wgrad_ws(long nrange, int KH, int64_t cout_pad, int64_t cin_pad) {
    return (conv2d_wgrad_slab_floats(nrange, KH, cout_pad, cin_pad) + (size_t)nrange * (size_t)cout_pad) * sizeof(float);
}
