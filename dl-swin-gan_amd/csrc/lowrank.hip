// Locally low-rank block operators of the DSLR family (reference dl_cs/mri/lowrank.py
// ArrayToBlocks :13-187 and Decompose.compose :247-253), complex64 data with an fp32
// window and fp32 weights.  One image [E, T, Y, X] (batch 1) is zero-padded to
// [Yp, Xp] = b (Y / b + 1), b (X / b + 1) with floor((Yp - Y) / 2) rows on the left (the
// extra row of an odd size goes right, lowrank:62-77) and cut into nby x nbx blocks of
// b x b at stride s = b / 2, block n = by nbx + bx, block matrix row p = e b^2 + iy b + ix,
// every element times the periodic sqrt-Hann window win[iy] win[ix]:
//
// * dlcs_lr_extract     blocks[n, p, t] = win (image / (weights + 1e-8) if divide)
// * dlcs_lr_combine     image = crop(sum over the <= 4 covering blocks of win blocks),
//                       / (weights + 1e-8) if divide: lowrank's combine; divide 0 is the
//                       exact adjoint of extract, divide 1 the adjoint of extract(divide 1)
// * dlcs_lr_compose     combine(L R^H) without the block tensor
// * dlcs_lr_project_l   extract(image) R    -> [N, E b^2, r]
// * dlcs_lr_project_r   extract(image)^H L  -> [N, T, r]
//
// Image -> block side (extract, project_l, project_r): a workgroup stages kRows rows of
// one block's matrix (all T frames) in LDS, reading the image in x-runs of b elements
// (8-B accesses: the pads shift every run by an arbitrary pixel count, so 16 B cannot be
// guaranteed there), and writes or contracts it from LDS.  The 4 blocks that cover a
// pixel are neighbours in the grid, so the three re-reads come from L2.
// Block -> image side (combine, compose): a workgroup owns kPix pixels that share their
// covering blocks (a run of s x s quadrants along x), gathers the four contributions of
// each pixel in the fixed order (by-1, bx-1), (by-1, bx), (by, bx-1), (by, bx), and writes
// x-runs.  No float atomics anywhere: the same input gives the same bits.
// R (and in compose the L rows) are staged in LDS with 16-B global reads when r is even
// and the pointer is 16-B aligned; the block-side stores of extract / project_* and the
// block reads of combine are 16 B under the same condition on T / r.
#include <type_traits>

#include "dlcs_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxT = 32, kMaxR = 8, kMaxE = 2;
constexpr int kRows = 64;                  // block-matrix rows per pass (image -> block side)
constexpr int kPix = 64;                   // pixels per workgroup (block -> image side)
constexpr int kMaxQ = 4;                   // quadrants along x per workgroup
constexpr int kTS = kMaxT + 1;             // LDS tile stride in complex elements
constexpr int kLS = kMaxR + 1;             // LDS L-row stride in complex elements

struct LrGeo {
    int E, T, Y, X, b, s;
    int py0, px0;                          // left pads
    int nby, nbx;
    int qw;                                // quadrants along x per workgroup: min(kMaxQ, kPix / s^2)
};

// acc += a b
DLCS_DEV void cfma(float2& acc, float2 a, float2 b) {
    acc.x = fmaf(a.x, b.x, acc.x); acc.x = fmaf(-a.y, b.y, acc.x);
    acc.y = fmaf(a.x, b.y, acc.y); acc.y = fmaf(a.y, b.x, acc.y);
}
// acc += a conj(b)
DLCS_DEV void cfma_conj(float2& acc, float2 a, float2 b) {
    acc.x = fmaf(a.x, b.x, acc.x); acc.x = fmaf(a.y, b.y, acc.x);
    acc.y = fmaf(a.y, b.x, acc.y); acc.y = fmaf(-a.x, b.y, acc.y);
}

// n complex elements global -> LDS (both contiguous); 16-B global reads when vec
DLCS_DEV void stage_flat(float2* dst, const float2* src, int n, bool vec) {
    if (vec) {
        for (int i = threadIdx.x; i < (n >> 1); i += kThreads) {
            const float4 v = reinterpret_cast<const float4*>(src)[i];
            dst[2 * i] = make_float2(v.x, v.y);
            dst[2 * i + 1] = make_float2(v.z, v.w);
        }
    } else {
        for (int i = threadIdx.x; i < n; i += kThreads) dst[i] = src[i];
    }
}

// tile[pl kTS + t] = win (image / (weights + 1e-8)) for rows [p0, p0 + rows) of block (by, bx),
// 0 in the pad; consecutive threads walk ix, then iy, then t
DLCS_DEV void load_tile(float2* tile, const float2* img, const float* wgt, const float* swin, const LrGeo& g, int by,
                        int bx, int p0, int rows) {
    const int bb = g.b * g.b;
    for (int i = threadIdx.x; i < rows * g.T; i += kThreads) {
        const int pl = i % rows, t = i / rows;
        const int p = p0 + pl;
        const int e = p / bb, q = p - e * bb;
        const int iy = q / g.b, ix = q - iy * g.b;
        const int y = by * g.s + iy - g.py0, x = bx * g.s + ix - g.px0;
        float2 v = make_float2(0.0f, 0.0f);
        if (y >= 0 && y < g.Y && x >= 0 && x < g.X) {
            v = img[(((long)e * g.T + t) * g.Y + y) * g.X + x];
            float w = swin[iy] * swin[ix];
            if (wgt) w = w / (wgt[(long)y * g.X + x] + 1e-8f);
            v.x *= w; v.y *= w;
        }
        tile[pl * kTS + t] = v;
    }
}

// ------------------------------------------------------------------ extract
__global__ void __launch_bounds__(kThreads) lr_extract_kernel(const float2* img, const float* wgt, const float* win,
                                                              float2* blocks, LrGeo g, int vec) {
    __shared__ float2 tile[kRows * kTS];
    __shared__ float swin[16];
    const int P = g.E * g.b * g.b;
    const int rows = min(kRows, P);
    const int ppb = P / rows;                              // passes per block (P is a multiple of rows)
    const int n = blockIdx.x / ppb, p0 = (blockIdx.x % ppb) * rows;
    if (threadIdx.x < g.b) swin[threadIdx.x] = win[threadIdx.x];
    __syncthreads();
    load_tile(tile, img, wgt, swin, g, n / g.nbx, n % g.nbx, p0, rows);
    __syncthreads();
    float2* dst = blocks + ((long)n * P + p0) * g.T;
    if (vec) {                                             // T even: pairs along t, 16-B stores
        const int h = g.T >> 1;
        for (int i = threadIdx.x; i < rows * h; i += kThreads) {
            const int pl = i / h, t = (i - pl * h) * 2;
            const float2 a = tile[pl * kTS + t], c = tile[pl * kTS + t + 1];
            reinterpret_cast<float4*>(dst)[i] = make_float4(a.x, a.y, c.x, c.y);
        }
    } else {
        for (int i = threadIdx.x; i < rows * g.T; i += kThreads) dst[i] = tile[(i / g.T) * kTS + i % g.T];
    }
}

// ------------------------------------------------------------------ project_l: extract(image) R
__global__ void __launch_bounds__(kThreads) lr_project_l_kernel(const float2* img, const float* wgt, const float* win,
                                                                const float2* R, float2* out, LrGeo g, int r, int vec_r,
                                                                int vec_o) {
    __shared__ float2 tile[kRows * kTS];
    __shared__ float2 sR[kMaxT * kMaxR];
    __shared__ float swin[16];
    const int P = g.E * g.b * g.b;
    const int rows = min(kRows, P);
    const int ppb = P / rows;
    const int n = blockIdx.x / ppb, p0 = (blockIdx.x % ppb) * rows;
    if (threadIdx.x < g.b) swin[threadIdx.x] = win[threadIdx.x];
    stage_flat(sR, R + (long)n * g.T * r, g.T * r, vec_r);
    __syncthreads();
    load_tile(tile, img, wgt, swin, g, n / g.nbx, n % g.nbx, p0, rows);
    __syncthreads();
    float2* dst = out + ((long)n * P + p0) * r;
    if (vec_o) {                                           // r even: two k per thread, 16-B stores
        const int h = r >> 1;
        for (int i = threadIdx.x; i < rows * h; i += kThreads) {
            const int pl = i / h, k = (i - pl * h) * 2;
            float2 a0 = make_float2(0.0f, 0.0f), a1 = a0;
            for (int t = 0; t < g.T; ++t) {
                const float2 x = tile[pl * kTS + t];
                cfma(a0, x, sR[t * r + k]);
                cfma(a1, x, sR[t * r + k + 1]);
            }
            reinterpret_cast<float4*>(dst)[i] = make_float4(a0.x, a0.y, a1.x, a1.y);
        }
    } else {
        for (int i = threadIdx.x; i < rows * r; i += kThreads) {
            const int pl = i / r, k = i - pl * r;
            float2 a = make_float2(0.0f, 0.0f);
            for (int t = 0; t < g.T; ++t) cfma(a, tile[pl * kTS + t], sR[t * r + k]);
            dst[i] = a;
        }
    }
}

// ------------------------------------------------------------------ project_r: extract(image)^H L
// One workgroup per block: thread (grp, t, k) sums conj(x[p, t]) L[p, k] over the rows
// p = grp, grp + G, ... of every pass in ascending order, then the G partials are added in
// ascending grp: a fixed order.
__global__ void __launch_bounds__(kThreads) lr_project_r_kernel(const float2* img, const float* wgt, const float* win,
                                                                const float2* L, float2* out, LrGeo g, int r, int vec_l) {
    __shared__ float2 tile[kRows * kTS];
    __shared__ float2 sL[kRows * kMaxR];
    __shared__ float2 red[kThreads];
    __shared__ float swin[16];
    const int P = g.E * g.b * g.b;
    const int rows = min(kRows, P);
    const int n = blockIdx.x;
    const int TR = g.T * r;                                // <= 256
    const int G = kThreads / TR;
    const int grp = threadIdx.x / TR, tk = threadIdx.x - grp * TR;
    const int t = tk / r, k = tk - t * r;
    if (threadIdx.x < g.b) swin[threadIdx.x] = win[threadIdx.x];
    float2 acc = make_float2(0.0f, 0.0f);
    for (int p0 = 0; p0 < P; p0 += rows) {
        __syncthreads();                                   // swin ready; the previous pass is consumed
        load_tile(tile, img, wgt, swin, g, n / g.nbx, n % g.nbx, p0, rows);
        stage_flat(sL, L + ((long)n * P + p0) * r, rows * r, vec_l);
        __syncthreads();
        if (grp < G)
            for (int pl = grp; pl < rows; pl += G) cfma_conj(acc, sL[pl * r + k], tile[pl * kTS + t]);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < TR) {
        float2 sum = red[threadIdx.x];
        for (int j = 1; j < G; ++j) { const float2 v = red[j * TR + threadIdx.x]; sum.x += v.x; sum.y += v.y; }
        out[(long)n * TR + threadIdx.x] = sum;
    }
}

// ------------------------------------------------------------------ block -> image side
// A workgroup owns quadrant row qy, quadrants [qx0, qx0 + nq) along x and one e: s rows of
// nq s pixels, padded coordinates (qy s + iy', qx0 s + xr).  Pixel (iy', xr), quadrant
// q = xr / s, ix' = xr % s, is covered by c = 2 cy + cx: block (qy - 1 + cy, qx0 + q - 1 + cx)
// at (iy' + (1 - cy) s, ix' + (1 - cx) s).
struct LrCover { int n, p; float w; };                  // block (-1: off the grid), row, window

DLCS_DEV LrCover lr_cover(const LrGeo& g, const float* swin, int e, int qy, int qx0, int iyq, int xr, int c) {
    const int q = xr / g.s, ixq = xr - q * g.s;
    const int cy = c >> 1, cx = c & 1;
    const int by = qy - 1 + cy, bx = qx0 + q - 1 + cx;
    const int iy = iyq + (1 - cy) * g.s, ix = ixq + (1 - cx) * g.s;
    LrCover o;
    o.n = (by >= 0 && by < g.nby && bx >= 0 && bx < g.nbx) ? by * g.nbx + bx : -1;
    o.p = (e * g.b + iy) * g.b + ix;
    o.w = swin[iy] * swin[ix];
    return o;
}

__global__ void __launch_bounds__(kThreads) lr_combine_kernel(const float2* blocks, const float* wgt, const float* win,
                                                              float2* img, LrGeo g, int vec) {
    __shared__ float2 tile[kMaxT * (kPix + 1)];
    __shared__ float swin[16];
    const int nqx = g.nbx + 1;
    const int qx0 = blockIdx.x * g.qw, qy = blockIdx.y, e = blockIdx.z;
    const int nq = min(g.qw, nqx - qx0);
    const int W = nq * g.s, npix = g.s * W;
    const long P = (long)g.E * g.b * g.b;
    if (threadIdx.x < g.b) swin[threadIdx.x] = win[threadIdx.x];
    __syncthreads();
    if (vec) {                                                       // T even: pairs along t, 16-B block reads
        const int h = g.T >> 1;
        for (int i = threadIdx.x; i < npix * h; i += kThreads) {
            const int j = i / h, t = (i - j * h) * 2;
            float2 v0 = make_float2(0.0f, 0.0f), v1 = v0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const LrCover cv = lr_cover(g, swin, e, qy, qx0, j / W, j % W, c);
                if (cv.n >= 0) {
                    const float4 b = *reinterpret_cast<const float4*>(blocks + ((long)cv.n * P + cv.p) * g.T + t);
                    v0.x = fmaf(cv.w, b.x, v0.x); v0.y = fmaf(cv.w, b.y, v0.y);
                    v1.x = fmaf(cv.w, b.z, v1.x); v1.y = fmaf(cv.w, b.w, v1.y);
                }
            }
            tile[t * (kPix + 1) + j] = v0;
            tile[(t + 1) * (kPix + 1) + j] = v1;
        }
    } else {
        for (int i = threadIdx.x; i < npix * g.T; i += kThreads) {   // t fastest: contiguous block reads
            const int j = i / g.T, t = i - j * g.T;
            float2 v = make_float2(0.0f, 0.0f);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const LrCover cv = lr_cover(g, swin, e, qy, qx0, j / W, j % W, c);
                if (cv.n >= 0) {
                    const float2 b = blocks[((long)cv.n * P + cv.p) * g.T + t];
                    v.x = fmaf(cv.w, b.x, v.x); v.y = fmaf(cv.w, b.y, v.y);
                }
            }
            tile[t * (kPix + 1) + j] = v;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < npix * g.T; i += kThreads) {       // x fastest: image writes in x-runs
        const int t = i / npix, j = i - t * npix;
        const int iyq = j / W, xr = j - iyq * W;
        const int y = qy * g.s + iyq - g.py0, x = qx0 * g.s + xr - g.px0;
        if (y >= 0 && y < g.Y && x >= 0 && x < g.X) {
            float2 v = tile[t * (kPix + 1) + j];
            if (wgt) { const float d = 1.0f / (wgt[(long)y * g.X + x] + 1e-8f); v.x *= d; v.y *= d; }
            img[(((long)e * g.T + t) * g.Y + y) * g.X + x] = v;
        }
    }
}

__global__ void __launch_bounds__(kThreads) lr_compose_kernel(const float2* L, const float2* R, const float* wgt,
                                                              const float* win, float2* img, LrGeo g, int r, int vec) {
    __shared__ float2 sR[2 * (kMaxQ + 1) * kMaxT * kMaxR];           // slot (cy, bx - qx0 + 1): R of that block
    __shared__ float2 sL[4 * kPix * kLS];                            // [c][pixel][k], window applied, 0 off the grid
    __shared__ float swin[16];
    const int nqx = g.nbx + 1;
    const int qx0 = blockIdx.x * g.qw, qy = blockIdx.y, e = blockIdx.z;
    const int nq = min(g.qw, nqx - qx0);
    const int W = nq * g.s, npix = g.s * W;
    const long P = (long)g.E * g.b * g.b;
    const int TR = g.T * r;
    if (threadIdx.x < g.b) swin[threadIdx.x] = win[threadIdx.x];
    for (int sl = 0; sl < 2 * (nq + 1); ++sl) {
        const int by = qy - 1 + sl / (nq + 1), bx = qx0 - 1 + sl % (nq + 1);
        if (by >= 0 && by < g.nby && bx >= 0 && bx < g.nbx)
            stage_flat(sR + sl * TR, R + ((long)by * g.nbx + bx) * TR, TR, vec);
    }
    __syncthreads();
    // L rows: k fastest, then ix', so a run of s r complex per (c, quadrant, iy') is contiguous
    const int kv = vec ? 2 : 1, rk = r / kv;
    for (int i = threadIdx.x; i < 4 * npix * rk; i += kThreads) {
        const int k = (i % rk) * kv, cj = i / rk;
        const int j = cj % npix, c = cj / npix;
        const LrCover cv = lr_cover(g, swin, e, qy, qx0, j / W, j % W, c);
        float2 a = make_float2(0.0f, 0.0f), b2 = a;
        if (cv.n >= 0) {
            const float2* src = L + ((long)cv.n * P + cv.p) * r + k;
            if (vec) {
                const float4 v = *reinterpret_cast<const float4*>(src);
                a = make_float2(v.x * cv.w, v.y * cv.w);
                b2 = make_float2(v.z * cv.w, v.w * cv.w);
            } else {
                a = make_float2(src->x * cv.w, src->y * cv.w);
            }
        }
        sL[(c * kPix + j) * kLS + k] = a;
        if (vec) sL[(c * kPix + j) * kLS + k + 1] = b2;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < npix * g.T; i += kThreads) {       // x fastest: image writes in x-runs
        const int t = i / npix, j = i - t * npix;
        const int iyq = j / W, xr = j - iyq * W;
        const int y = qy * g.s + iyq - g.py0, x = qx0 * g.s + xr - g.px0;
        if (y < 0 || y >= g.Y || x < 0 || x >= g.X) continue;
        const int q = xr / g.s;
        float2 v = make_float2(0.0f, 0.0f);
#pragma unroll
        for (int c = 0; c < 4; ++c) {                                // an absent block has zero rows in sL
            const int cy = c >> 1, cx = c & 1;
            const int by = qy - 1 + cy, bx = qx0 + q - 1 + cx;
            if (by < 0 || by >= g.nby || bx < 0 || bx >= g.nbx) continue;
            const float2* rr = sR + (cy * (nq + 1) + q + cx) * TR + t * r;
            const float2* ll = sL + (c * kPix + j) * kLS;
            float2 a = make_float2(0.0f, 0.0f);
            for (int k = 0; k < r; ++k) cfma_conj(a, ll[k], rr[k]);
            v.x += a.x; v.y += a.y;
        }
        if (wgt) { const float d = 1.0f / (wgt[(long)y * g.X + x] + 1e-8f); v.x *= d; v.y *= d; }
        img[(((long)e * g.T + t) * g.Y + y) * g.X + x] = v;
    }
}

// ------------------------------------------------------------------ decompose: one block SVD per workgroup
// Hestenes one-sided Jacobi on the T columns of the block matrix B [M = E b^2, T], held
// column-major in LDS (sB[t M + p]) beside V [T, T] (sV[k T + t], the identity at the
// start).  A step of the round-robin tournament has T / 2 disjoint column pairs; pair k is
// rotated by the 16 lanes of group k = threadIdx.x / 16 (one DPP row): lane l holds rows
// l, l + 16, ... (M / 16 of them, a template parameter: 8-B LDS accesses, the rows kept in
// registers), the four sums alpha, beta, Re gamma, Im gamma are reduced inside the row in a
// fixed order, and every lane of the group computes the same c, s, phi and rotates its rows
// of both columns (and of V) in place.  The host launches at least 16 (T + 1) / 2 threads, so
// a step is one pass; a barrier separates the steps.
constexpr int kSvdMaxSweeps = 30;
constexpr float kSvdTol = 1.1920928955078125e-7f;          // 2^-23: |gamma| <= tol sqrt(alpha beta) is orthogonal
constexpr float kSvdNull = 9.094947017729282e-13f;         // 2^-40 of the largest initial squared column norm

// sum over the 16 lanes of a DPP row (quad_perm xor 1, xor 2, row_half_mirror, row_mirror):
// every step adds two partial sums of disjoint halves, so all 16 lanes end with the same
// bits.  All 16 lanes of the row must be active (the callers keep a group's control flow uniform).
DLCS_DEV float row16_sum(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));
}

// squared norm of a column of n rows (n = 0: an idle group, which still takes part in the reduction)
DLCS_DEV float col_norm2(const float2* col, int n, int lane) {
    float a = 0.0f;
    for (int i = lane; i < n; i += 16) {
        const float2 v = col[i];
        a = fmaf(v.x, v.x, a); a = fmaf(v.y, v.y, a);
    }
    return row16_sum(a);
}

// a_p <- c a_p - conj(m) a_q,  a_q <- m a_p + c a_q  (m = s phi)
DLCS_DEV void rotate2(float2& a, float2& b, float c, float2 m) {
    float2 na, nb;
    na.x = fmaf(c, a.x, -fmaf(m.x, b.x, m.y * b.y));
    na.y = fmaf(c, a.y, -fmaf(m.x, b.y, -m.y * b.x));
    nb.x = fmaf(c, b.x, fmaf(m.x, a.x, -m.y * a.y));
    nb.y = fmaf(c, b.y, fmaf(m.x, a.y, m.y * a.x));
    a = na; b = nb;
}

// One column pair by one 16-lane group: lane l holds rows l + 16 (k ^ k0), k < NIT = M / 16, of
// both columns in registers between the sums and the rotation, so a step reads and writes
// each row once and all its LDS reads are in flight together.  k0 = 1 in odd groups starts
// them 16 rows (32 banks) down, so that the two groups of a 32-lane half use other banks.
// An idle group (act false) adds zeros and still takes part in the reductions.  Returns
// whether the pair was rotated (the same in all 16 lanes).
template <int NIT>
DLCS_DEV bool svd_pair(float2* cp, float2* cq, float2* vp, float2* vq, int T, bool act, int lane, int k0, float thr) {
    float2 a[NIT], b[NIT];
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        a[k] = b[k] = make_float2(0.0f, 0.0f);
        if (act) { a[k] = cp[lane + 16 * (k ^ k0)]; b[k] = cq[lane + 16 * (k ^ k0)]; }
    }
    float al = 0.0f, be = 0.0f, gr = 0.0f, gi = 0.0f;
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        al = fmaf(a[k].x, a[k].x, al); al = fmaf(a[k].y, a[k].y, al);
        be = fmaf(b[k].x, b[k].x, be); be = fmaf(b[k].y, b[k].y, be);
        gr = fmaf(a[k].x, b[k].x, gr); gr = fmaf(a[k].y, b[k].y, gr);      // gamma = a_p^H a_q
        gi = fmaf(a[k].x, b[k].y, gi); gi = fmaf(-a[k].y, b[k].x, gi);
    }
    al = row16_sum(al); be = row16_sum(be); gr = row16_sum(gr); gi = row16_sum(gi);
    const float absg = sqrtf(fmaf(gr, gr, gi * gi));
    if (!(act && al > thr && be > thr && absg > kSvdTol * (sqrtf(al) * sqrtf(be)))) return false;
    const float z = (be - al) / (2.0f * absg);
    const float t = (z >= 0.0f ? 1.0f : -1.0f) / (fabsf(z) + sqrtf(fmaf(z, z, 1.0f)));
    const float c = 1.0f / sqrtf(fmaf(t, t, 1.0f));
    const float s = c * t;
    const float2 m = make_float2(s * (gr / absg), s * (gi / absg));
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        rotate2(a[k], b[k], c, m);
        cp[lane + 16 * (k ^ k0)] = a[k]; cq[lane + 16 * (k ^ k0)] = b[k];
    }
    for (int i = lane; i < T; i += 16) {                   // the same rotation on V's columns
        float2 x = vp[i], y = vq[i];
        rotate2(x, y, c, m);
        vp[i] = x; vq[i] = y;
    }
    return true;
}

template <int NIT>
__global__ void __launch_bounds__(kThreads) lr_decompose_kernel(const float2* img, const float* win, float2* L,
                                                                float2* R, float* S, int* info, LrGeo g, int r) {
    extern __shared__ float2 svd_smem[];                   // sB [T][M], then sV [T][T]
    __shared__ float swin[16];
    __shared__ float s_n2[kMaxT];                          // squared column norms
    __shared__ int s_order[kMaxR], s_null[kMaxR];          // output component j: its column, sigma^2 null
    __shared__ float2 s_sl[kMaxR], s_sr[kMaxR];            // phase / sqrt(sigma), phase sqrt(sigma)
    __shared__ int s_rot;                                  // a pair of this sweep was rotated
    const int T = g.T, M = 16 * NIT;                       // M = E b^2, a multiple of 16
    float2* sB = svd_smem;
    float2* sV = svd_smem + T * M;
    const int n = blockIdx.x, nthr = blockDim.x;
    const int lane = threadIdx.x & 15, grp = threadIdx.x >> 4, ngrp = nthr >> 4;

    // ---- stage the block as lr_extract_kernel does (x-runs; divide 0), V = identity
    if (threadIdx.x < g.b) swin[threadIdx.x] = win[threadIdx.x];
    __syncthreads();
    {
        const int by = n / g.nbx, bx = n % g.nbx, bb = g.b * g.b;
        for (int i = threadIdx.x; i < M * T; i += nthr) {
            const int p = i % M, t = i / M;
            const int e = p / bb, q = p - e * bb;
            const int iy = q / g.b, ix = q - iy * g.b;
            const int y = by * g.s + iy - g.py0, x = bx * g.s + ix - g.px0;
            float2 v = make_float2(0.0f, 0.0f);
            if (y >= 0 && y < g.Y && x >= 0 && x < g.X) {
                v = img[(((long)e * T + t) * g.Y + y) * g.X + x];
                const float w = swin[iy] * swin[ix];
                v.x *= w; v.y *= w;
            }
            sB[t * M + p] = v;
        }
        for (int i = threadIdx.x; i < T * T; i += nthr) sV[i] = make_float2(i / T == i % T ? 1.0f : 0.0f, 0.0f);
    }
    __syncthreads();

    // ---- the null threshold from the initial column norms
    for (int t0 = 0; t0 < T; t0 += ngrp) {
        const int t = t0 + grp;
        const float n2 = col_norm2(sB + (t < T ? t : 0) * M, t < T ? M : 0, lane);
        if (t < T && lane == 0) s_n2[t] = n2;
    }
    __syncthreads();
    float thr = 0.0f;
    for (int t = 0; t < T; ++t) thr = fmaxf(thr, s_n2[t]);
    thr *= kSvdNull;

    // ---- sweeps: np - 1 steps over np = T rounded up to even players; an index >= T is the bye
    const int np = (T + 1) & ~1, half = np >> 1;
    int sweeps = 0;
    while (sweeps < kSvdMaxSweeps) {
        if (threadIdx.x == 0) s_rot = 0;
        __syncthreads();
        for (int step = 0; step < np - 1; ++step) {
            int p = 0, q = 0;
            bool act = grp < half;
            if (act) {                                     // circle method: player np - 1 stays, the rest turn
                const int a = grp == 0 ? np - 1 : (step + grp) % (np - 1);
                const int c = grp == 0 ? step : (step - grp + np - 1) % (np - 1);
                p = a < c ? a : c; q = a < c ? c : a;
                act = q < T;
            }
            const int k0 = (NIT > 1 && (grp & 1)) ? 1 : 0;
            if (svd_pair<NIT>(sB + p * M, sB + q * M, sV + p * T, sV + q * T, T, act, lane, k0, thr) && lane == 0)
                s_rot = 1;
            __syncthreads();
        }
        ++sweeps;
        const int rotated = s_rot;
        __syncthreads();                                   // all have read s_rot before it is cleared
        if (!rotated) break;
    }

    // ---- order the columns by sigma^2 descending (ties: the lower column first), phases, scales
    for (int t0 = 0; t0 < T; t0 += ngrp) {
        const int t = t0 + grp;
        const float n2 = col_norm2(sB + (t < T ? t : 0) * M, t < T ? M : 0, lane);
        if (t < T && lane == 0) s_n2[t] = n2;
    }
    if (threadIdx.x < r) s_order[threadIdx.x] = threadIdx.x;       // NaN norms rank nothing: keep the indices valid
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += nthr) {
        const float v = s_n2[t];
        int rank = 0;
        for (int j = 0; j < T; ++j) { const float u = s_n2[j]; rank += (u > v || (u == v && j < t)) ? 1 : 0; }
        if (rank < r) s_order[rank] = t;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < r; j += nthr) {
        const int k = s_order[j];
        const float s2 = s_n2[k];
        const float sig = sqrtf(s2), rs = sqrtf(sig);
        // the unit phase that makes the largest entry of v_k real and positive (the lowest t on a tie)
        float best = -1.0f;
        float2 vb = make_float2(1.0f, 0.0f);
        for (int t = 0; t < T; ++t) {
            const float2 v = sV[k * T + t];
            const float m2 = fmaf(v.x, v.x, v.y * v.y);
            if (m2 > best) { best = m2; vb = v; }
        }
        const float mag = sqrtf(best);
        const float2 ph = mag > 0.0f ? make_float2(vb.x / mag, -vb.y / mag) : make_float2(1.0f, 0.0f);
        const int null = !(s2 > thr);
        s_null[j] = null;
        s_sl[j] = null ? make_float2(0.0f, 0.0f) : make_float2(ph.x / rs, ph.y / rs);
        s_sr[j] = make_float2(ph.x * rs, ph.y * rs);
        if (S) S[(long)n * r + j] = sig;
    }
    if (info && threadIdx.x == 0) info[n] = sweeps;
    __syncthreads();

    // ---- L[n, p, j] = a_k[p] phase / sqrt(sigma),  R[n, t, j] = v_k[t] phase sqrt(sigma);  0 for a null sigma^2
    float2* Ln = L + (long)n * M * r;
    for (int i = threadIdx.x; i < M * r; i += nthr) {
        const int p = i / r, j = i - p * r;
        float2 o = make_float2(0.0f, 0.0f);
        if (!s_null[j]) {
            const float2 a = sB[s_order[j] * M + p], sc = s_sl[j];
            o.x = fmaf(a.x, sc.x, -a.y * sc.y);
            o.y = fmaf(a.x, sc.y, a.y * sc.x);
        }
        Ln[i] = o;
    }
    float2* Rn = R + (long)n * T * r;
    for (int i = threadIdx.x; i < T * r; i += nthr) {
        const int t = i / r, j = i - t * r;
        float2 o = make_float2(0.0f, 0.0f);
        if (!s_null[j]) {
            const float2 a = sV[s_order[j] * T + t], sc = s_sr[j];
            o.x = fmaf(a.x, sc.x, -a.y * sc.y);
            o.y = fmaf(a.x, sc.y, a.y * sc.x);
        }
        Rn[i] = o;
    }
}

// geometry of lowrank:47-77; false outside the supported range
bool lr_geo(int64_t E, int64_t T, int64_t Y, int64_t X, int64_t b, LrGeo* g) {
    if (!(b == 4 || b == 8 || b == 16)) return false;
    if (E < 1 || E > kMaxE || T < 1 || T > kMaxT || Y < 1 || X < 1 || Y > 32768 || X > 32768) return false;
    g->E = (int)E; g->T = (int)T; g->Y = (int)Y; g->X = (int)X; g->b = (int)b; g->s = (int)b / 2;
    const int Yp = (int)(b * (Y / b + 1)), Xp = (int)(b * (X / b + 1));
    g->py0 = (Yp - (int)Y) / 2;
    g->px0 = (Xp - (int)X) / 2;
    g->nby = (Yp - (int)b) / g->s + 1;
    g->nbx = (Xp - (int)b) / g->s + 1;
    g->qw = kPix / (g->s * g->s) < kMaxQ ? kPix / (g->s * g->s) : kMaxQ;
    return g->nby + 1 <= 65535;
}

}  // namespace

extern "C" {

int dlcs_lr_extract(const void* image, const float* weights, const float* win, int divide, void* blocks, int64_t E,
                    int64_t T, int64_t Y, int64_t X, int64_t b, dlcs_stream_t stream) {
    LrGeo g;
    DLCS_CHECK_ARG(image && win && blocks && (!divide || weights));
    if (!lr_geo(E, T, Y, X, b, &g)) return DLCS_ERR_UNSUPPORTED_SIZE;
    const int P = g.E * g.b * g.b, rows = P < kRows ? P : kRows;
    const long nwg = (long)g.nby * g.nbx * (P / rows);
    const int vec = (g.T % 2 == 0) && al16(blocks);
    hipLaunchKernelGGL(lr_extract_kernel, dim3((unsigned)nwg), dim3(kThreads), 0, (hipStream_t)stream,
                       (const float2*)image, divide ? weights : nullptr, win, (float2*)blocks, g, vec);
    return dlcs_launch_status();
}

int dlcs_lr_combine(const void* blocks, const float* weights, const float* win, int divide, void* image, int64_t E,
                    int64_t T, int64_t Y, int64_t X, int64_t b, dlcs_stream_t stream) {
    LrGeo g;
    DLCS_CHECK_ARG(image && win && blocks && (!divide || weights));
    if (!lr_geo(E, T, Y, X, b, &g)) return DLCS_ERR_UNSUPPORTED_SIZE;
    const int vec = (g.T % 2 == 0) && al16(blocks);
    hipLaunchKernelGGL(lr_combine_kernel, dim3(cdiv(g.nbx + 1, g.qw), g.nby + 1, g.E), dim3(kThreads), 0,
                       (hipStream_t)stream, (const float2*)blocks, divide ? weights : nullptr, win, (float2*)image, g,
                       vec);
    return dlcs_launch_status();
}

int dlcs_lr_compose(const void* L, const void* R, const float* weights, const float* win, int divide, void* image,
                    int64_t E, int64_t T, int64_t Y, int64_t X, int64_t b, int64_t r, dlcs_stream_t stream) {
    LrGeo g;
    DLCS_CHECK_ARG(image && win && L && R && (!divide || weights));
    if (!lr_geo(E, T, Y, X, b, &g) || r < 1 || r > kMaxR) return DLCS_ERR_UNSUPPORTED_SIZE;
    const int vec = (r % 2 == 0) && al16(L) && al16(R);
    hipLaunchKernelGGL(lr_compose_kernel, dim3(cdiv(g.nbx + 1, g.qw), g.nby + 1, g.E), dim3(kThreads), 0,
                       (hipStream_t)stream, (const float2*)L, (const float2*)R, divide ? weights : nullptr, win,
                       (float2*)image, g, (int)r, vec);
    return dlcs_launch_status();
}

int dlcs_lr_project_l(const void* image, const void* R, const float* weights, const float* win, int divide, void* out,
                      int64_t E, int64_t T, int64_t Y, int64_t X, int64_t b, int64_t r, dlcs_stream_t stream) {
    LrGeo g;
    DLCS_CHECK_ARG(image && win && R && out && (!divide || weights));
    if (!lr_geo(E, T, Y, X, b, &g) || r < 1 || r > kMaxR) return DLCS_ERR_UNSUPPORTED_SIZE;
    const int P = g.E * g.b * g.b, rows = P < kRows ? P : kRows;
    const long nwg = (long)g.nby * g.nbx * (P / rows);
    const int vec_r = ((g.T * r) % 2 == 0) && al16(R) && (r % 2 == 0 || g.T % 2 == 0);
    const int vec_o = (r % 2 == 0) && al16(out);
    hipLaunchKernelGGL(lr_project_l_kernel, dim3((unsigned)nwg), dim3(kThreads), 0, (hipStream_t)stream,
                       (const float2*)image, divide ? weights : nullptr, win, (const float2*)R, (float2*)out, g, (int)r,
                       vec_r, vec_o);
    return dlcs_launch_status();
}

int dlcs_lr_project_r(const void* image, const void* L, const float* weights, const float* win, int divide, void* out,
                      int64_t E, int64_t T, int64_t Y, int64_t X, int64_t b, int64_t r, dlcs_stream_t stream) {
    LrGeo g;
    DLCS_CHECK_ARG(image && win && L && out && (!divide || weights));
    if (!lr_geo(E, T, Y, X, b, &g) || r < 1 || r > kMaxR) return DLCS_ERR_UNSUPPORTED_SIZE;
    const int vec_l = (r % 2 == 0) && al16(L);
    hipLaunchKernelGGL(lr_project_r_kernel, dim3((unsigned)(g.nby * g.nbx)), dim3(kThreads), 0, (hipStream_t)stream,
                       (const float2*)image, divide ? weights : nullptr, win, (const float2*)L, (float2*)out, g, (int)r,
                       vec_l);
    return dlcs_launch_status();
}

int dlcs_lr_decompose(const void* image, const float* win, void* L, void* R, float* S, int32_t* info, int64_t E,
                      int64_t T, int64_t Y, int64_t X, int64_t b, int64_t r, dlcs_stream_t stream) {
    LrGeo g;
    DLCS_CHECK_ARG(image && win && L && R);
    if (!lr_geo(E, T, Y, X, b, &g) || r < 1 || r > kMaxR || r > T) return DLCS_ERR_UNSUPPORTED_SIZE;
    // 16 lanes per pair of a step, whole waves: 64 threads up to T = 8, 256 from T = 25
    const int pairs = (g.T + 1) / 2;
    const int threads = (16 * pairs + 63) & ~63;
    const size_t sm = (size_t)g.T * (g.E * g.b * g.b + g.T) * sizeof(float2);   // at most 136 KiB
    auto launch = [&](auto NIT) {
        constexpr int nit = decltype(NIT)::value;
        (void)hipFuncSetAttribute((const void*)lr_decompose_kernel<nit>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)sm);
        hipLaunchKernelGGL(lr_decompose_kernel<nit>, dim3((unsigned)(g.nby * g.nbx)), dim3(threads), sm,
                           (hipStream_t)stream, (const float2*)image, win, (float2*)L, (float2*)R, S, (int*)info, g,
                           (int)r);
    };
    switch (g.E * g.b * g.b / 16) {                        // rows per lane: E b^2 / 16
        case 1: launch(std::integral_constant<int, 1>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        case 4: launch(std::integral_constant<int, 4>{}); break;
        case 8: launch(std::integral_constant<int, 8>{}); break;
        case 16: launch(std::integral_constant<int, 16>{}); break;
        default: launch(std::integral_constant<int, 32>{}); break;
    }
    return dlcs_launch_status();
}

}  // extern "C"
