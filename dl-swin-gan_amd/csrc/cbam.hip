// Spatial gate of the CBAM-ResNet regulariser (reference CBAM.py:425-521) around the
// fused ResNet conv trunk and the SE channel gate (se.hip), fp32 (the five row passes
// also on bf16 rows, their *_bf16 entry points: se_rows.h).  Row operands are the
// conv node's patch-blocked channels-last rows [B nT nY nX 64, ld] of a [B, D, H, W]
// grid (D, H, W multiples of 4; row formula in layout.hip); maps are dense [B, D, H, W]:
//
// * dlcs_cbam_chan_mean        a[b, v] = (1 / C) sum_c gate[b, c] o[v, c]
// * dlcs_cbam_stencil5         out = bias + w5 * in (5 x 5 x 5 cross-correlation, zero
//                              border), or the transposed form (flipped kernel, no bias)
// * dlcs_cbam_stencil5_wgrad   dw5[d] += sum_{b, v} dq[b, v] a[b, v + d], db5 += sum dq
// * dlcs_cbam_scale_res_relu   out = relu(q[v] gate[b, c] o + res)
// * dlcs_cbam_bwd_rowdot       dq[b, v] = sum_c g [r_next > 0] gate[b, c] o
// * dlcs_cbam_bwd_reduce       dgate[b, c] = sum_v (g [r_next > 0] q[v] + da[v] / C) o
// * dlcs_cbam_bwd_apply        g <- g [r_next > 0] in place,
//                              dout = (g q[v] + da[v] / C) gate[b, c] + dmean[b, c]
//
// The element-wise passes and the reduction over voxels keep se.hip's geometry (a
// thread owns one column chunk and walks rows; 16-B accesses when C % 4 == 0,
// ld % 4 == 0 and the pointers are aligned, else one float; columns [C, ld) are never
// touched) and read their map values through the row -> voxel formula.  The two row
// dots give a power-of-two group of lanes to each row and sum the group across lanes.  The stencils work on a 4 x 8 x 32 tile with a 2-voxel halo in LDS, one
// thread per (y, x) column of 4 outputs.  Both reductions store per-workgroup partials
// in the caller's workspace and sum them in a fixed order: no float atomics.
#include "se_rows.h"

namespace {

constexpr int kTT = 4, kTY = 8, kTX = 32;                 // stencil tile (t, y, x): 256 threads x 4 outputs
constexpr int kHT = kTT + 4, kHY = kTY + 4, kHX = kTX + 4; // with the halo
constexpr int kTaps = 125;
constexpr int kWgPart = 128;                               // floats per wgrad partial row: 125 taps, the bias, 2 unused
constexpr long kWgBlocks = 1024;                           // workgroups of the wgrad at most

// the grid of a row operand: a batch item's rows are its nT nY nX patches of 64
struct CbGrid {
    long N;            // voxels (= rows) per batch item
    int H, W;
    unsigned nY, nX;
};

// row within a batch item -> dense voxel index within that item
DLCS_DEV long cb_voxel(long rl, const CbGrid& gd) {
    const unsigned p = (unsigned)(rl >> 6);
    const int ip = (int)(rl & 63);
    const unsigned px = p % gd.nX, t1 = p / gd.nX;
    const unsigned py = t1 % gd.nY, pt = t1 / gd.nY;
    return ((long)(pt * 4 + (ip >> 4)) * gd.H + (py * 4 + ((ip >> 2) & 3))) * gd.W + px * 4 + (ip & 3);
}

// sum over the aligned group of L lanes (a power of two) that holds a row, in every lane
// of the group: xor shuffles down to 16 lanes, then DPP inside the 16-lane row (quad_perm
// xor 1 / xor 2, row_half_mirror, row_mirror: each step pairs a lane with one holding the
// other half of its group) -- a fixed order, and no LDS round trip on the 16-B path (L <= 16)
DLCS_DEV float cb_group_sum(float v, int L) {
    for (int m = L >> 1; m >= 16; m >>= 1) v += __shfl_xor(v, m, 64);
    if (L >= 2) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
    if (L >= 4) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));
    if (L >= 8) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));
    if (L >= 16) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));
    return v;
}

// ------------------------------------------------------------------ row dots
// map[b, voxel(row)] = scale sum_c gate[b, c] x[row, c], x = o (BWD false) or
// g [r_next > 0] o (BWD true).  A row belongs to L lanes (a power of two; at most 16 on
// the 16-B path, so a 64-channel row is one access per lane and wider rows amortise the
// lane sum over several, at most 64 on the scalar path): lane j takes the column chunks
// j, j + L, ...; the gate row sits in LDS; 4 rows in flight per lane.
template <typename T, int V, bool BWD>
__global__ void __launch_bounds__(256) cbam_rowdot_kernel(const T* o, const T* g, const T* rn,
                                                          const float* gate, float scale, float* map, CbGrid gd, int C,
                                                          long ld, long rows_per_block, int L) {
    __shared__ __attribute__((aligned(16))) float sg[kSeMaxC];
    const long b = blockIdx.y;
    for (int c = threadIdx.x; c < C; c += 256) sg[c] = gate[b * C + c];
    __syncthreads();
    const int nch = C / V;
    const int sub = threadIdx.x & (L - 1), slot = threadIdx.x / L, nslots = 256 / L;
    const long r0 = (long)blockIdx.x * rows_per_block;
    const long r1 = min(gd.N, r0 + rows_per_block);
    constexpr int U = 4;                                   // rows in flight per thread
    for (long r = r0 + slot; r < r1; r += (long)U * nslots) {
        float acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = 0.0f;
        for (int ch = sub; ch < nch; ch += L) {
            const int col = ch * V;
            SeVec<V> fo[U], fg[BWD ? U : 1], fr[BWD ? U : 1];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long ru = r + (long)u * nslots;
                if (ru < r1) {
                    const long off = (b * gd.N + ru) * ld + col;
                    fo[u] = se_load<V>(o + off);
                    if constexpr (BWD) { fg[u] = se_load<V>(g + off); fr[u] = se_load<V>(rn + off); }
                }
            }
            const SeVec<V> s = se_load<V>(sg + col);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (r + (long)u * nslots < r1) {
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        if constexpr (BWD) acc[u] += (fr[u].v[e] > 0.0f) ? fg[u].v[e] * s.v[e] * fo[u].v[e] : 0.0f;
                        else acc[u] += s.v[e] * fo[u].v[e];
                    }
                }
            }
        }
        // every lane of a row's group has the same r, so the whole group is here
#pragma unroll
        for (int u = 0; u < U; ++u) {
            acc[u] = cb_group_sum(acc[u], L);
            const long ru = r + (long)u * nslots;
            if (sub == 0 && ru < r1) map[b * gd.N + cb_voxel(ru, gd)] = acc[u] * scale;
        }
    }
}

// ------------------------------------------------------------------ reduction over voxels
// part[(b G + blockIdx.x) C + c] = sum over this workgroup's rows of
// (g [r_next > 0] q[v] + da[v] inv_c) o; se_reduce_kernel's layout and order.
template <typename T, int V>
__global__ void __launch_bounds__(256) cbam_reduce_kernel(const T* o, const T* g, const T* rn, const float* q,
                                                          const float* da, float inv_c, CbGrid gd, int C, long ld,
                                                          long rows_per_block, float* part) {
    __shared__ float sm[256 * V];
    const int nch = C / V;
    const int cpb = nch < 256 ? nch : 256;
    const int ngrp = 256 / cpb;
    const int ch = threadIdx.x % cpb, grp = threadIdx.x / cpb;
    const long b = blockIdx.y;
    const long r0 = (long)blockIdx.x * rows_per_block;
    const long r1 = min(gd.N, r0 + rows_per_block);
    float* dst = part + (b * gridDim.x + blockIdx.x) * C;
    for (int cb = 0; cb < nch; cb += cpb) {
        float acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.0f;
        if (grp < ngrp && cb + ch < nch) {
            const long col = (long)(cb + ch) * V;
            constexpr int U = 4;
            for (long r = r0 + grp; r < r1; r += (long)U * ngrp) {
                SeVec<V> fo[U], fg[U], fr[U];
                float fq[U], fd[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const long ru = r + (long)u * ngrp;
                    if (ru < r1) {
                        const long off = (b * gd.N + ru) * ld + col;
                        const long vx = b * gd.N + cb_voxel(ru, gd);
                        fo[u] = se_load<V>(o + off);
                        fg[u] = se_load<V>(g + off);
                        fr[u] = se_load<V>(rn + off);
                        fq[u] = q[vx];
                        fd[u] = da[vx] * inv_c;
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (r + (long)u * ngrp < r1) {
#pragma unroll
                        for (int e = 0; e < V; ++e) {
                            const float gz = (fr[u].v[e] > 0.0f) ? fg[u].v[e] : 0.0f;
                            acc[e] += (gz * fq[u] + fd[u]) * fo[u].v[e];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) sm[threadIdx.x * V + e] = acc[e];
        __syncthreads();
        for (int i = threadIdx.x; i < cpb * V; i += 256) {
            const int cc = i / V, e = i % V;
            if (cb + cc < nch) {
                float s = 0.0f;
                for (int k = 0; k < ngrp; ++k) s += sm[(k * cpb + cc) * V + e];
                dst[(cb + cc) * V + e] = s;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ element-wise passes
// APPLY_BWD false: out = relu(q[v] gate o + res) (a = o, bsrc = res; out may alias res).
// APPLY_BWD true : g (= gio) <- g [r_next > 0] in place (a = r_next),
//                  out = (g q[v] + da[v] inv_c) gate + dmean.
template <typename T, int V, bool APPLY_BWD>
__global__ void __launch_bounds__(256) cbam_rows_kernel(const T* a, const T* bsrc, T* gio, const float* gate,
                                                        const float* q, const float* da, float inv_c, const float* dmean,
                                                        T* out, CbGrid gd, int C, long ld, long rows_per_block) {
    const int nch = C / V;
    const int cpb = nch < 256 ? nch : 256;
    const int ngrp = 256 / cpb;
    const int ch = threadIdx.x % cpb, grp = threadIdx.x / cpb;
    if (grp >= ngrp) return;
    const long b = blockIdx.y;
    const long r0 = (long)blockIdx.x * rows_per_block;
    const long r1 = min(gd.N, r0 + rows_per_block);
    for (int cb = 0; cb + ch < nch; cb += cpb) {
        const long col = (long)(cb + ch) * V;
        float s[V], d[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            s[e] = gate[b * C + col + e];
            if constexpr (APPLY_BWD) d[e] = dmean[b * C + col + e];
            else d[e] = 0.0f;
        }
        constexpr int U = 4;
        for (long r = r0 + grp; r < r1; r += (long)U * ngrp) {
            SeVec<V> fa[U], fb[U];
            float fq[U], fd[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long ru = r + (long)u * ngrp;
                if (ru < r1) {
                    const long off = (b * gd.N + ru) * ld + col;
                    const long vx = b * gd.N + cb_voxel(ru, gd);
                    fa[u] = se_load<V>(a + off);
                    fb[u] = se_load<V>((APPLY_BWD ? gio : bsrc) + off);
                    fq[u] = q[vx];
                    if constexpr (APPLY_BWD) fd[u] = da[vx] * inv_c;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long ru = r + (long)u * ngrp;
                if (ru < r1) {
                    const long off = (b * gd.N + ru) * ld + col;
                    SeVec<V> y;
                    if constexpr (APPLY_BWD) {
#pragma unroll
                        for (int e = 0; e < V; ++e) {
                            if (!(fa[u].v[e] > 0.0f)) fb[u].v[e] = 0.0f;
                            y.v[e] = (fb[u].v[e] * fq[u] + fd[u]) * s[e] + d[e];
                        }
                        se_store<V>(gio + off, fb[u]);
                    } else {
#pragma unroll
                        for (int e = 0; e < V; ++e) {
                            const float v = fq[u] * s[e] * fa[u].v[e] + fb[u].v[e];
                            y.v[e] = v > 0.0f ? v : 0.0f;
                        }
                    }
                    se_store<V>(out + off, y);
                }
            }
        }
    }
}

// ------------------------------------------------------------------ stencils
struct CbTiles {
    int D, H, W;
    int ntt, nty, ntx;     // tiles along t, y, x
};

// sa[kHT][kHY][kHX] <- the tile at (t0, y0, x0) of item `src` with its halo; outside the grid: 0, not loaded
// (all of a thread's loads are issued before its first LDS store)
DLCS_DEV void cb_load_tile(float* sa, const float* src, int t0, int y0, int x0, const CbTiles& tl) {
    constexpr int kElems = kHT * kHY * kHX, kIter = (kElems + 255) / 256;
    float v[kIter];
#pragma unroll
    for (int k = 0; k < kIter; ++k) {
        const int i = threadIdx.x + k * 256;
        const int xx = i % kHX, yy = (i / kHX) % kHY, tt = i / (kHX * kHY);
        const int t = t0 + tt - 2, y = y0 + yy - 2, x = x0 + xx - 2;
        v[k] = 0.0f;
        if (i < kElems && t >= 0 && t < tl.D && y >= 0 && y < tl.H && x >= 0 && x < tl.W)
            v[k] = src[((long)t * tl.H + y) * tl.W + x];
    }
#pragma unroll
    for (int k = 0; k < kIter; ++k) {
        const int i = threadIdx.x + k * 256;
        if (i < kElems) sa[i] = v[k];
    }
}

// tile index -> (b, t0, y0, x0)
DLCS_DEV void cb_tile_origin(long tile, const CbTiles& tl, long& b, int& t0, int& y0, int& x0) {
    x0 = (int)(tile % tl.ntx) * kTX; tile /= tl.ntx;
    y0 = (int)(tile % tl.nty) * kTY; tile /= tl.nty;
    t0 = (int)(tile % tl.ntt) * kTT;
    b = tile / tl.ntt;
}

// out[b, v] = bias + sum_d w[d] in[b, v + d - 2]; TRANSPOSED: sum_d w[d] in[b, v - (d - 2)], no bias
// (the flipped kernel).  The weight index is a compile-time constant, so the 125 weights
// come through uniform loads into scalar registers.
template <bool TRANSPOSED>
__global__ void __launch_bounds__(256) cbam_stencil_kernel(const float* __restrict__ in, const float* __restrict__ w5,
                                                           const float* __restrict__ bias, float* __restrict__ out,
                                                           CbTiles tl) {
    __shared__ float sa[kHT * kHY * kHX];
    long b; int t0, y0, x0;
    cb_tile_origin(blockIdx.x, tl, b, t0, y0, x0);
    const long item = (long)tl.D * tl.H * tl.W;
    cb_load_tile(sa, in + b * item, t0, y0, x0, tl);
    __syncthreads();
    const int lx = threadIdx.x & (kTX - 1), ly = threadIdx.x / kTX;
    const float b0 = TRANSPOSED ? 0.0f : bias[0];
    float acc[kTT];
#pragma unroll
    for (int j = 0; j < kTT; ++j) acc[j] = b0;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy)
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) {
            float col[kHT];
#pragma unroll
            for (int j = 0; j < kHT; ++j) col[j] = sa[(j * kHY + ly + dy) * kHX + lx + dx];
#pragma unroll
            for (int dt = 0; dt < 5; ++dt) {
                const float wv = w5[TRANSPOSED ? kTaps - 1 - (dt * 25 + dy * 5 + dx) : dt * 25 + dy * 5 + dx];
#pragma unroll
                for (int j = 0; j < kTT; ++j) acc[j] += wv * col[j + dt];
            }
        }
    const int y = y0 + ly, x = x0 + lx;
    if (y < tl.H && x < tl.W) {
#pragma unroll
        for (int j = 0; j < kTT; ++j)
            if (t0 + j < tl.D) out[b * item + ((long)(t0 + j) * tl.H + y) * tl.W + x] = acc[j];
    }
}

// part[blockIdx.x][d] = sum over this workgroup's tiles of dq[v] a[v + d - 2] (d < 125),
// part[blockIdx.x][125] = sum dq: 126 accumulators per thread over its (y, x) columns.
// The wave sums them as a halving butterfly: at each of six steps a lane keeps one half of
// its values, hands the other half to the lane across the step's bit and adds what it
// receives (128, 64, ... 2 values per lane: 126 exchanges instead of 6 x 126), the first two
// steps as v_permlane32_swap / v_permlane16_swap of the (low, high) pair; lane l ends with
// the wave's sums 2 l and 2 l + 1.  Then the four waves in ascending order.
__global__ void __launch_bounds__(256) cbam_wgrad_kernel(const float* dq, const float* a, CbTiles tl, long ntiles,
                                                         float* part) {
    __shared__ float sa[kHT * kHY * kHX];
    __shared__ float sr[4][kWgPart];
    const long item = (long)tl.D * tl.H * tl.W;
    const int lx = threadIdx.x & (kTX - 1), ly = threadIdx.x / kTX;
    float acc[kWgPart];                                    // 125 taps, the bias, two zeros
#pragma unroll
    for (int i = 0; i < kWgPart; ++i) acc[i] = 0.0f;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        long b; int t0, y0, x0;
        cb_tile_origin(tile, tl, b, t0, y0, x0);
        __syncthreads();                                   // the previous tile's readers are done
        cb_load_tile(sa, a + b * item, t0, y0, x0, tl);
        const int y = y0 + ly, x = x0 + lx;
        float dv[kTT];
#pragma unroll
        for (int j = 0; j < kTT; ++j)
            dv[j] = (y < tl.H && x < tl.W && t0 + j < tl.D) ? dq[b * item + ((long)(t0 + j) * tl.H + y) * tl.W + x] : 0.0f;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kTT; ++j) acc[kTaps] += dv[j];
#pragma unroll
        for (int dy = 0; dy < 5; ++dy)
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) {
                float col[kHT];
#pragma unroll
                for (int j = 0; j < kHT; ++j) col[j] = sa[(j * kHY + ly + dy) * kHX + lx + dx];
#pragma unroll
                for (int dt = 0; dt < 5; ++dt)
#pragma unroll
                    for (int j = 0; j < kTT; ++j) acc[dt * 25 + dy * 5 + dx] += dv[j] * col[j + dt];
            }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < 64; ++i) {                         // lanes 0..31 keep [0, 64), lanes 32..63 [64, 128)
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[i]), __float_as_uint(acc[i + 64]), false, false);
        acc[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
#pragma unroll
    for (int i = 0; i < 32; ++i) {                         // even 16-lane rows keep [0, 32), odd rows [32, 64)
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[i]), __float_as_uint(acc[i + 32]), false, false);
        acc[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {                          // lane bits 8, 4, 2, 1: 16, 8, 4, 2 values kept
        const int h = 16 >> s, m = 8 >> s;
        const bool up = (lane & m) != 0;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (i < h) {
                const float keep = up ? acc[i + h] : acc[i], send = up ? acc[i] : acc[i + h];
                acc[i] = keep + __shfl_xor(send, m, 64);
            }
    }
    sr[wave][2 * lane] = acc[0];
    sr[wave][2 * lane + 1] = acc[1];
    __syncthreads();
    if (threadIdx.x <= kTaps)
        part[(long)blockIdx.x * kWgPart + threadIdx.x] =
            ((sr[0][threadIdx.x] + sr[1][threadIdx.x]) + sr[2][threadIdx.x]) + sr[3][threadIdx.x];
}

// dw5[d] += sum_g part[g][d], db5 += sum_g part[g][125] in a fixed order
// (se_partial_sum_kernel's: 16 columns x 64 slices per workgroup; G <= 1024, so a slice
// sums at most 16 partials into four interleaved accumulators, a dependent chain of 4;
// then the slices in ascending order).
__global__ void __launch_bounds__(1024) cbam_wgrad_sum_kernel(const float* part, int G, float* dw5, float* db5) {
    __shared__ float sm[kSeSumSlices][kSeSumCols + 1];
    const int cl = threadIdx.x % kSeSumCols, sl = threadIdx.x / kSeSumCols;
    const int c = blockIdx.x * kSeSumCols + cl;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    if (c <= kTaps) {
        int k = sl;
        for (; k + 3 * kSeSumSlices < G; k += 4 * kSeSumSlices) {
            a0 += part[(long)k * kWgPart + c];
            a1 += part[(long)(k + kSeSumSlices) * kWgPart + c];
            a2 += part[(long)(k + 2 * kSeSumSlices) * kWgPart + c];
            a3 += part[(long)(k + 3 * kSeSumSlices) * kWgPart + c];
        }
        for (; k < G; k += kSeSumSlices) a0 += part[(long)k * kWgPart + c];
    }
    sm[sl][cl] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (sl == 0 && c <= kTaps) {
        float t = 0.0f;
        for (int k = 0; k < kSeSumSlices; ++k) t += sm[k][cl];
        if (c < kTaps) dw5[c] += t;
        else db5[0] += t;
    }
}

// ------------------------------------------------------------------ host side
bool cb_dims_ok(long B, long D, long H, long W) { return B > 0 && D > 0 && H > 0 && W > 0; }
bool cb_rows_ok(long B, long D, long H, long W, long C, long ld) { return cb_dims_ok(B, D, H, W) && C > 0 && ld >= C; }
// row operands: whole 4 x 4 x 4 patches, a patch index that fits 32 bits, int extents
bool cb_rows_supported(long B, long D, long H, long W, long C) {
    return !(D % 4 || H % 4 || W % 4) && D < (1L << 24) && H < (1L << 24) && W < (1L << 24) &&
           D * H * W < (1L << 36) && se_rows_supported(B, C);
}
CbGrid cb_grid(long D, long H, long W) {
    CbGrid gd;
    gd.N = D * H * W;
    gd.H = (int)H;
    gd.W = (int)W;
    gd.nY = (unsigned)(H / 4);
    gd.nX = (unsigned)(W / 4);
    return gd;
}
// lanes per row of the row dots: the power of two >= the column chunks, at most `cap`
int cb_row_lanes(long nch, int cap) {
    int L = 1;
    while (L < nch && L < cap) L <<= 1;
    return L;
}
bool cb_map_supported(long B, long D, long H, long W) {
    return D < (1L << 24) && H < (1L << 24) && W < (1L << 24) && D * H * W < (1L << 36) && B < (1L << 20);
}
CbTiles cb_tiles(long D, long H, long W) {
    CbTiles tl;
    tl.D = (int)D; tl.H = (int)H; tl.W = (int)W;
    tl.ntt = (int)((D + kTT - 1) / kTT);
    tl.nty = (int)((H + kTY - 1) / kTY);
    tl.ntx = (int)((W + kTX - 1) / kTX);
    return tl;
}
long cb_ntiles(long B, const CbTiles& tl) { return B * tl.ntt * (long)tl.nty * tl.ntx; }
size_t cb_wgrad_bytes(long B, long D, long H, long W) {
    const long nt = cb_ntiles(B, cb_tiles(D, H, W));
    return ws_align((size_t)std::min(nt, kWgBlocks) * kWgPart * sizeof(float));
}

}  // namespace

namespace {

// the row entry points on fp32 (T = float) or bf16 rows
template <typename T>
int cbam_chan_mean_rows(const T* o, const float* gate, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C,
                        int64_t ld, float* map, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(o && gate && map && cb_rows_ok(B, D, H, W, C, ld));
    if (!cb_rows_supported(B, D, H, W, C)) return DLCS_ERR_UNSUPPORTED_SIZE;
    const CbGrid gd = cb_grid(D, H, W);
    const SeGeom q = se_geom(B, gd.N);
    const dim3 grid(q.G, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    const float scale = 1.0f / (float)C;
    if (se_vec<T>(C, ld, {o}))
        hipLaunchKernelGGL((cbam_rowdot_kernel<T, RowVec<T>::v, false>), grid, dim3(256), 0, st, o, nullptr, nullptr, gate,
                           scale, map, gd, (int)C, (long)ld, q.rpb, cb_row_lanes(C / RowVec<T>::v, 16));
    else
        hipLaunchKernelGGL((cbam_rowdot_kernel<T, 1, false>), grid, dim3(256), 0, st, o, nullptr, nullptr, gate, scale,
                           map, gd, (int)C, (long)ld, q.rpb, cb_row_lanes(C, 64));
    return dlcs_launch_status();
}

template <typename T>
int cbam_scale_res_relu_rows(const T* o, const float* gate, const float* q, const T* res, T* out, int64_t B,
                             int64_t D, int64_t H, int64_t W, int64_t C, int64_t ld, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(o && gate && q && res && out && out != o && cb_rows_ok(B, D, H, W, C, ld));
    if (!cb_rows_supported(B, D, H, W, C)) return DLCS_ERR_UNSUPPORTED_SIZE;
    const CbGrid gd = cb_grid(D, H, W);
    const SeGeom geo = se_geom(B, gd.N);
    const dim3 grid(geo.G, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (se_vec<T>(C, ld, {o, res, out}))
        hipLaunchKernelGGL((cbam_rows_kernel<T, RowVec<T>::v, false>), grid, dim3(256), 0, st, o, res, nullptr, gate, q,
                           nullptr, 0.0f, nullptr, out, gd, (int)C, (long)ld, geo.rpb);
    else
        hipLaunchKernelGGL((cbam_rows_kernel<T, 1, false>), grid, dim3(256), 0, st, o, res, nullptr, gate, q, nullptr, 0.0f,
                           nullptr, out, gd, (int)C, (long)ld, geo.rpb);
    return dlcs_launch_status();
}

template <typename T>
int cbam_bwd_rowdot_rows(const T* g, const T* r_next, const T* o, const float* gate, int64_t B, int64_t D,
                         int64_t H, int64_t W, int64_t C, int64_t ld, float* dq, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(g && r_next && o && gate && dq && cb_rows_ok(B, D, H, W, C, ld));
    if (!cb_rows_supported(B, D, H, W, C)) return DLCS_ERR_UNSUPPORTED_SIZE;
    const CbGrid gd = cb_grid(D, H, W);
    const SeGeom geo = se_geom(B, gd.N);
    const dim3 grid(geo.G, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (se_vec<T>(C, ld, {g, r_next, o}))
        hipLaunchKernelGGL((cbam_rowdot_kernel<T, RowVec<T>::v, true>), grid, dim3(256), 0, st, o, g, r_next, gate, 1.0f,
                           dq, gd, (int)C, (long)ld, geo.rpb, cb_row_lanes(C / RowVec<T>::v, 16));
    else
        hipLaunchKernelGGL((cbam_rowdot_kernel<T, 1, true>), grid, dim3(256), 0, st, o, g, r_next, gate, 1.0f, dq, gd,
                           (int)C, (long)ld, geo.rpb, cb_row_lanes(C, 64));
    return dlcs_launch_status();
}

template <typename T>
int cbam_bwd_reduce_rows(const T* g, const T* r_next, const T* o, const float* q, const float* da, int64_t B,
                         int64_t D, int64_t H, int64_t W, int64_t C, int64_t ld, float* dgate, void* workspace,
                         size_t workspace_bytes, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(g && r_next && o && q && da && dgate && cb_rows_ok(B, D, H, W, C, ld));
    if (!cb_rows_supported(B, D, H, W, C)) return DLCS_ERR_UNSUPPORTED_SIZE;
    const CbGrid gd = cb_grid(D, H, W);
    if (!ws_ok(workspace, workspace_bytes, se_partial_bytes(B, gd.N, C))) return DLCS_ERR_WORKSPACE;
    const SeGeom geo = se_geom(B, gd.N);
    const dim3 grid(geo.G, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    const float inv_c = 1.0f / (float)C;
    if (se_vec<T>(C, ld, {g, r_next, o}))
        hipLaunchKernelGGL((cbam_reduce_kernel<T, RowVec<T>::v>), grid, dim3(256), 0, st, o, g, r_next, q, da, inv_c, gd,
                           (int)C, (long)ld, geo.rpb, part);
    else
        hipLaunchKernelGGL((cbam_reduce_kernel<T, 1>), grid, dim3(256), 0, st, o, g, r_next, q, da, inv_c, gd, (int)C,
                           (long)ld, geo.rpb, part);
    hipLaunchKernelGGL(se_partial_sum_kernel, dim3(cdiv(C, kSeSumCols), (unsigned)B), dim3(1024), 0, st, part, (int)geo.G,
                       (int)C, 1.0f, dgate);
    return dlcs_launch_status();
}

template <typename T>
int cbam_bwd_apply_rows(T* g, const T* r_next, const float* gate, const float* q, const float* da,
                        const float* dmean, T* dout, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C, int64_t ld,
                        dlcs_stream_t stream) {
    DLCS_CHECK_ARG(g && r_next && gate && q && da && dmean && dout && dout != g && cb_rows_ok(B, D, H, W, C, ld));
    if (!cb_rows_supported(B, D, H, W, C)) return DLCS_ERR_UNSUPPORTED_SIZE;
    const CbGrid gd = cb_grid(D, H, W);
    const SeGeom geo = se_geom(B, gd.N);
    const dim3 grid(geo.G, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    const float inv_c = 1.0f / (float)C;
    if (se_vec<T>(C, ld, {g, r_next, dout}))
        hipLaunchKernelGGL((cbam_rows_kernel<T, RowVec<T>::v, true>), grid, dim3(256), 0, st, r_next, nullptr, g, gate, q,
                           da, inv_c, dmean, dout, gd, (int)C, (long)ld, geo.rpb);
    else
        hipLaunchKernelGGL((cbam_rows_kernel<T, 1, true>), grid, dim3(256), 0, st, r_next, nullptr, g, gate, q, da, inv_c,
                           dmean, dout, gd, (int)C, (long)ld, geo.rpb);
    return dlcs_launch_status();
}

}  // namespace

extern "C" {

int dlcs_cbam_chan_mean(const float* o, const float* gate, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C,
                        int64_t ld, float* map, dlcs_stream_t stream) {
    return cbam_chan_mean_rows<float>(o, gate, B, D, H, W, C, ld, map, stream);
}

int dlcs_cbam_chan_mean_bf16(const void* o, const float* gate, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C,
                             int64_t ld, float* map, dlcs_stream_t stream) {
    return cbam_chan_mean_rows<bf16>((const bf16*)o, gate, B, D, H, W, C, ld, map, stream);
}

int dlcs_cbam_stencil5(const float* in, const float* w5, const float* bias, int transposed, float* out, int64_t B,
                       int64_t D, int64_t H, int64_t W, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(in && w5 && out && out != in && (transposed || bias) && cb_dims_ok(B, D, H, W));
    if (!cb_map_supported(B, D, H, W)) return DLCS_ERR_UNSUPPORTED_SIZE;
    const CbTiles tl = cb_tiles(D, H, W);
    const long nt = cb_ntiles(B, tl);
    if (nt >= (1L << 31)) return DLCS_ERR_UNSUPPORTED_SIZE;
    if (transposed)
        hipLaunchKernelGGL(cbam_stencil_kernel<true>, dim3((unsigned)nt), dim3(256), 0, (hipStream_t)stream, in, w5, bias,
                           out, tl);
    else
        hipLaunchKernelGGL(cbam_stencil_kernel<false>, dim3((unsigned)nt), dim3(256), 0, (hipStream_t)stream, in, w5, bias,
                           out, tl);
    return dlcs_launch_status();
}

size_t dlcs_cbam_stencil5_wgrad_workspace_bytes(int64_t B, int64_t D, int64_t H, int64_t W) {
    return (cb_dims_ok(B, D, H, W) && cb_map_supported(B, D, H, W)) ? cb_wgrad_bytes(B, D, H, W) : 0;
}

int dlcs_cbam_stencil5_wgrad(const float* dq, const float* a, int64_t B, int64_t D, int64_t H, int64_t W, float* dw5,
                             float* db5, void* workspace, size_t workspace_bytes, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(dq && a && dw5 && db5 && cb_dims_ok(B, D, H, W));
    if (!cb_map_supported(B, D, H, W)) return DLCS_ERR_UNSUPPORTED_SIZE;
    if (!ws_ok(workspace, workspace_bytes, cb_wgrad_bytes(B, D, H, W))) return DLCS_ERR_WORKSPACE;
    const CbTiles tl = cb_tiles(D, H, W);
    const long nt = cb_ntiles(B, tl);
    const int G = (int)std::min(nt, kWgBlocks);
    float* part = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cbam_wgrad_kernel, dim3((unsigned)G), dim3(256), 0, st, dq, a, tl, nt, part);
    hipLaunchKernelGGL(cbam_wgrad_sum_kernel, dim3(kWgPart / kSeSumCols), dim3(1024), 0, st, part, G, dw5, db5);
    return dlcs_launch_status();
}

int dlcs_cbam_scale_res_relu(const float* o, const float* gate, const float* q, const float* res, float* out, int64_t B,
                             int64_t D, int64_t H, int64_t W, int64_t C, int64_t ld, dlcs_stream_t stream) {
    return cbam_scale_res_relu_rows<float>(o, gate, q, res, out, B, D, H, W, C, ld, stream);
}

int dlcs_cbam_scale_res_relu_bf16(const void* o, const float* gate, const float* q, const void* res, void* out, int64_t B,
                                  int64_t D, int64_t H, int64_t W, int64_t C, int64_t ld, dlcs_stream_t stream) {
    return cbam_scale_res_relu_rows<bf16>((const bf16*)o, gate, q, (const bf16*)res, (bf16*)out, B, D, H, W, C, ld, stream);
}

int dlcs_cbam_bwd_rowdot(const float* g, const float* r_next, const float* o, const float* gate, int64_t B, int64_t D,
                         int64_t H, int64_t W, int64_t C, int64_t ld, float* dq, dlcs_stream_t stream) {
    return cbam_bwd_rowdot_rows<float>(g, r_next, o, gate, B, D, H, W, C, ld, dq, stream);
}

int dlcs_cbam_bwd_rowdot_bf16(const void* g, const void* r_next, const void* o, const float* gate, int64_t B, int64_t D,
                              int64_t H, int64_t W, int64_t C, int64_t ld, float* dq, dlcs_stream_t stream) {
    return cbam_bwd_rowdot_rows<bf16>((const bf16*)g, (const bf16*)r_next, (const bf16*)o, gate, B, D, H, W, C, ld, dq,
                                      stream);
}

size_t dlcs_cbam_bwd_reduce_workspace_bytes(int64_t B, int64_t D, int64_t H, int64_t W, int64_t C) {
    return (cb_dims_ok(B, D, H, W) && C > 0 && cb_rows_supported(B, D, H, W, C)) ? se_partial_bytes(B, D * H * W, C) : 0;
}

int dlcs_cbam_bwd_reduce(const float* g, const float* r_next, const float* o, const float* q, const float* da, int64_t B,
                         int64_t D, int64_t H, int64_t W, int64_t C, int64_t ld, float* dgate, void* workspace,
                         size_t workspace_bytes, dlcs_stream_t stream) {
    return cbam_bwd_reduce_rows<float>(g, r_next, o, q, da, B, D, H, W, C, ld, dgate, workspace, workspace_bytes, stream);
}

int dlcs_cbam_bwd_reduce_bf16(const void* g, const void* r_next, const void* o, const float* q, const float* da, int64_t B,
                              int64_t D, int64_t H, int64_t W, int64_t C, int64_t ld, float* dgate, void* workspace,
                              size_t workspace_bytes, dlcs_stream_t stream) {
    return cbam_bwd_reduce_rows<bf16>((const bf16*)g, (const bf16*)r_next, (const bf16*)o, q, da, B, D, H, W, C, ld, dgate,
                                      workspace, workspace_bytes, stream);
}

int dlcs_cbam_bwd_apply(float* g, const float* r_next, const float* gate, const float* q, const float* da,
                        const float* dmean, float* dout, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C, int64_t ld,
                        dlcs_stream_t stream) {
    return cbam_bwd_apply_rows<float>(g, r_next, gate, q, da, dmean, dout, B, D, H, W, C, ld, stream);
}

int dlcs_cbam_bwd_apply_bf16(void* g, const void* r_next, const float* gate, const float* q, const float* da,
                             const float* dmean, void* dout, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C, int64_t ld,
                             dlcs_stream_t stream) {
    return cbam_bwd_apply_rows<bf16>((bf16*)g, (const bf16*)r_next, gate, q, da, dmean, (bf16*)dout, B, D, H, W, C, ld,
                                     stream);
}

}  // extern "C"
