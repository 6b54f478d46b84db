// The 2-plane f16 split of fp32 tensors (numerics: conv3d_f16x3.inc's header): what
// planes_f16x3.hip, conv3d_f16x3.hip and gemm_f16x3.hip share.
#pragma once
#include "lds_dma.h"

// planes_f16x3.hip's kernels that the other units launch (a kernel is compiled in one
// unit only): colsum[c] += sum of nblk rows of cpart; *out = max(*out, max |x| bits)
namespace dlcs_internal {
__attribute__((visibility("hidden"))) int launch_colsum_parts(const float* cpart, int nblk, float* colsum, hipStream_t st);
__attribute__((visibility("hidden"))) int launch_absmax_flat(const float* x, long n, unsigned* out, unsigned grid, hipStream_t st);
}  // namespace dlcs_internal

namespace {
typedef _Float16 f16;
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_h3 __attribute__((ext_vector_type(4)));

DLCS_DEV void mfma16h(f32x4_t& acc, const f16x8_t& a, const f16x8_t& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
}

// the power-of-two scale of a tensor from the bits of max|x| (conv3d_f16x3.inc's header)
DLCS_DEV float f16x3_scale(unsigned maxbits) {
    const float m = __uint_as_float(maxbits);
    if (!(m > 0.0f) || !(m < 3.0e38f)) return 1.0f;
    int e;
    const float f = frexpf(m, &e);                  // m = f 2^e, f in [0.5, 1)
    int k = 14 - (f == 0.5f ? e - 1 : e);           // 14 - ceil(log2 m)
    k = k < -100 ? -100 : (k > 100 ? 100 : k);
    return ldexpf(1.0f, k);
}

// hi / lo planes of the 8 (4) consecutive channels c.. of row r of a split2 image
// (split2_f16_kernel's layout: per 32-channel chunk the high plane, then the low);
// the low plane of u = s x given its high plane; a nonzero u whose planes would both
// round to zero (|u| < 2^-25) keeps its sign in the smallest subnormal, so "x != 0"
// (a ReLU mask read from the planes of a non-negative tensor) survives the split
DLCS_DEV f16 plane_lo(float u, f16 h) {
    f16 l = (f16)(u - (float)h);
    if (u != 0.0f && h == (f16)0.0f && l == (f16)0.0f) l = u > 0.0f ? (f16)5.9604645e-8f : (f16)-5.9604645e-8f;
    return l;
}
DLCS_DEV void put_planes8(f16* xp, long r, int c, const f32x4_t& v0, const f32x4_t& v1, float s) {
    f16x8_t h, l;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float u = (e < 4 ? v0[e] : v1[e - 4]) * s;
        h[e] = (f16)u;
        l[e] = plane_lo(u, h[e]);
    }
    f16* d = xp + r * 320 + (c >> 5) * 64 + (c & 31);
    *reinterpret_cast<f16x8_t*>(d) = h;
    *reinterpret_cast<f16x8_t*>(d + 32) = l;
}
DLCS_DEV void put_planes4(f16* xp, long r, int c, const f32x4_t& v, float s) {
    f16x4_t h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float u = v[e] * s;
        h[e] = (f16)u;
        l[e] = plane_lo(u, h[e]);
    }
    f16* d = xp + r * 320 + (c >> 5) * 64 + (c & 31);
    *reinterpret_cast<f16x4_t*>(d) = h;
    *reinterpret_cast<f16x4_t*>(d + 32) = l;
}

// (hi + lo) / s of 4 channels c.. of row r of a split2 image (rinv = 1 / s): the
// value to 2^-22 relative (+ 2^-38 of the image's bound), hi + lo exact in fp32
DLCS_DEV f32x4_t get_planes4(const f16* xp, long r, int c, float rinv) {
    const f16* d = xp + r * 320 + (c >> 5) * 64 + (c & 31);
    const f16x4_t h = *reinterpret_cast<const f16x4_t*>(d), l = *reinterpret_cast<const f16x4_t*>(d + 32);
    f32x4_t v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ((float)h[e] + (float)l[e]) * rinv;
    return v;
}

// max |.| of a workgroup into *omax (float bits): one wave reduction, one LDS
// slot per wave, and one atomicMax per workgroup -- skipped when the word
// already holds at least this value (a plain read; the word only grows, so a
// stale read can only cause a redundant atomic).  Thousands of workgroups
// hammering one address with per-wave atomics cost ~0.5 ms per launch.
// Every thread of the workgroup must call it (it holds a barrier).
DLCS_DEV void block_max_to(unsigned* omax, float v, float* red) {
    v = wave_max(v);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = red[0];
        for (int i = 1; i < nw; ++i) m = fmaxf(m, red[i]);
        if (m > 0.0f && m > __uint_as_float(__atomic_load_n(omax, __ATOMIC_RELAXED)))
            atomicMax(omax, __float_as_uint(m));
    }
}

DLCS_DEV int f16x3_halo_swz(int hy, int hx) { return 2 * (hy & 3) + ((hx >> 1) & 1); }
static unsigned h3_grid(long n) { return (unsigned)std::min<long>((n + 255) / 256, 8192); }
// byte offset of the zero row of a split2 buffer of `rows` rows (dlcs_split2_f16_bytes)
DLCS_DEV long h3_zero_row_byte(long rows) { return rows * 640 + 256; }
constexpr size_t kW3Bytes = (size_t)5 * 27 * 160 * 64 * 2;   // the packed 160 x 160 conv weight planes [5][27][160][64] f16
// column-sum partials of a producer that also sums its output's columns: 160 per tile
static size_t colsum_part_bytes(long nwg, bool colsum) { return colsum ? (size_t)nwg * 160 * sizeof(float) : 0; }

}  // namespace
