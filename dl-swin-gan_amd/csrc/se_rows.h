// Shared by se.hip and cbam.hip: the row-pass geometry of the gate kernels (one thread per
// column chunk, rows strided by the row groups of a workgroup), the 16-B / scalar row
// accessors, and the fixed-order sum of per-workgroup partial rows.
#pragma once
#include <algorithm>
#include <initializer_list>

#include "dlcs_common.h"

namespace {

constexpr int kSeMaxC = 1024;
constexpr int kSeMaxR = 256;
constexpr long kSeBlocks = 2048;     // workgroups of a row pass (8 per CU)
constexpr long kSeMinRows = 64;      // rows per workgroup at least

template <int V> struct SeVec { float v[V]; };

// rows are touched through se_load / se_store only: fp32 rows 4 columns per 16-B access, bf16
// rows 8 (RowVec<T>::v), or one element; the values a kernel works on are always fp32
// (V = 8 on floats: the gate row in LDS beside bf16 rows, two 16-B accesses)
template <typename T> struct RowVec;
template <> struct RowVec<float> { static constexpr int v = 4; };
template <> struct RowVec<bf16> { static constexpr int v = 8; };

template <int V> DLCS_DEV SeVec<V> se_load(const float* p) {
    SeVec<V> r;
    if constexpr (V == 4 || V == 8) {
#pragma unroll
        for (int h = 0; h < V / 4; ++h) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(p + 4 * h);
            r.v[4 * h] = t[0]; r.v[4 * h + 1] = t[1]; r.v[4 * h + 2] = t[2]; r.v[4 * h + 3] = t[3];
        }
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int V> DLCS_DEV void se_store(float* p, const SeVec<V>& r) {
    if constexpr (V == 4) {
        f32x4 t;
        t[0] = r.v[0]; t[1] = r.v[1]; t[2] = r.v[2]; t[3] = r.v[3];
        *reinterpret_cast<f32x4*>(p) = t;
    } else {
        static_assert(V == 1, "fp32 rows: 4 columns or 1");
        *p = r.v[0];
    }
}
template <int V> DLCS_DEV SeVec<V> se_load(const bf16* p) {
    SeVec<V> r;
    if constexpr (V == 8) {
        const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
        for (int e = 0; e < 8; ++e) r.v[e] = (float)t[e];
    } else {
        static_assert(V == 1, "bf16 rows: 8 columns or 1");
        r.v[0] = (float)*p;
    }
    return r;
}
template <int V> DLCS_DEV void se_store(bf16* p, const SeVec<V>& r) {     // one rounding, to nearest even
    if constexpr (V == 8) {
        bf16x8 t;
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = (bf16)r.v[e];
        *reinterpret_cast<bf16x8*>(p) = t;
    } else {
        static_assert(V == 1, "bf16 rows: 8 columns or 1");
        *p = (bf16)r.v[0];
    }
}

// out[b, c] = (sum_g part[(b G + g) C + c]) / denom in a fixed order: workgroup = 16
// columns x 64 slices (blockIdx.y = b); slice s sums g = s, s + 64, ... into four
// interleaved accumulators (a short dependent chain: the G <= 2048 partial rows are
// read with many loads in flight), then the 64 slices are summed in ascending order.
constexpr int kSeSumCols = 16, kSeSumSlices = 64;
__global__ void __launch_bounds__(1024) se_partial_sum_kernel(const float* part, int G, int C, float denom, float* out) {
    __shared__ float sm[kSeSumSlices][kSeSumCols + 1];
    const int cl = threadIdx.x % kSeSumCols, sl = threadIdx.x / kSeSumCols;
    const int c = blockIdx.x * kSeSumCols + cl;
    const long b = blockIdx.y;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    if (c < C) {
        const float* src = part + b * G * C + c;
        int q = sl;
        for (; q + 3 * kSeSumSlices < G; q += 4 * kSeSumSlices) {
            a0 += src[(long)q * C];
            a1 += src[(long)(q + kSeSumSlices) * C];
            a2 += src[(long)(q + 2 * kSeSumSlices) * C];
            a3 += src[(long)(q + 3 * kSeSumSlices) * C];
        }
        for (; q < G; q += kSeSumSlices) a0 += src[(long)q * C];
    }
    sm[sl][cl] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (sl == 0 && c < C) {
        float t = 0.0f;
        for (int k = 0; k < kSeSumSlices; ++k) t += sm[k][cl];
        out[b * C + c] = t / denom;
    }
}

struct SeGeom {
    long rpb;       // rows per workgroup
    unsigned G;     // workgroups per batch item
};
SeGeom se_geom(long B, long N) {
    SeGeom q;
    q.rpb = std::max<long>(kSeMinRows, (N * B + kSeBlocks - 1) / kSeBlocks);
    q.G = (unsigned)((N + q.rpb - 1) / q.rpb);
    return q;
}
size_t se_partial_bytes(long B, long N, long C) { return ws_align((size_t)B * se_geom(B, N).G * (size_t)C * sizeof(float)); }
bool se_rows_ok(long B, long N, long C, long ld) { return B > 0 && N > 0 && C > 0 && ld >= C; }
bool se_rows_supported(long B, long C) { return C <= kSeMaxC && B <= 65535; }
template <typename T = float>
bool se_vec(long C, long ld, std::initializer_list<const void*> ptrs) {
    if (C % RowVec<T>::v || ld % RowVec<T>::v) return false;
    for (const void* p : ptrs)
        if (!al16(p)) return false;
    return true;
}

}  // namespace
