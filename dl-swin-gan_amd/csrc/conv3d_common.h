// What conv3d.hip and conv3d_f16x3.hip share: tile and workspace arithmetic, the row
// index, the argument structs, the epilogue codes and the fp32 tile epilogue.
#pragma once
#include "lds_dma.h"

namespace {
// 4 x 8 x 8 output tiles (1 x 2 x 2 patches) of the 160-channel conv kernels
inline long conv_tiles(long B, long D, long H, long W) { return B * (D / 4) * ((H / 4 + 1) / 2) * ((W / 4 + 1) / 2); }
// tiles of the last partial round of 256 workgroups that run as 5 single-chunk
// workgroups each (the tail split of the f16x3, v6 and v7 kernels), 0 = no split
inline unsigned conv_tail_tiles(long ntile) {
    const long ntail = ntile % 256;
    return ntile > ntail && ntail > 0 && ntail * 5 <= 256 ? (unsigned)ntail : 0u;
}
// the tail split's partial tiles: [ntail][5][256][160] floats (v7: twice the units of 80 channels)
inline size_t conv_tail_bytes(long ntile) { return (size_t)conv_tail_tiles(ntile) * 5 * 256 * 160 * sizeof(float); }

// a weight gradient's voxel ranges: nr non-empty ranges of pp patches, nr <= want
struct PatchRanges { int nr; long pp; };
inline PatchRanges patch_ranges(long npatch, long want) {
    const long n0 = std::max<long>(1, std::min<long>(want, npatch));
    const long pp = (npatch + n0 - 1) / n0;
    return {(int)((npatch + pp - 1) / std::max<long>(1, pp)), pp};
}
constexpr size_t kWgSlabBytes = (size_t)27 * 160 * 160 * sizeof(float);         // one range's dW partial

constexpr int kHaloT = 6, kHaloY = 10, kHaloX = 10;
constexpr int kHalo = kHaloT * kHaloY * kHaloX;     // 600 voxels
constexpr int CK = 32;                              // channel chunk (K per tap step)

DLCS_DEV long brow(int b, int t, int y, int x, int nT, int nY, int nX) {
    const long patch = (((long)b * nT + (t >> 2)) * nY + (y >> 2)) * nX + (x >> 2);
    return patch * 64 + ((t & 3) << 4) + ((y & 3) << 2) + (x & 3);
}

struct ConvArgs {
    const void* in; const void* w; const float* bias; void* out;
    const void* mask; const void* res;
    int B, D, H, W, Cin, cin_ld, cin_pad, Cout, cout_pad, cout_ld;
    int mask_ld, res_ld, relu_in, out_f32, res_f32, accumulate, relu_out;
    float res_scale;
};

struct ConvV2Args {
    const bf16* in; const bf16* w; const float* bias; void* out;
    const bf16* mask; const void* res;
    int B, D, H, W, cin_ld, cin_pad;
    int cout_ld, mask_ld, res_ld, out_f32, res_f32, accumulate, relu_out;
    float res_scale;
    int xcd_major;          // v5: number tiles XCD-major (neighbouring halos in one L2)
};

struct WgradArgs {
    const void* in; const void* g; float* dw;
    int B, D, H, W, Cin, cin_ld, cin_pad, Cout, g_ld, cout_pad, relu_in;
    long vox_per_block;
    float* dbias;           // optional: += column sums of g (the conv bias gradient)
};

enum { kEpiRes = 1, kEpiResF32 = 2, kEpiMask = 4, kEpiAcc = 8, kEpiOutF32 = 16, kEpiGeneric = 32 };

template <int EPI>
struct EpiFlags {
    const ConvV2Args& a;
    DLCS_DEV bool res() const { return (EPI & kEpiGeneric) ? a.res != nullptr : (EPI & kEpiRes); }
    DLCS_DEV bool res_f32() const { return (EPI & kEpiGeneric) ? a.res_f32 != 0 : (EPI & kEpiResF32); }
    DLCS_DEV bool mask() const { return (EPI & kEpiGeneric) ? a.mask != nullptr : (EPI & kEpiMask); }
    DLCS_DEV bool accum() const { return (EPI & kEpiGeneric) ? a.accumulate != 0 : (EPI & kEpiAcc); }
    DLCS_DEV bool out_f32() const { return (EPI & kEpiGeneric) ? a.out_f32 != 0 : (EPI & kEpiOutF32); }
};
// The epilogue instance of a launch: a fused form (0: bias only; kEpiRes: + residual, if the
// launch can take that form; kEpiMask: + ReLU mask) for a plainly written output, else generic.
inline int conv_epi_code(bool res, bool mask, bool plain_out, bool res_form_ok) {
    if (plain_out && !res && !mask) return 0;
    if (plain_out && res && !mask && res_form_ok) return kEpiRes;
    if (plain_out && !res && mask) return kEpiMask;
    return kEpiGeneric;
}

struct ConvF32Args {
    const float* in; const float* w; const float* bias; float* out;
    const float* mask; const float* res;
    int B, D, H, W, cin_ld, cin_pad;
    int cout_ld, mask_ld, res_ld, accumulate, relu_out;
    float res_scale;
    int cout, cout_pad;
    unsigned* omax;         // optional: max |out| as float bits (atomicMax) for the next f16 split
    const void* mplanes;    // the f16x3 fused epilogue: the ReLU mask as the split2 planes of a non-negative tensor
};

// epilogue of the 256 x 160 tile (acc[4][5] per wave, rows = voxels), staged
// through LDS in two 80-channel passes, 16-B accesses throughout (s3d:256-259,
// :339-340, :368, :427).  The main loop is 90 barrier steps long, so the
// epilogue's operand loads are simply issued after the LDS round trip (no
// register prefetch: it would spill beside the 80 accumulators).
template <int EPI, int NPASS = 2>
DLCS_DEV void conv_epilogue_f32(const ConvF32Args& a, const f32x4_t (&acc)[4][5], float* Es, int pw, int cw0,
                                int lane, int b, int pt, int pyq, int pxq, int nT, int nY, int nX) {
    constexpr int PC = 160 / NPASS, EL = PC + 4, NCH = PC / 8, PER = 256 * NCH / 512;
    static_assert(256 * NCH % 512 == 0, "whole 8-channel chunks per thread");
    const bool has_res = (EPI & kEpiGeneric) ? a.res != nullptr : (EPI & kEpiRes);
    const bool has_mask = (EPI & kEpiGeneric) ? a.mask != nullptr : (EPI & kEpiMask);
    const bool accum = (EPI & kEpiGeneric) ? a.accumulate != 0 : (EPI & kEpiAcc);
    float vmax = 0.0f;
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int c0 = cw0 + j * 16 - pass * PC;
            if (c0 + 16 <= 0 || c0 >= PC) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int vl = pw * 64 + i * 16 + (lane >> 4) * 4 + r;
                    const int cl = c0 + (lane & 15);
                    if (cl >= 0 && cl < PC) Es[vl * EL + cl] = acc[i][j][r];
                }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int c = threadIdx.x + k * 512;
            const int vl = c / NCH, ch = (c % NCH) * 8;
            const int pwv = vl >> 6;
            const int py = pyq + (pwv >> 1), px = pxq + (pwv & 1);
            if (py >= nY || px >= nX) continue;
            const long orow = ((((long)b * nT + pt) * nY + py) * nX + px) * 64 + (vl & 63);
            const int co = pass * PC + ch;
            f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(Es + vl * EL + ch);
            f32x4_t v1 = *reinterpret_cast<const f32x4_t*>(Es + vl * EL + ch + 4);
            if (a.bias) {
                v0 += *reinterpret_cast<const f32x4_t*>(a.bias + co);
                v1 += *reinterpret_cast<const f32x4_t*>(a.bias + co + 4);
            }
            if (has_mask) {
                const float* mp = a.mask + orow * a.mask_ld + co;
                const f32x4_t m0 = *reinterpret_cast<const f32x4_t*>(mp);
                const f32x4_t m1 = *reinterpret_cast<const f32x4_t*>(mp + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v0[e] = m0[e] > 0.0f ? v0[e] : 0.0f;
                    v1[e] = m1[e] > 0.0f ? v1[e] : 0.0f;
                }
            }
            if (has_res) {
                const float* rp = a.res + orow * a.res_ld + co;
                v0 += a.res_scale * *reinterpret_cast<const f32x4_t*>(rp);
                v1 += a.res_scale * *reinterpret_cast<const f32x4_t*>(rp + 4);
            }
            if (a.relu_out) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { v0[e] = fmaxf(v0[e], 0.0f); v1[e] = fmaxf(v1[e], 0.0f); }
            }
            float* o = a.out + orow * a.cout_ld + co;
            if (accum) {
                v0 += *reinterpret_cast<const f32x4_t*>(o);
                v1 += *reinterpret_cast<const f32x4_t*>(o + 4);
            }
            *reinterpret_cast<f32x4_t*>(o) = v0;
            *reinterpret_cast<f32x4_t*>(o + 4) = v1;
            if (a.omax) {
#pragma unroll
                for (int e = 0; e < 4; ++e) vmax = fmaxf(vmax, fmaxf(fabsf(v0[e]), fabsf(v1[e])));
            }
        }
        __syncthreads();
    }
    if (a.omax) {
        vmax = wave_max(vmax);
        // one atomic per wave, skipped unless it raises the max (see block_max_to in f16x3_common.h)
        if ((threadIdx.x & 63) == 0 && vmax > 0.0f && vmax > __uint_as_float(__atomic_load_n(a.omax, __ATOMIC_RELAXED)))
            atomicMax(a.omax, __float_as_uint(vmax));
    }
}

}  // namespace
