// The fp32 Conv3d(k=3, s=1, p=1) kernels on the fp16 matrix cores (2-plane split,
// conv3d_f16x3.inc): 160 -> 160 forward / dgrad / wgrad from plane buffers (planes_f16x3.hip),
// the thin ends from fp32 rows (conv3d_thin_f16x3.inc) or planes (conv3d_thin_planes.inc).
#include "conv3d_common.h"
#include "f16x3_common.h"
#include "wgrad_live.h"
#include <type_traits>

namespace {
__device__ uint4 g_wg_zero_row[160 / 8];   // this unit's zero source row (halo voxels off the grid)
// ---- shared by the .inc files below (none depends on another): the thin ends' packed weight
// images (f16 counts; the float s_w follows the planes), the transposed f16 read, the fused epilogue
constexpr int kThinInHalfs = 2 * 4 * 4 * 160 * 8;      // [plane][ks 4][kg 4][co 160][8]
constexpr int kThinOutHalfs = 5 * 9 * 2 * 4 * 16 * 8;  // [cc 5][kk 9][plane][kg 4][n 16][8]
constexpr int kThinOutW2 = 5 * 9 * 2 * 4 * 12 * 8;    // f16 of the LDS weight image

DLCS_DEV f16x8_t tr_read16h(const f16* p0, const f16* p1) {
    return __builtin_bit_cast(f16x8_t, tr_read16(reinterpret_cast<const bf16*>(p0), reinterpret_cast<const bf16*>(p1)));
}

// Epilogue of the f16x3 conv for the two fused forms (EPI = kEpiRes: bias +
// res_scale residual [+ ReLU-out, out_max]; EPI = kEpiMask: bias + ReLU mask
// [+ out_max]): conv_epilogue_f32's two 80-channel LDS passes, with the residual
// or mask of BOTH passes loaded into registers before the accumulators are staged,
// so their HBM latency overlaps the LDS round trips instead of following them
// (DIAG stamps: the epilogue was 28.6 k of a tile's 197 k cycles; 80 VGPRs of
// prefetch beside the 80 accumulators once the main loop's registers are dead).
// PREF = false (a caller short of registers): each pass's operands loaded in that pass.
template <int EPI, int NPASS, bool PREF = true>
DLCS_DEV void conv_epilogue_h3(const ConvF32Args& a, const f32x4_t (&acc)[4][5], float* Es, int pw, int cw0,
                               int lane, int b, int pt, int pyq, int pxq, int nT, int nY, int nX,
                               f16* op, const unsigned* opmax, float* cpart) {
    const float ps = op ? f16x3_scale(*opmax) : 1.0f;
    static_assert(EPI == kEpiRes || EPI == kEpiMask, "fused forms only");
    constexpr int PC = 160 / NPASS, EL = PC + 4, NCH = PC / 8, PER = 256 * NCH / 512;
    static_assert(PC % 8 == 0 && 256 * NCH % 512 == 0 && PC <= 512, "whole 8-channel chunks per thread");
    const float* src = EPI == kEpiRes ? a.res : a.mask;
    const int sld = EPI == kEpiRes ? a.res_ld : a.mask_ld;
    // kEpiMask with a.mplanes: the mask tensor's planes (hi | lo != 0 <=> x > 0 for x >= 0)
    const f16* mp = EPI == kEpiMask ? reinterpret_cast<const f16*>(a.mplanes) : nullptr;
    f32x4_t pre[PREF ? NPASS : 1][PER][2];
    long orows[PER];
    bool oks[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = threadIdx.x + k * 512;
        const int vl = c / NCH;
        const int pwv = vl >> 6;
        const int py = pyq + (pwv >> 1), px = pxq + (pwv & 1);
        oks[k] = py < nY && px < nX;
        orows[k] = ((((long)b * nT + pt) * nY + min(py, nY - 1)) * nX + min(px, nX - 1)) * 64 + (vl & 63);
    }
    auto load_pre = [&](int pass, int slot) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int c = threadIdx.x + k * 512;
            const int co = pass * PC + (c % NCH) * 8;
            if (mp) {                                       // the raw hi / lo planes, tested at use
                const f16* q = mp + orows[k] * 320 + (co >> 5) * 64 + (co & 31);
                pre[slot][k][0] = *reinterpret_cast<const f32x4_t*>(q);
                pre[slot][k][1] = *reinterpret_cast<const f32x4_t*>(q + 32);
            } else {
                const float* sp = src + orows[k] * sld + co;
                pre[slot][k][0] = *reinterpret_cast<const f32x4_t*>(sp);
                pre[slot][k][1] = *reinterpret_cast<const f32x4_t*>(sp + 4);
            }
        }
    };
    if constexpr (PREF) {
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) load_pre(pass, pass);
    }
    float vmax = 0.0f;
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
        const int ps_ = PREF ? pass : 0;                  // this pass's operand slot
        if constexpr (!PREF) load_pre(pass, 0);
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
            const int co = pass * PC + ch;
            if (!oks[k]) {
                if (cpart) {                                // rows off the grid add nothing
                    *reinterpret_cast<f32x4_t*>(Es + vl * EL + ch) = (f32x4_t)0.0f;
                    *reinterpret_cast<f32x4_t*>(Es + vl * EL + ch + 4) = (f32x4_t)0.0f;
                }
                continue;
            }
            f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(Es + vl * EL + ch);
            f32x4_t v1 = *reinterpret_cast<const f32x4_t*>(Es + vl * EL + ch + 4);
            if (a.bias) {
                v0 += *reinterpret_cast<const f32x4_t*>(a.bias + co);
                v1 += *reinterpret_cast<const f32x4_t*>(a.bias + co + 4);
            }
            if (EPI == kEpiMask && mp) {
                // channel e of the 8: half e of the hi and lo f16x8 (dword e / 2)
                const u32x4_h3 hb = __builtin_bit_cast(u32x4_h3, pre[ps_][k][0]);
                const u32x4_h3 lb = __builtin_bit_cast(u32x4_h3, pre[ps_][k][1]);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const unsigned nz = ((hb[e >> 1] | lb[e >> 1]) >> (16 * (e & 1))) & 0x7fffu;   // -0 is zero
                    if (e < 4) v0[e] = nz ? v0[e] : 0.0f;
                    else v1[e - 4] = nz ? v1[e - 4] : 0.0f;
                }
            } else if (EPI == kEpiMask) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v0[e] = pre[ps_][k][0][e] > 0.0f ? v0[e] : 0.0f;
                    v1[e] = pre[ps_][k][1][e] > 0.0f ? v1[e] : 0.0f;
                }
            } else {
                v0 += a.res_scale * pre[ps_][k][0];
                v1 += a.res_scale * pre[ps_][k][1];
            }
            if (a.relu_out) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { v0[e] = fmaxf(v0[e], 0.0f); v1[e] = fmaxf(v1[e], 0.0f); }
            }
            if (a.out) {                                    // (planes-only output: no fp32 tensor)
                float* o = a.out + orows[k] * a.cout_ld + co;
                *reinterpret_cast<f32x4_t*>(o) = v0;
                *reinterpret_cast<f32x4_t*>(o + 4) = v1;
            }
            if (op) put_planes8(op, orows[k], co, v0, v1, ps);
            if (cpart) {                                    // the final values back into this item's own slot
                *reinterpret_cast<f32x4_t*>(Es + vl * EL + ch) = v0;
                *reinterpret_cast<f32x4_t*>(Es + vl * EL + ch + 4) = v1;
            }
            if (a.omax) {
#pragma unroll
                for (int e = 0; e < 4; ++e) vmax = fmaxf(vmax, fmaxf(fabsf(v0[e]), fabsf(v1[e])));
            }
        }
        if (cpart) {                                        // the tile's column sums of this pass, fixed order
            constexpr int G = 512 / PC;                     // row groups: 6 (PC 80) or 16 (PC 32)
            __syncthreads();
            float* red = Es + 256 * EL;                     // [G][PC], past the staged tile
            const int t = threadIdx.x;
            if (t < G * PC) {
                const int cc = t % PC, g = t / PC;
                float cs = 0.0f;
                for (int r = g; r < 256; r += G) cs += Es[r * EL + cc];
                red[g * PC + cc] = cs;
            }
            __syncthreads();
            if (t < PC) {
                float cs = 0.0f;
#pragma unroll
                for (int g = 0; g < G; ++g) cs += red[g * PC + t];
                cpart[pass * PC + t] = cs;
            }
        }
        __syncthreads();
    }
    if (a.omax) {
        vmax = wave_max(vmax);
        if ((threadIdx.x & 63) == 0 && vmax > 0.0f && vmax > __uint_as_float(__atomic_load_n(a.omax, __ATOMIC_RELAXED)))
            atomicMax(a.omax, __float_as_uint(vmax));
    }
}

#include "conv3d_f16x3.inc"
#include "conv3d_thin_f16x3.inc"
#include "conv3d_thin_planes.inc"

}  // namespace

using namespace dlcs_internal;

extern "C" {

#ifdef DLCS_DIAG_BUILD
int dlcs_debug_h3_stamps(void* host, int64_t n) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_h3_stamps), (size_t)n * 8, 0, hipMemcpyDeviceToHost);
}
#endif

// the column-sum partials, then (at a 256-B offset) the tail split's partial tiles
size_t dlcs_conv3d_k3_f16x3_workspace_bytes(int64_t B, int64_t D, int64_t H, int64_t W, int has_colsum) {
    const long ntile = conv_tiles(B, D, H, W);
    return ws_align(colsum_part_bytes(ntile, has_colsum != 0)) + conv_tail_bytes(ntile);
}

int dlcs_conv3d_k3_f16x3(const void* xplanes, const void* wpacked, const float* bias, float* out, int64_t cout_ld,
                         int64_t B, int64_t D, int64_t H, int64_t W, const float* mask, int64_t mask_ld,
                         const float* residual, int64_t res_ld, float res_scale, int accumulate, int relu_out,
                         unsigned* out_max, void* out_planes, float* colsum, const void* mask_planes,
                         void* workspace, size_t workspace_bytes, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(xplanes && wpacked && B > 0 && (out || (out_planes && !accumulate)) && !(mask && mask_planes));
    if (!out) cout_ld = 160;
    const long rows = (long)B * D * H * W;
    if (D % 4 || H % 4 || W % 4 || cout_ld % 4 || !al16(xplanes) || !al16(wpacked) || !al16(out) ||
        (mask && (mask_ld % 4 || !al16(mask))) || (residual && (res_ld % 4 || !al16(residual))) || (bias && !al16(bias)) ||
        rows * 320 >= (1L << 31))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    ConvH3Args v{};
    v.xp = (const f16*)xplanes; v.wp = (const f16*)wpacked;
    v.xmax = planes_trailer(xplanes, rows); v.wmax = (const unsigned*)((const char*)wpacked + kW3Bytes);
    v.bias = bias; v.out = out; v.mask = mask; v.res = residual;
    v.B = (int)B; v.D = (int)D; v.H = (int)H; v.W = (int)W;
    v.cout_ld = (int)cout_ld; v.mask_ld = (int)mask_ld; v.res_ld = (int)res_ld; v.accumulate = accumulate;
    v.relu_out = relu_out; v.res_scale = res_scale; v.omax = out_max;
    if (mask_planes && !al16(mask_planes)) return DLCS_ERR_UNSUPPORTED_SIZE;
    v.mplanes = mask_planes;
    if (out_planes) {
        if (cout_ld != 160 || !al16(out_planes)) return DLCS_ERR_UNSUPPORTED_SIZE;
        v.oplanes = (f16*)out_planes; v.opmax = planes_trailer(out_planes, rows);
    }
#ifdef DLCS_DIAG_BUILD
    static const int stamps = [] { const char* e = dlcs_knob("DLCS_CONV_STAMP"); return e && e[0] == '1'; }();
    v.stamp = stamps;
    static const int h3_exp = [] { const char* e = dlcs_knob("DLCS_H3_EXP"); return e ? atoi(e) : 0; }();
    v.exp = h3_exp;
#endif
    hipStream_t st = (hipStream_t)stream;
    const long ntile = conv_tiles(B, D, H, W);
    if (!ws_ok(workspace, workspace_bytes, dlcs_conv3d_k3_f16x3_workspace_bytes(B, D, H, W, colsum != nullptr)))
        return DLCS_ERR_WORKSPACE;
    if (colsum) v.cpart = static_cast<float*>(workspace);     // one row of 160 per tile
    float* tail_ws = reinterpret_cast<float*>(static_cast<char*>(workspace) +
                                              ws_align(colsum_part_bytes(ntile, colsum != nullptr)));
    const int rc = conv_f16x3_launch(v, tail_ws, st);
    if (rc || !colsum) return rc;
    return launch_colsum_parts(v.cpart, (int)ntile, colsum, st);
}

size_t dlcs_conv3d_k3_wgrad_f16x3_workspace_bytes(int64_t B, int64_t D, int64_t H, int64_t W) {
    return (size_t)wgh3_ranges(B * (D / 4) * (H / 4) * (W / 4), true).nr * kWgSlabBytes;
}

int dlcs_conv3d_k3_wgrad_f16x3(const void* xplanes, const void* gplanes, float* dw_packed, int64_t B, int64_t D,
                               int64_t H, int64_t W, void* workspace, size_t workspace_bytes,
                               dlcs_stream_t stream) {
    return dlcs_conv3d_k3_wgrad_f16x3_live(xplanes, gplanes, dw_packed, B, D, H, W, 0, D, workspace, workspace_bytes,
                                           stream);
}

int dlcs_conv3d_k3_wgrad_f16x3_live(const void* xplanes, const void* gplanes, float* dw_packed, int64_t B, int64_t D,
                                    int64_t H, int64_t W, int64_t t_lo, int64_t t_hi, void* workspace,
                                    size_t workspace_bytes, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(xplanes && gplanes && dw_packed && B > 0);
    const long rows = (long)B * D * H * W;
    if (D % 4 || H % 4 || W % 4 || !al16(xplanes) || !al16(gplanes) || rows * 320 >= (1L << 40))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    WgradH3Args v{};
    v.xp = (const f16*)xplanes; v.gp = (const f16*)gplanes;
    v.xmax = planes_trailer(xplanes, rows); v.gmax = planes_trailer(gplanes, rows);
    v.dw = dw_packed; v.B = (int)B; v.D = (int)D; v.H = (int)H; v.W = (int)W;
    if (!ws_ok(workspace, workspace_bytes, dlcs_conv3d_k3_wgrad_f16x3_workspace_bytes(B, D, H, W)))
        return DLCS_ERR_WORKSPACE;
    v.part = static_cast<float*>(workspace);
    const int lo = (int)std::max<int64_t>(0, std::min<int64_t>(t_lo, D));
    const int hi = (int)std::max<int64_t>(0, std::min<int64_t>(t_hi, D));
    return wgrad_f16x3_launch(v, lo, hi, (hipStream_t)stream);
}

size_t dlcs_conv3d_thin_pack_f16x3_bytes(int kind) {
    return (size_t)(kind == 0 ? kThinInHalfs : kThinOutHalfs) * 2 + 256;
}

int dlcs_conv3d_thin_pack_f16x3(const float* wpacked, int64_t cout, int64_t cout_pad, int64_t cin, int64_t cin_pad,
                                int kind, void* out, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(wpacked && out && (kind == 0 || kind == 1) && cout <= cout_pad && cin <= cin_pad);
    if (kind == 0 ? !(cout == 160 && cout_pad == 160 && cin >= 1 && cin <= 4)
                  : !(cin == 160 && cin_pad == 160 && cout >= 1 && cout <= 4))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    if ((uintptr_t)out & 15) return DLCS_ERR_UNSUPPORTED_SIZE;
    hipStream_t st = (hipStream_t)stream;
    const int halfs = kind == 0 ? kThinInHalfs : kThinOutHalfs;
    // max |w| word past the scale float (the buffer has 256 B of trailer)
    unsigned* mx = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(out) + (size_t)halfs * 2 + 16);
    if (hipMemsetAsync(mx, 0, 4, st) != hipSuccess) return dlcs_launch_status();
    const long n = 27L * cout_pad * cin_pad;
    const int rc = launch_absmax_flat(wpacked, n, mx, (unsigned)std::min<long>(64, (n / 4 + 255) / 256), st);
    if (rc) return rc;
    hipLaunchKernelGGL(pack_thin_f16x3_grid_kernel, dim3((unsigned)((halfs / 2 + 255) / 256)), dim3(256), 0, st,
                       wpacked, (int)cout, (int)cout_pad, (int)cin, (int)cin_pad, kind, (const unsigned*)mx, (f16*)out);
    return dlcs_launch_status();
}

size_t dlcs_conv3d_thin_f16x3_workspace_bytes(int64_t B, int64_t D, int64_t H, int64_t W, int has_colsum) {
    return colsum_part_bytes(conv_tiles(B, D, H, W), has_colsum != 0);
}

int dlcs_conv3d_thin_f16x3(const float* in, int64_t cin, int64_t cin_ld, const unsigned* in_max, const void* wthin,
                           const float* bias, float* out, int64_t cout, int64_t cout_ld, int64_t B, int64_t D,
                           int64_t H, int64_t W, const float* mask, int64_t mask_ld, const float* residual,
                           int64_t res_ld, float res_scale, int accumulate, int relu_out, unsigned* out_max,
                           void* out_planes, float* colsum, const void* mask_planes, void* workspace,
                           size_t workspace_bytes, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(in && in_max && wthin && B > 0 && (out || out_planes) && !(mask && mask_planes));
    if (!out) cout_ld = 160;
    const long rows = (long)B * D * H * W;
    if (D % 4 || H % 4 || W % 4 || cin_ld % 4 || cout_ld % 4 || !al16(in) || !al16(out) || !al16(wthin) ||
        (bias && !al16(bias)) || rows * std::max(cin_ld, cout_ld) >= (1L << 31) || rows / 64 >= (1L << 24))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    const bool thin_in = cin >= 1 && cin <= 4 && cout == 160;
    const bool thin_out = cin == 160 && cout >= 1 && cout <= 4;
    if (!thin_in && !thin_out) return DLCS_ERR_UNSUPPORTED_SIZE;
    if (thin_in && ((mask && (mask_ld % 4 || !al16(mask))) || (residual && (res_ld % 4 || !al16(residual)))))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    if (thin_out && (mask || residual || out_max || cout_ld < 4)) return DLCS_ERR_UNSUPPORTED_SIZE;
    ConvF32Args v{};
    v.in = in; v.bias = bias; v.out = out; v.mask = mask; v.res = residual;
    v.B = (int)B; v.D = (int)D; v.H = (int)H; v.W = (int)W; v.cin_ld = (int)cin_ld; v.cin_pad = (int)cin;
    v.cout_ld = (int)cout_ld; v.mask_ld = (int)mask_ld; v.res_ld = (int)res_ld; v.accumulate = accumulate;
    v.relu_out = relu_out; v.res_scale = res_scale; v.cout = (int)cout; v.cout_pad = (int)cout; v.omax = out_max;
    v.mplanes = mask_planes;
    hipStream_t st = (hipStream_t)stream;
    if (!thin_in && (out_planes || colsum || mask_planes || !out)) return DLCS_ERR_UNSUPPORTED_SIZE;
    if (mask_planes && !al16(mask_planes)) return DLCS_ERR_UNSUPPORTED_SIZE;
    if (out_planes && (!al16(out_planes) || cout_ld != 160)) return DLCS_ERR_UNSUPPORTED_SIZE;
    const unsigned* opmax = out_planes ? planes_trailer(out_planes, rows) : nullptr;
    const long ntile = conv_tiles(B, D, H, W);
    if (!ws_ok(workspace, workspace_bytes, colsum_part_bytes(ntile, colsum != nullptr))) return DLCS_ERR_WORKSPACE;
    float* cpart = colsum ? static_cast<float*>(workspace) : nullptr;
    const int rc = conv_thin_f16x3_launch(v, (const f16*)wthin, in_max, (int)cin, thin_in, st, (f16*)out_planes, opmax,
                                          cpart);
    if (rc || !colsum) return rc;
    return launch_colsum_parts(cpart, (int)ntile, colsum, st);
}

int dlcs_conv3d_thin_wgrad_f16x3(const float* in, int64_t cin, int64_t cin_ld, const unsigned* in_max,
                                 const float* g, int64_t cout, int64_t g_ld, const unsigned* g_max, float* dw_packed,
                                 int64_t cout_pad, int64_t cin_pad, float* colsum, int64_t B, int64_t D, int64_t H,
                                 int64_t W, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(in && in_max && g && g_max && dw_packed && B > 0 && cout <= cout_pad && cin <= cin_pad);
    const bool thin_sfe = cout == 160 && cin >= 1 && cin <= 4;
    const bool thin_fin = cin == 160 && cout >= 1 && cout <= 4;
    const long npatch = B * (D / 4) * (H / 4) * (W / 4);
    if ((!thin_sfe && !thin_fin) || (colsum && !thin_sfe) || D % 4 || H % 4 || W % 4 || cin_ld % 4 || g_ld % 4 ||
        !al16(in) || !al16(g) || npatch >= (1L << 24))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    ThinWgH3Args t{};
    t.big = thin_sfe ? g : in;
    t.thin = thin_sfe ? in : g;
    t.big_max = thin_sfe ? g_max : in_max;
    t.thin_max = thin_sfe ? in_max : g_max;
    t.dw = dw_packed; t.colsum = colsum;
    t.big_ld = (int)(thin_sfe ? g_ld : cin_ld); t.thin_ld = (int)(thin_sfe ? cin_ld : g_ld);
    t.sgn = thin_sfe ? 1 : -1; t.big_is_co = thin_sfe; t.thin_ch = (int)(thin_sfe ? cin : cout);
    t.cout_pad = (int)cout_pad; t.cin_pad = (int)cin_pad;
    t.B = (int)B; t.D = (int)D; t.H = (int)H; t.W = (int)W;
    const int nr = (int)std::min<long>(256, npatch);
    const int pp = (int)((npatch + nr - 1) / nr);
    hipLaunchKernelGGL(conv3d_wgrad_thin_f16x3_kernel, dim3(nr), dim3(512), 0, (hipStream_t)stream, t, nr, pp);
    return dlcs_launch_status();
}

int dlcs_conv3d_thin_out_planes_f16x3(const void* xplanes, const void* wthin, const float* bias, float* out,
                                      int64_t cout, int64_t cout_ld, int64_t B, int64_t D, int64_t H, int64_t W,
                                      int accumulate, int relu_out, dlcs_stream_t stream) {
    return dlcs_conv3d_thin_out_planes_f16x3_slabs(xplanes, wthin, bias, out, cout, cout_ld, B, D, H, W, accumulate,
                                                   relu_out, 0, D / 4, stream);
}

int dlcs_conv3d_thin_out_planes_f16x3_slabs(const void* xplanes, const void* wthin, const float* bias, float* out,
                                            int64_t cout, int64_t cout_ld, int64_t B, int64_t D, int64_t H, int64_t W,
                                            int accumulate, int relu_out, int64_t tb0, int64_t tb1,
                                            dlcs_stream_t stream) {
    DLCS_CHECK_ARG(xplanes && wthin && out && B > 0 && cout >= 1 && cout <= 4 && cout_ld >= 4);
    if (D % 4 || H % 4 || W % 4 || cout_ld % 4 || !al16(xplanes) || !al16(wthin) || !al16(out))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    ConvF32Args v{};
    v.bias = bias; v.out = out;
    v.B = (int)B; v.D = (int)D; v.H = (int)H; v.W = (int)W;
    v.cout_ld = (int)cout_ld; v.accumulate = accumulate; v.relu_out = relu_out; v.cout = (int)cout;
    v.cout_pad = (int)cout;
    const int64_t nT = D / 4;
    const int s0 = (int)std::max<int64_t>(0, std::min(tb0, nT)), s1 = (int)std::max<int64_t>(0, std::min(tb1, nT));
    return conv_thin_out_p_launch(v, (const f16*)xplanes, (const f16*)wthin, s0, s1, (hipStream_t)stream);
}

size_t dlcs_conv3d_thin_wgrad_planes_f16x3_workspace_bytes(void) { return (size_t)kTwpWG * 160 * 128 * sizeof(float); }

int dlcs_conv3d_thin_wgrad_planes_f16x3(const void* bigplanes, const float* thin, int64_t thin_ch, int64_t thin_ld,
                                        const unsigned* thin_max, int big_is_co, float* dw_packed, int64_t cout_pad,
                                        int64_t cin_pad, int64_t B, int64_t D, int64_t H, int64_t W, void* workspace,
                                        size_t workspace_bytes, dlcs_stream_t stream) {
    return dlcs_conv3d_thin_wgrad_planes_f16x3_live(bigplanes, thin, thin_ch, thin_ld, thin_max, big_is_co, dw_packed,
                                                    cout_pad, cin_pad, B, D, H, W, 0, D, workspace, workspace_bytes,
                                                    stream);
}

int dlcs_conv3d_thin_wgrad_planes_f16x3_live(const void* bigplanes, const float* thin, int64_t thin_ch,
                                             int64_t thin_ld, const unsigned* thin_max, int big_is_co,
                                             float* dw_packed, int64_t cout_pad, int64_t cin_pad, int64_t B, int64_t D,
                                             int64_t H, int64_t W, int64_t t_lo, int64_t t_hi, void* workspace,
                                             size_t workspace_bytes, dlcs_stream_t stream) {
    // the window is on the thin operand as g (the final conv's shape)
    DLCS_CHECK_ARG(!big_is_co || (t_lo <= 0 && t_hi >= D));
    DLCS_CHECK_ARG(bigplanes && thin && thin_max && dw_packed && B > 0 && thin_ch >= 1 && thin_ch <= 4 &&
                   thin_ld >= 4);
    if (D % 4 || H % 4 || W % 4 || thin_ld % 4 || !al16(bigplanes) || !al16(thin) ||
        (big_is_co ? (cout_pad < 160 || cin_pad < thin_ch) : (cin_pad < 160 || cout_pad < thin_ch)))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    ThinWgPArgs t{};
    t.bp = (const f16*)bigplanes; t.thin = thin; t.dw = dw_packed; t.thin_max = thin_max;
    t.rows = (long)B * D * H * W;
    t.thin_ld = (int)thin_ld; t.sgn = big_is_co ? 1 : -1; t.big_is_co = big_is_co ? 1 : 0; t.thin_ch = (int)thin_ch;
    t.cout_pad = (int)cout_pad; t.cin_pad = (int)cin_pad;
    t.B = (int)B; t.D = (int)D; t.H = (int)H; t.W = (int)W;
    if (!ws_ok(workspace, workspace_bytes, dlcs_conv3d_thin_wgrad_planes_f16x3_workspace_bytes()))
        return DLCS_ERR_WORKSPACE;
    t.part = static_cast<float*>(workspace);                 // one [160][128] slab per workgroup
    const int lo = (int)std::max<int64_t>(0, std::min(t_lo, D)), hi = (int)std::max<int64_t>(0, std::min(t_hi, D));
    return wgrad_thin_p_launch(t, lo, hi, (hipStream_t)stream);
}

}  // extern "C"
