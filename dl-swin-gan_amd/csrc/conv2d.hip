// Plane conv for the DSLR family's bf16 compute path (dlcs.h "Plane conv"): a k = 3
// convolution over independent planes as an implicit GEMM on v_mfma_f32_32x32x16_bf16.
//
//   KH = 3: planes [N][H][W], taps (dy, dx), zero padding at the H and W borders
//   KH = 1: sequences [N H][W], taps dx only
//
// Rows are channels-last, row = (n H + h) W + w, not patch-blocked; the planes of a tile are
// consecutive rows.
//
// Forward / dgrad (conv2d_k3_kernel).  A workgroup of 4 waves owns an M tile of PP whole planes
// (PP H W <= 256 pixels: 16 planes of 4 x 4, 4 of 8 x 8, 1 of 16 x 16; 10 sequences of 24) and
// 32 NT output channels.  Per 32-channel chunk of cin it stages the planes' halo image
// [PP][HR][HC][32 ch] in LDS -- halo positions outside a plane, planes the last tile does not
// have and channels >= cin are zero fill, so no row of another plane is ever read -- and every
// wave multiplies its 64 pixels (two 32-pixel MFMA tiles) by the taps' weight fragments, which
// come straight from the packed weight [tap][co][ci] (16 B per lane, shared by all workgroups,
// L2 resident).  The weights are the A operand, so a lane ends up with one pixel and groups of 4
// consecutive channels: the epilogue (bias, ReLU mask, residual, ReLU) reads and writes 8- or
// 16-B pieces.  LDS rows are 32 + 8 channels (80 B), 51,200 B per workgroup.
//
// Weight gradient (conv2d_wgrad_kernel).  K = pixels.  A workgroup owns (pixel range, tap,
// 128 output channels); its 4 waves own one 32-row co tile each with all of cin_pad as NT 32 x 32
// accumulators.  Per 64 pixels it stages g [64][co] and the tap-shifted x [64][ci] (zero where
// the shifted pixel leaves its plane) and reads both pixel-contiguous with ds_read_b64_tr_b16,
// as conv3d_wgrad_row.inc does.  Every workgroup stores its whole slab to the caller's workspace
// and conv2d_wgrad_reduce_kernel adds the ranges in order: no atomics, the same bits every run.
#include "dlcs_common.h"
#include "conv2d_geom.h"

namespace {

constexpr int C2_XLD = 40;         // bf16 per halo row in LDS: a 32-channel chunk + 8 (80 B)

struct Conv2dArgs {
    const bf16* in;
    const bf16* w;
    const float* bias;
    void* out;
    const bf16* mask;
    const void* res;
    int cin, cin_ld, cin_pad, cout, cout_pad, cout_ld, mask_ld, res_ld;
    int out_bf16, res_bf16, relu_out;
    float res_scale;
    int PH, PW, HR, HC, PP;
    long nplanes;
};

template <int KH, int NT>
__global__ void __launch_bounds__(256) conv2d_k3_kernel(Conv2dArgs a) {
    __shared__ __attribute__((aligned(16))) bf16 Xs[C2_HALO * C2_XLD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const long plane0 = (long)blockIdx.x * a.PP;
    const long left = a.nplanes - plane0;
    const int np = left < a.PP ? (int)left : a.PP;           // the last tile masks the planes it does not have
    const int ppix = a.PH * a.PW, hpl = a.HR * a.HC;
    const int mp = np * ppix, nhalo = np * hpl;
    const long row0 = plane0 * ppix;
    const int n0 = blockIdx.y * (NT * 32);

    int hb[2];                                                // halo row of the lane's pixel at tap (0, 0)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int m = wave * 64 + mt * 32 + r;
        const int mm = m < mp ? m : 0;
        const int pl = mm / ppix, rem = mm - pl * ppix;
        const int y = rem / a.PW, x = rem - y * a.PW;
        hb[mt] = pl * hpl + y * a.HC + x;
    }
    f32x16 acc[NT][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { acc[nt][0] = (f32x16)0.0f; acc[nt][1] = (f32x16)0.0f; }

    for (int c0 = 0; c0 < a.cin_pad; c0 += 32) {
        __syncthreads();
        for (int i = threadIdx.x; i < nhalo * 4; i += 256) {
            const int hr = i >> 2, c8 = c0 + (i & 3) * 8;
            const int pl = hr / hpl, rem = hr - pl * hpl;
            const int hy = rem / a.HC, hx = rem - hy * a.HC;
            const int y = KH == 3 ? hy - 1 : 0, x = hx - 1;
            Frag8<bf16> f = zero8<bf16>();
            if (c8 < a.cin && y >= 0 && y < a.PH && x >= 0 && x < a.PW) {
                f = load8<bf16>(a.in + (row0 + (long)pl * ppix + y * a.PW + x) * a.cin_ld + c8);
#pragma unroll
                for (int e = 0; e < 8; ++e) if (c8 + e >= a.cin) f.v[e] = (bf16)0.0f;
            }
            *reinterpret_cast<bf16x8*>(Xs + hr * C2_XLD + (i & 3) * 8) = f.v;
        }
        __syncthreads();
        if (wave * 64 < mp) {
#pragma unroll
            for (int tap = 0; tap < KH * 3; ++tap) {
                const int toff = (tap / 3) * a.HC + tap % 3;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const Frag8<bf16> b0 = load8<bf16>(Xs + (hb[0] + toff) * C2_XLD + ks * 16 + 8 * h);
                    const Frag8<bf16> b1 = load8<bf16>(Xs + (hb[1] + toff) * C2_XLD + ks * 16 + 8 * h);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const Frag8<bf16> aw = load8<bf16>(a.w + ((long)tap * a.cout_pad + n0 + nt * 32 + r) * a.cin_pad +
                                                           c0 + ks * 16 + 8 * h);
                        mfma32(acc[nt][0], aw, b0);
                        mfma32(acc[nt][1], aw, b1);
                    }
                }
            }
        }
    }

    // epilogue: lane = pixel, registers 4 q .. 4 q + 3 = channels n0 + 32 nt + 8 q + 4 h + (0..3)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int m = wave * 64 + mt * 32 + r;
        if (m >= mp) continue;
        const long row = row0 + m;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int co = n0 + nt * 32 + 8 * q + 4 * h;
                if (co >= a.cout) continue;
                const bool full = co + 4 <= a.cout;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[nt][mt][4 * q + e];
                if (a.bias) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (co + e < a.cout) v[e] += a.bias[co + e];
                }
                if (a.mask) {
                    const bf16* mp_ = a.mask + row * a.mask_ld + co;
                    if (full) {
                        const bf16x4 mk = *reinterpret_cast<const bf16x4*>(mp_);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = (float)mk[e] > 0.0f ? v[e] : 0.0f;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (co + e < a.cout) v[e] = (float)mp_[e] > 0.0f ? v[e] : 0.0f;
                    }
                }
                if (a.res) {
                    if (a.res_bf16) {
                        const bf16* rp = reinterpret_cast<const bf16*>(a.res) + row * a.res_ld + co;
                        if (full) {
                            const bf16x4 rv = *reinterpret_cast<const bf16x4*>(rp);
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] += a.res_scale * (float)rv[e];
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) if (co + e < a.cout) v[e] += a.res_scale * (float)rp[e];
                        }
                    } else {
                        const float* rp = reinterpret_cast<const float*>(a.res) + row * a.res_ld + co;
                        if (full) {
                            const f32x4 rv = *reinterpret_cast<const f32x4*>(rp);
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] += a.res_scale * rv[e];
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) if (co + e < a.cout) v[e] += a.res_scale * rp[e];
                        }
                    }
                }
                if (a.relu_out) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
                }
                if (a.out_bf16) {
                    bf16* op = reinterpret_cast<bf16*>(a.out) + row * a.cout_ld + co;
                    if (full) {
                        bf16x4 ov;
#pragma unroll
                        for (int e = 0; e < 4; ++e) ov[e] = (bf16)v[e];
                        *reinterpret_cast<bf16x4*>(op) = ov;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (co + e < a.cout) op[e] = (bf16)v[e];
                    }
                } else {
                    float* op = reinterpret_cast<float*>(a.out) + row * a.cout_ld + co;
                    if (full) {
                        f32x4 ov;
#pragma unroll
                        for (int e = 0; e < 4; ++e) ov[e] = v[e];
                        *reinterpret_cast<f32x4*>(op) = ov;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (co + e < a.cout) op[e] = v[e];
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------ weight gradient
struct Wgrad2dArgs {
    const bf16* in;
    const bf16* g;
    float* ws;        // [range][tap][cout_pad][cin_pad] partial slabs
    float* wsb;       // [range][cout_pad] partial column sums of g (NULL: no bias gradient)
    int cin, cin_ld, cin_pad, cout, g_ld, cout_pad;
    int PH, PW, KH;
    long rows, ppr;
};

typedef short c2_v4s __attribute__((ext_vector_type(4)));

// 8 pixels (rows a0 .. + 3 and a1 .. + 3 of the lane group's 4 x 16 blocks) of one channel
DLCS_DEV Frag8<bf16> c2_tr_rows(const bf16* a0, const bf16* a1) {
    typedef __attribute__((address_space(3))) c2_v4s lds_v4s;
    typedef short v8s __attribute__((ext_vector_type(8)));
    const c2_v4s r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(const_cast<bf16*>(a0)));
    const c2_v4s r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(const_cast<bf16*>(a1)));
    const v8s both = {r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], r1[2], r1[3]};
    Frag8<bf16> f;
    f.v = __builtin_bit_cast(bf16x8, both);
    return f;
}

template <int NT>
__global__ void __launch_bounds__(256) conv2d_wgrad_kernel(Wgrad2dArgs a) {
    constexpr int GLD = C2_WG_CO + 32;                        // 16 or 48 dwords mod 64 (conv3d_wgrad_row.inc)
    constexpr int XLD = NT * 32 + (NT % 2 ? 0 : 32);
    __shared__ __attribute__((aligned(16))) bf16 Gs[C2_WG_PIX * GLD];
    __shared__ __attribute__((aligned(16))) bf16 Xs[C2_WG_PIX * XLD];
    const int range = blockIdx.x, tap = blockIdx.y;
    const int co0 = blockIdx.z * C2_WG_CO;
    const int cow = min(C2_WG_CO, a.cout_pad - co0);          // a multiple of 32
    const int dy = a.KH == 3 ? tap / 3 - 1 : 0, dx = tap % 3 - 1;
    const int ppix = a.PH * a.PW;
    const long p0 = (long)range * a.ppr;
    const long p1 = min(a.rows, p0 + a.ppr);
    const int lane = threadIdx.x & 63, mt = threadIdx.x >> 6;
    const bool active = mt * 32 < cow;                        // wave-uniform: the transposed reads need a full wave

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = (f32x16)0.0f;
    const bool sums = a.wsb && tap == 0 && (int)threadIdx.x < cow;       // thread = a column of g
    float bs = 0.0f;

    const int hh = lane >> 5, c16 = (lane >> 4) & 1, q = (lane >> 2) & 3, p4 = (lane & 3) * 4;
    const bf16* Ga = Gs + (8 * hh + q) * GLD + mt * 32 + 16 * c16 + p4;
    const bf16* Xa = Xs + (8 * hh + q) * XLD + 16 * c16 + p4;
    const int gpc = cow / 8, xpc = a.cin_pad / 8;

    for (long pb = p0; pb < p1; pb += C2_WG_PIX) {
        __syncthreads();
        for (int i = threadIdx.x; i < C2_WG_PIX * gpc; i += 256) {
            const int vl = i / gpc, c8 = (i - vl * gpc) * 8;
            const long p = pb + vl;
            Frag8<bf16> f = zero8<bf16>();
            if (p < p1 && co0 + c8 < a.cout) {
                f = load8<bf16>(a.g + p * a.g_ld + co0 + c8);
#pragma unroll
                for (int e = 0; e < 8; ++e) if (co0 + c8 + e >= a.cout) f.v[e] = (bf16)0.0f;
            }
            *reinterpret_cast<bf16x8*>(Gs + vl * GLD + c8) = f.v;
        }
        for (int i = threadIdx.x; i < C2_WG_PIX * xpc; i += 256) {
            const int vl = i / xpc, c8 = (i - vl * xpc) * 8;
            const long p = pb + vl;
            Frag8<bf16> f = zero8<bf16>();
            if (p < p1 && c8 < a.cin) {
                const int rem = (int)(p % ppix);
                const int y = rem / a.PW + dy, x = rem % a.PW + dx;
                if (y >= 0 && y < a.PH && x >= 0 && x < a.PW) {
                    f = load8<bf16>(a.in + (p + dy * a.PW + dx) * a.cin_ld + c8);
#pragma unroll
                    for (int e = 0; e < 8; ++e) if (c8 + e >= a.cin) f.v[e] = (bf16)0.0f;
                }
            }
            *reinterpret_cast<bf16x8*>(Xs + vl * XLD + c8) = f.v;
        }
        __syncthreads();
        if (sums) {
            for (int vl = 0; vl < C2_WG_PIX; ++vl) bs += (float)Gs[vl * GLD + threadIdx.x];
        }
        if (active) {
#pragma unroll
            for (int kk = 0; kk < C2_WG_PIX / 16; ++kk) {
                const Frag8<bf16> af = c2_tr_rows(Ga + kk * 16 * GLD, Ga + (kk * 16 + 4) * GLD);
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    if (j * 32 < a.cin_pad) {
                        const Frag8<bf16> bfr = c2_tr_rows(Xa + kk * 16 * XLD + j * 32, Xa + (kk * 16 + 4) * XLD + j * 32);
                        mfma32(acc[j], af, bfr);
                    }
                }
            }
        }
    }
    if (sums) a.wsb[(long)range * a.cout_pad + co0 + threadIdx.x] = bs;
    if (!active) return;
    float* slab = a.ws + ((long)range * (a.KH * 3) + tap) * a.cout_pad * a.cin_pad;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int ci = j * 32 + (lane & 31);
        if (ci >= a.cin_pad) continue;
#pragma unroll
        for (int rg = 0; rg < 16; ++rg) {
            const int co = co0 + mt * 32 + acc_row(rg, lane);
            slab[(long)co * a.cin_pad + ci] = acc[j][rg];
        }
    }
}

// dw[i] += the ranges' slabs, dbias[c] += their column sums, in range order
__global__ void conv2d_wgrad_reduce_kernel(const float* ws, float* dw, long n, int nrange, const float* wsb, float* dbias,
                                           int cout, int cout_pad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    float s = 0.0f;
    if (i < n) {
        for (int k = 0; k < nrange; ++k) s += ws[(long)k * n + i];
        dw[i] += s;
    } else if (dbias && i - n < cout) {
        for (int k = 0; k < nrange; ++k) s += wsb[(long)k * cout_pad + (i - n)];
        dbias[i - n] += s;
    }
}

__global__ void conv2d_pack_kernel(const float* w, bf16* packed, int cout, int cin, int rows_pad, int cols_pad,
                                   int ntap, int mode) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long n = (long)ntap * rows_pad * cols_pad;
    if (i >= n) return;
    const int col = (int)(i % cols_pad), row = (int)((i / cols_pad) % rows_pad), tap = (int)(i / ((long)cols_pad * rows_pad));
    const int co = mode == 0 ? row : col, ci = mode == 0 ? col : row;
    const int t = mode == 0 ? tap : ntap - 1 - tap;
    packed[i] = (co < cout && ci < cin) ? (bf16)w[((long)co * cin + ci) * ntap + t] : (bf16)0.0f;
}

__global__ void conv2d_unpack_kernel(const float* dw, float* grad, int cout, int cin, int rows_pad, int cols_pad, int ntap,
                                     int accumulate) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)cout * cin * ntap) return;
    const int t = (int)(i % ntap), ci = (int)((i / ntap) % cin), co = (int)(i / ((long)ntap * cin));
    const float v = dw[((long)t * rows_pad + co) * cols_pad + ci];
    grad[i] = accumulate ? grad[i] + v : v;
}

}  // namespace

extern "C" {

int dlcs_conv2d_k3(const void* in, int64_t cin, int64_t cin_ld, const void* wpacked, int64_t cin_pad,
                   const float* bias, void* out, int out_dtype, int64_t cout, int64_t cout_pad, int64_t cout_ld,
                   int64_t N, int64_t H, int64_t W, int KH, const void* mask, int64_t mask_ld,
                   const void* residual, int res_dtype, int64_t res_ld, float res_scale, int relu_out,
                   dlcs_stream_t stream) {
    DLCS_CHECK_ARG(in && wpacked && out);
    DLCS_CHECK_ARG(out_dtype == DLCS_F32 || out_dtype == DLCS_BF16);
    DLCS_CHECK_ARG(!residual || res_dtype == DLCS_F32 || res_dtype == DLCS_BF16);
    Conv2dGeom g;
    const int st = conv2d_geom(N, H, W, KH, &g);
    if (st) return st;
    if (cin < 1 || cout < 1 || cin > C2_MAX_CH || cout > C2_MAX_CH) return DLCS_ERR_UNSUPPORTED_SIZE;
    DLCS_CHECK_ARG(conv2d_channels_ok(cin, cin_pad) && conv2d_channels_ok(cout, cout_pad));
    const int64_t ldmax = (int64_t)1 << 20;
    DLCS_CHECK_ARG(cin_ld >= cin && cin_ld % 8 == 0 && cout_ld >= cout && cout_ld % 8 == 0 && cin_ld < ldmax && cout_ld < ldmax);
    DLCS_CHECK_ARG(!mask || (mask_ld >= cout && mask_ld % 8 == 0 && mask_ld < ldmax));
    DLCS_CHECK_ARG(!residual || (res_ld >= cout && res_ld % 8 == 0 && res_ld < ldmax));
    DLCS_CHECK_ARG(al16(in) && al16(wpacked) && al16(out) && al16(mask) && al16(residual));
    Conv2dArgs a;
    a.in = (const bf16*)in; a.w = (const bf16*)wpacked; a.bias = bias; a.out = out;
    a.mask = (const bf16*)mask; a.res = residual;
    a.cin = (int)cin; a.cin_ld = (int)cin_ld; a.cin_pad = (int)cin_pad;
    a.cout = (int)cout; a.cout_pad = (int)cout_pad; a.cout_ld = (int)cout_ld;
    a.mask_ld = (int)mask_ld; a.res_ld = (int)res_ld;
    a.out_bf16 = out_dtype == DLCS_BF16; a.res_bf16 = res_dtype == DLCS_BF16; a.relu_out = relu_out;
    a.res_scale = res_scale;
    a.PH = g.PH; a.PW = g.PW; a.HR = g.HR; a.HC = g.HC; a.PP = g.PP; a.nplanes = g.nplanes;
    hipStream_t s = (hipStream_t)stream;
    const int nt = cout_pad % 64 == 0 ? 2 : 1;
    const dim3 grid((unsigned)g.ntiles, (unsigned)(cout_pad / (32 * nt))), block(256);
    if (KH == 3 && nt == 2) hipLaunchKernelGGL((conv2d_k3_kernel<3, 2>), grid, block, 0, s, a);
    else if (KH == 3) hipLaunchKernelGGL((conv2d_k3_kernel<3, 1>), grid, block, 0, s, a);
    else if (nt == 2) hipLaunchKernelGGL((conv2d_k3_kernel<1, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((conv2d_k3_kernel<1, 1>), grid, block, 0, s, a);
    return dlcs_launch_status();
}

int dlcs_conv2d_pack_weights(const float* w, void* packed, int64_t cout, int64_t cin, int64_t rows_pad,
                             int64_t cols_pad, int KH, int mode, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(w && packed && (KH == 3 || KH == 1) && (mode == 0 || mode == 1));
    if (cin < 1 || cout < 1 || cin > C2_MAX_CH || cout > C2_MAX_CH) return DLCS_ERR_UNSUPPORTED_SIZE;
    DLCS_CHECK_ARG(conv2d_channels_ok(mode == 0 ? cout : cin, rows_pad) && conv2d_channels_ok(mode == 0 ? cin : cout, cols_pad));
    const long n = (long)KH * 3 * rows_pad * cols_pad;
    hipLaunchKernelGGL(conv2d_pack_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, w, (bf16*)packed,
                       (int)cout, (int)cin, (int)rows_pad, (int)cols_pad, KH * 3, mode);
    return dlcs_launch_status();
}

size_t dlcs_conv2d_k3_wgrad_workspace_bytes(int64_t cin_pad, int64_t cout_pad, int64_t N, int64_t H, int64_t W, int KH,
                                            int64_t pix_per_block) {
    Conv2dGeom g;
    if (conv2d_geom(N, H, W, KH, &g)) return 0;
    if (cin_pad < 32 || cout_pad < 32 || cin_pad > C2_MAX_CH || cout_pad > C2_MAX_CH) return 0;
    const long ppr = conv2d_wgrad_ppr(pix_per_block);
    return conv2d_wgrad_ws(conv2d_wgrad_ranges(g.rows, ppr), KH, cout_pad, cin_pad);
}

int dlcs_conv2d_k3_wgrad(const void* in, int64_t cin, int64_t cin_ld, int64_t cin_pad, const void* gout, int64_t cout,
                         int64_t g_ld, int64_t cout_pad, float* dw_packed, float* dbias, int64_t N, int64_t H, int64_t W, int KH,
                         int64_t pix_per_block, void* workspace, size_t workspace_bytes, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(in && gout && dw_packed);
    Conv2dGeom g;
    const int st = conv2d_geom(N, H, W, KH, &g);
    if (st) return st;
    if (cin < 1 || cout < 1 || cin > C2_MAX_CH || cout > C2_MAX_CH) return DLCS_ERR_UNSUPPORTED_SIZE;
    DLCS_CHECK_ARG(conv2d_channels_ok(cin, cin_pad) && conv2d_channels_ok(cout, cout_pad));
    const int64_t ldmax = (int64_t)1 << 20;
    DLCS_CHECK_ARG(cin_ld >= cin && cin_ld % 8 == 0 && g_ld >= cout && g_ld % 8 == 0 && cin_ld < ldmax && g_ld < ldmax);
    DLCS_CHECK_ARG(al16(in) && al16(gout) && al16(workspace));
    const long ppr = conv2d_wgrad_ppr(pix_per_block);
    const long nrange = conv2d_wgrad_ranges(g.rows, ppr);
    if (nrange > 65535) return DLCS_ERR_UNSUPPORTED_SIZE;
    if (!ws_ok(workspace, workspace_bytes, conv2d_wgrad_ws(nrange, KH, cout_pad, cin_pad))) return DLCS_ERR_WORKSPACE;
    Wgrad2dArgs a;
    a.in = (const bf16*)in; a.g = (const bf16*)gout; a.ws = (float*)workspace;
    a.wsb = dbias ? a.ws + conv2d_wgrad_slab_floats(nrange, KH, cout_pad, cin_pad) : nullptr;
    a.cin = (int)cin; a.cin_ld = (int)cin_ld; a.cin_pad = (int)cin_pad;
    a.cout = (int)cout; a.g_ld = (int)g_ld; a.cout_pad = (int)cout_pad;
    a.PH = g.PH; a.PW = g.PW; a.KH = KH; a.rows = g.rows; a.ppr = ppr;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)nrange, (unsigned)(KH * 3), (unsigned)((cout_pad + C2_WG_CO - 1) / C2_WG_CO)), block(256);
    const int nt = (int)(cin_pad / 32);
    if (nt == 1) hipLaunchKernelGGL((conv2d_wgrad_kernel<1>), grid, block, 0, s, a);
    else if (nt == 2) hipLaunchKernelGGL((conv2d_wgrad_kernel<2>), grid, block, 0, s, a);
    else if (nt <= 4) hipLaunchKernelGGL((conv2d_wgrad_kernel<4>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((conv2d_wgrad_kernel<8>), grid, block, 0, s, a);
    int e = dlcs_launch_status();
    if (e) return e;
    const long n = (long)KH * 3 * cout_pad * cin_pad;
    hipLaunchKernelGGL(conv2d_wgrad_reduce_kernel, dim3(cdiv(n + cout_pad, 256)), dim3(256), 0, s, (const float*)workspace,
                       dw_packed, n, (int)nrange, (const float*)a.wsb, dbias, (int)cout, (int)cout_pad);
    return dlcs_launch_status();
}

int dlcs_conv2d_unpack_wgrad(const float* dw_packed, float* grad, int64_t cout, int64_t cin, int64_t cout_pad,
                             int64_t cin_pad, int KH, int accumulate, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(dw_packed && grad && (KH == 3 || KH == 1));
    if (cin < 1 || cout < 1 || cin > C2_MAX_CH || cout > C2_MAX_CH) return DLCS_ERR_UNSUPPORTED_SIZE;
    DLCS_CHECK_ARG(conv2d_channels_ok(cout, cout_pad) && conv2d_channels_ok(cin, cin_pad));
    hipLaunchKernelGGL(conv2d_unpack_kernel, dim3(cdiv((long)cout * cin * KH * 3, 256)), dim3(256), 0, (hipStream_t)stream,
                       dw_packed, grad, (int)cout, (int)cin, (int)cout_pad, (int)cin_pad, KH * 3, accumulate);
    return dlcs_launch_status();
}

}  // extern "C"
