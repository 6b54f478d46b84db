// A box inside a padded grid: what lets the conv trunks of the ResNet, SE and CBAM
// regularisers take any grid size.  fp32 rows; the *_bf16 entries write / clear bf16 rows.
//
// The conv, SE and CBAM kernels work on the patch-blocked channels-last rows of a grid
// (B, Dp, Hp, Wp) whose axes are multiples of 4.  A true grid ("box") (B, D, H, W),
// D <= Dp, H <= Hp, W <= Wp, sits at the origin of that grid; the rows whose (t, y, x)
// lies outside the box are "slack rows".  A k3 / pad-1 convolution on the padded grid
// equals the zero-padded convolution on the box as long as every tensor a stencil or a
// reduction reads is zero on the slack rows:
//
// * dlcs_box_pre / _pre_bwd / _post / _post_bwd -- dlcs_swin_pre / ... for a box: complex
//   [B,E,T,Y,X] <-> real re | im channels, circular time pad (D = T + 2 pad), rows
//   addressed in (Dp, Hp, Wp).  pre and post_bwd write every row of the padded grid
//   (slack rows +0.0 in all ldc columns), pre_bwd and post read rows of the box only.
// * dlcs_box_zero -- +0.0 into columns [0, C) of every slack row, nothing else touched.
//   A batch item's slack rows are three disjoint slabs,
//       t in [D, Dp)                                  (Dp - D) Hp Wp rows
//       t in [0, D), y in [H, Hp)                     D (Hp - H) Wp rows
//       t in [0, D), y in [0, H), x in [W, Wp)        D H (Wp - W) rows
//   and the kernel enumerates exactly those: one thread per (slack row, column chunk),
//   4 columns as one 16-B store when C % 4 == 0, ld % 4 == 0 and the base is 16-B
//   aligned (se.hip's rule), else one float.  It reads no memory.  bf16 rows: 8 columns per
//   16-B store when C % 8 == 0, ld % 8 == 0 and the base is aligned, else one element.
// * dlcs_box_shift -- the box moved by a voxel shift (sd, sh, sw) inside the padded grid and
//   its adjoint: the centre crop of the DiT / Latte unpatchify2, whose subpatches the final
//   Linear scatters at the origin.  A gather per dst row (one thread per row and 16-B column
//   chunk, rows in blocked order), +0.0 on the rows without a source, optionally + a residual
//   row and a ReLU (DiTResNet's relu(DiT(res) + res)).
#include "dlcs_common.h"

namespace {

// blocked offset of voxel (b, t, y, x) in a [B, Dp, Hp, Wp] grid (all multiples of 4)
DLCS_DEV long box_row(int b, int t, int y, int x, int Dp, int Hp, int Wp) {
    const int nT = Dp >> 2, nY = Hp >> 2, nX = Wp >> 2;
    const long patch = (((long)b * nT + (t >> 2)) * nY + (y >> 2)) * nX + (x >> 2);
    return patch * 64 + ((t & 3) << 4) + ((y & 3) << 2) + (x & 3);
}

struct BoxDims {
    int B, E, Tn, Y, X, pad, Dp, Hp, Wp, ldc;
};

// u[b, t', y, x, c] = (c < E ? Re : Im) x[b, c mod E, (t' - pad) mod T, y, x] inside the box,
// c < 2E; zero for c >= 2E and on slack rows.  POST_BWD: no wrap, zero for t' - pad outside [0, T).
template <bool POST_BWD, typename T>
__global__ void __launch_bounds__(256) box_scatter_kernel(const float2* x, T* u, BoxDims d) {
    const int D = d.Tn + 2 * d.pad;
    const long total = (long)d.B * d.Dp * d.Hp * d.Wp;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int xx = (int)(i % d.Wp);
        long q = i / d.Wp;
        const int y = (int)(q % d.Hp); q /= d.Hp;
        const int tp = (int)(q % d.Dp);
        const int b = (int)(q / d.Dp);
        T* dst = u + box_row(b, tp, y, xx, d.Dp, d.Hp, d.Wp) * d.ldc;
        bool in = tp < D && y < d.Y && xx < d.X;
        int t = tp - d.pad;
        if (POST_BWD) in = in && t >= 0 && t < d.Tn;
        else t = (t % d.Tn + d.Tn) % d.Tn;
        for (int c = 0; c < d.ldc; ++c) {
            float v = 0.0f;
            if (in && c < 2 * d.E) {
                const int e = c % d.E;
                const float2 z = x[((((long)b * d.E + e) * d.Tn + t) * d.Y + y) * d.X + xx];
                v = (c < d.E) ? z.x : z.y;
            }
            dst[c] = from_f<T>(v);
        }
    }
}

// PRE_BWD: gx[b, e, t] = sum over t' = t + pad + k T in [0, D) of g_u (circular-pad adjoint, the
// order of dlcs_swin_pre_bwd); else out[b, e, t] = complex(o[c = e], o[c = E + e]) at t' = t + pad.
template <bool PRE_BWD>
__global__ void __launch_bounds__(256) box_gather_kernel(const float* o, float2* out, BoxDims d) {
    const int D = d.Tn + 2 * d.pad;
    const long total = (long)d.B * d.E * d.Tn * d.Y * d.X;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int xx = (int)(i % d.X);
        long q = i / d.X;
        const int y = (int)(q % d.Y); q /= d.Y;
        const int t = (int)(q % d.Tn); q /= d.Tn;
        const int e = (int)(q % d.E);
        const int b = (int)(q / d.E);
        if (PRE_BWD) {
            float re = 0.0f, im = 0.0f;
            for (int tp = (t + d.pad) % d.Tn; tp < D; tp += d.Tn) {
                const float* src = o + box_row(b, tp, y, xx, d.Dp, d.Hp, d.Wp) * d.ldc;
                re += src[e];
                im += src[d.E + e];
            }
            out[i] = make_float2(re, im);
        } else {
            const float* src = o + box_row(b, t + d.pad, y, xx, d.Dp, d.Hp, d.Wp) * d.ldc;
            out[i] = make_float2(src[e], src[d.E + e]);
        }
    }
}

struct ZeroDims {
    int Dp, Hp, Wp, D, H, W;
    long n1, n2, n3;        // rows of the three slack slabs of one batch item
};

// blockIdx.y = batch item; grid-stride over (slack row, column chunk) pairs of V columns
// (V > 1: one 16-B store, 4 floats or 8 bf16)
template <typename T, int V>
__global__ void __launch_bounds__(256) box_zero_kernel(T* x, long ld, int nch, ZeroDims z) {
    const int b = blockIdx.y;
    const long total = (z.n1 + z.n2 + z.n3) * nch;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int ch = (int)(i % nch);
        long s = i / nch;
        int t, y, xx;
        if (s < z.n1) {                                   // t in [D, Dp), all y, all x
            xx = (int)(s % z.Wp); s /= z.Wp;
            y = (int)(s % z.Hp);
            t = z.D + (int)(s / z.Hp);
        } else if (s < z.n1 + z.n2) {                     // t in [0, D), y in [H, Hp), all x
            s -= z.n1;
            const int hs = z.Hp - z.H;
            xx = (int)(s % z.Wp); s /= z.Wp;
            y = z.H + (int)(s % hs);
            t = (int)(s / hs);
        } else {                                          // t in [0, D), y in [0, H), x in [W, Wp)
            s -= z.n1 + z.n2;
            const int ws = z.Wp - z.W;
            xx = z.W + (int)(s % ws); s /= ws;
            y = (int)(s % z.H);
            t = (int)(s / z.H);
        }
        T* dst = x + box_row(b, t, y, xx, z.Dp, z.Hp, z.Wp) * ld + (long)ch * V;
        if constexpr (V > 1) {
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};             // 16 B of +0.0 in either format
            *reinterpret_cast<f32x4*>(dst) = v;
        } else {
            *dst = from_f<T>(0.0f);
        }
    }
}

struct ShiftDims {
    int Dp, Hp, Wp, D, H, W, sd, sh, sw, nch;
    long rows, ld_src, ld_dst, ld_res;
};

// one thread per (row of the padded grid, chunk of V columns), rows in blocked order so a
// wave's stores are contiguous; the source row is a box_row() gather.  TR false: a box row
// reads the voxel shifted by (+sd, +sh, +sw) (plus its own row of res, then the ReLU), a slack
// row gets +0.0.  TR true (the adjoint): a row reads the voxel at (-sd, -sh, -sw) when that
// is a box voxel, else gets +0.0.
template <int V, bool TR>
__global__ void __launch_bounds__(256) box_shift_kernel(const float* src, float* dst, const float* res, int relu,
                                                        ShiftDims s) {
    const long total = s.rows * s.nch;
    const int nY = s.Hp >> 2, nX = s.Wp >> 2, nT = s.Dp >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / s.nch;
        const long col = (i - r * s.nch) * V;
        const int in = (int)(r & 63);
        long q = r >> 6;
        const int x = (int)(q % nX) * 4 + (in & 3); q /= nX;
        const int y = (int)(q % nY) * 4 + ((in >> 2) & 3); q /= nY;
        const int t = (int)(q % nT) * 4 + (in >> 4);
        const int b = (int)(q / nT);
        const int ts = TR ? t - s.sd : t + s.sd, ys = TR ? y - s.sh : y + s.sh, xs = TR ? x - s.sw : x + s.sw;
        const bool live = TR ? (ts >= 0 && ts < s.D && ys >= 0 && ys < s.H && xs >= 0 && xs < s.W)
                             : (t < s.D && y < s.H && x < s.W);
        float* d = dst + r * s.ld_dst + col;
        if constexpr (V > 1) {
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (live) {
                v = *reinterpret_cast<const f32x4*>(src + box_row(b, ts, ys, xs, s.Dp, s.Hp, s.Wp) * s.ld_src + col);
                if (res) v += *reinterpret_cast<const f32x4*>(res + r * s.ld_res + col);
                if (relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
                }
            }
            *reinterpret_cast<f32x4*>(d) = v;
        } else {
            float v = 0.0f;
            if (live) {
                v = src[box_row(b, ts, ys, xs, s.Dp, s.Hp, s.Wp) * s.ld_src + col];
                if (res) v += res[r * s.ld_res + col];
                if (relu) v = fmaxf(v, 0.0f);
            }
            *d = v;
        }
    }
}

unsigned box_blocks(long n) {
    long g = (n + 255) / 256;
    if (g > 8192) g = 8192;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// the padded grid holds the box, its axes are multiples of 4, every index the kernels form
// in int fits and the row counts formed in long cannot overflow (2^40 rows per batch item
// is beyond any memory)
bool box_grid_ok(long Dp, long Hp, long Wp, long D, long H, long W) {
    return Dp % 4 == 0 && Hp % 4 == 0 && Wp % 4 == 0 && D <= Dp && H <= Hp && W <= Wp &&
           Dp < (1L << 30) && Hp < (1L << 30) && Wp < (1L << 30) && Dp * Hp <= (1L << 40) / Wp;
}

int box_dims(BoxDims* d, const void* a, const void* b, int64_t B, int64_t E, int64_t Tn, int64_t Y, int64_t X,
             int64_t pad, int64_t Dp, int64_t Hp, int64_t Wp, int64_t ldc) {
    DLCS_CHECK_ARG(a && b && B > 0 && E > 0 && Tn > 0 && Y > 0 && X > 0 && pad >= 0 && ldc >= 2 * E &&
                   Tn < (1L << 30) && pad < (1L << 30));
    if (!box_grid_ok(Dp, Hp, Wp, Tn + 2 * pad, Y, X) || B > (1L << 20) || E > (1L << 20) || B * E > (1L << 20) ||
        ldc >= (1L << 30))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    *d = BoxDims{(int)B, (int)E, (int)Tn, (int)Y, (int)X, (int)pad, (int)Dp, (int)Hp, (int)Wp, (int)ldc};
    return 0;
}

}  // namespace

extern "C" {

int dlcs_box_pre(const void* x, float* u, int64_t B, int64_t E, int64_t T, int64_t Y, int64_t X, int64_t pad,
                 int64_t Dp, int64_t Hp, int64_t Wp, int64_t ldc, dlcs_stream_t stream) {
    BoxDims d;
    if (const int rc = box_dims(&d, x, u, B, E, T, Y, X, pad, Dp, Hp, Wp, ldc)) return rc;
    hipLaunchKernelGGL((box_scatter_kernel<false, float>), dim3(box_blocks(B * Dp * Hp * Wp)), dim3(256), 0,
                       (hipStream_t)stream, (const float2*)x, u, d);
    return dlcs_launch_status();
}

int dlcs_box_pre_bf16(const void* x, void* u, int64_t B, int64_t E, int64_t T, int64_t Y, int64_t X, int64_t pad,
                      int64_t Dp, int64_t Hp, int64_t Wp, int64_t ldc, dlcs_stream_t stream) {
    BoxDims d;
    if (const int rc = box_dims(&d, x, u, B, E, T, Y, X, pad, Dp, Hp, Wp, ldc)) return rc;
    hipLaunchKernelGGL((box_scatter_kernel<false, bf16>), dim3(box_blocks(B * Dp * Hp * Wp)), dim3(256), 0,
                       (hipStream_t)stream, (const float2*)x, (bf16*)u, d);
    return dlcs_launch_status();
}

int dlcs_box_pre_bwd(const float* gu, void* gx, int64_t B, int64_t E, int64_t T, int64_t Y, int64_t X, int64_t pad,
                     int64_t Dp, int64_t Hp, int64_t Wp, int64_t ldc, dlcs_stream_t stream) {
    BoxDims d;
    if (const int rc = box_dims(&d, gu, gx, B, E, T, Y, X, pad, Dp, Hp, Wp, ldc)) return rc;
    hipLaunchKernelGGL(box_gather_kernel<true>, dim3(box_blocks(B * E * T * Y * X)), dim3(256), 0, (hipStream_t)stream,
                       gu, (float2*)gx, d);
    return dlcs_launch_status();
}

int dlcs_box_post(const float* o, void* out, int64_t B, int64_t E, int64_t T, int64_t Y, int64_t X, int64_t pad,
                  int64_t Dp, int64_t Hp, int64_t Wp, int64_t ldc, dlcs_stream_t stream) {
    BoxDims d;
    if (const int rc = box_dims(&d, o, out, B, E, T, Y, X, pad, Dp, Hp, Wp, ldc)) return rc;
    hipLaunchKernelGGL(box_gather_kernel<false>, dim3(box_blocks(B * E * T * Y * X)), dim3(256), 0, (hipStream_t)stream,
                       o, (float2*)out, d);
    return dlcs_launch_status();
}

int dlcs_box_post_bwd(const void* gout, float* go, int64_t B, int64_t E, int64_t T, int64_t Y, int64_t X, int64_t pad,
                      int64_t Dp, int64_t Hp, int64_t Wp, int64_t ldc, dlcs_stream_t stream) {
    BoxDims d;
    if (const int rc = box_dims(&d, gout, go, B, E, T, Y, X, pad, Dp, Hp, Wp, ldc)) return rc;
    hipLaunchKernelGGL((box_scatter_kernel<true, float>), dim3(box_blocks(B * Dp * Hp * Wp)), dim3(256), 0,
                       (hipStream_t)stream, (const float2*)gout, go, d);
    return dlcs_launch_status();
}

int dlcs_box_post_bwd_bf16(const void* gout, void* go, int64_t B, int64_t E, int64_t T, int64_t Y, int64_t X,
                           int64_t pad, int64_t Dp, int64_t Hp, int64_t Wp, int64_t ldc, dlcs_stream_t stream) {
    BoxDims d;
    if (const int rc = box_dims(&d, gout, go, B, E, T, Y, X, pad, Dp, Hp, Wp, ldc)) return rc;
    hipLaunchKernelGGL((box_scatter_kernel<true, bf16>), dim3(box_blocks(B * Dp * Hp * Wp)), dim3(256), 0,
                       (hipStream_t)stream, (const float2*)gout, (bf16*)go, d);
    return dlcs_launch_status();
}

int dlcs_box_zero(float* x, int64_t ld, int64_t C, int64_t B, int64_t Dp, int64_t Hp, int64_t Wp, int64_t D, int64_t H,
                  int64_t W, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(x && B > 0 && C > 0 && ld >= C && D > 0 && H > 0 && W > 0);
    if (!box_grid_ok(Dp, Hp, Wp, D, H, W) || B > 65535 || C >= (1L << 30)) return DLCS_ERR_UNSUPPORTED_SIZE;
    ZeroDims z{(int)Dp, (int)Hp, (int)Wp, (int)D, (int)H, (int)W, (Dp - D) * Hp * Wp, D * (Hp - H) * Wp, D * H * (Wp - W)};
    const long n = z.n1 + z.n2 + z.n3;
    if (n == 0) return 0;
    const bool vec = C % 4 == 0 && ld % 4 == 0 && al16(x);
    const int nch = (int)(vec ? C / 4 : C);
    const dim3 grid(box_blocks(n * nch), (unsigned)B);
    if (vec)
        hipLaunchKernelGGL((box_zero_kernel<float, 4>), grid, dim3(256), 0, (hipStream_t)stream, x, (long)ld, nch, z);
    else
        hipLaunchKernelGGL((box_zero_kernel<float, 1>), grid, dim3(256), 0, (hipStream_t)stream, x, (long)ld, nch, z);
    return dlcs_launch_status();
}

int dlcs_box_shift(const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int64_t C, int64_t B, int64_t Dp,
                   int64_t Hp, int64_t Wp, int64_t D, int64_t H, int64_t W, int64_t sd, int64_t sh, int64_t sw,
                   int transpose, const float* residual, int64_t ld_res, int relu, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(src && dst && (const float*)dst != src && B > 0 && C > 0 && ld_src >= C && ld_dst >= C && D > 0 &&
                   H > 0 && W > 0 && sd >= 0 && sh >= 0 && sw >= 0 && (!residual || ld_res >= C) &&
                   (!transpose || (!residual && !relu)));
    long ld_max = ld_src > ld_dst ? ld_src : ld_dst;
    if (residual && ld_res > ld_max) ld_max = ld_res;
    // the shifted box stays inside the padded grid: D + sd <= Dp, ... (no overflow: all < 2^30 is checked first)
    if (!box_grid_ok(Dp, Hp, Wp, D, H, W) || sd >= (1L << 30) || sh >= (1L << 30) || sw >= (1L << 30) ||
        D + sd > Dp || H + sh > Hp || W + sw > Wp || B > (1L << 20) || C > (1L << 20) || ld_max >= (1L << 30) ||
        B * Dp * Hp * Wp > (1L << 62) / ld_max)
        return DLCS_ERR_UNSUPPORTED_SIZE;
    const bool vec = C % 4 == 0 && ld_src % 4 == 0 && ld_dst % 4 == 0 && al16(src) && al16(dst) &&
                     (!residual || (ld_res % 4 == 0 && al16(residual)));
    ShiftDims s{(int)Dp, (int)Hp, (int)Wp, (int)D, (int)H, (int)W, (int)sd, (int)sh, (int)sw, (int)(vec ? C / 4 : C),
                B * Dp * Hp * Wp, (long)ld_src, (long)ld_dst, (long)ld_res};
    const dim3 grid(box_blocks(s.rows * s.nch)), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (vec && transpose) hipLaunchKernelGGL((box_shift_kernel<4, true>), grid, block, 0, st, src, dst, residual, relu, s);
    else if (vec) hipLaunchKernelGGL((box_shift_kernel<4, false>), grid, block, 0, st, src, dst, residual, relu, s);
    else if (transpose) hipLaunchKernelGGL((box_shift_kernel<1, true>), grid, block, 0, st, src, dst, residual, relu, s);
    else hipLaunchKernelGGL((box_shift_kernel<1, false>), grid, block, 0, st, src, dst, residual, relu, s);
    return dlcs_launch_status();
}

int dlcs_box_zero_bf16(void* x, int64_t ld, int64_t C, int64_t B, int64_t Dp, int64_t Hp, int64_t Wp, int64_t D,
                       int64_t H, int64_t W, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(x && B > 0 && C > 0 && ld >= C && D > 0 && H > 0 && W > 0);
    if (!box_grid_ok(Dp, Hp, Wp, D, H, W) || B > 65535 || C >= (1L << 30)) return DLCS_ERR_UNSUPPORTED_SIZE;
    ZeroDims z{(int)Dp, (int)Hp, (int)Wp, (int)D, (int)H, (int)W, (Dp - D) * Hp * Wp, D * (Hp - H) * Wp, D * H * (Wp - W)};
    const long n = z.n1 + z.n2 + z.n3;
    if (n == 0) return 0;
    const bool vec = C % 8 == 0 && ld % 8 == 0 && al16(x);
    const int nch = (int)(vec ? C / 8 : C);
    const dim3 grid(box_blocks(n * nch), (unsigned)B);
    if (vec)
        hipLaunchKernelGGL((box_zero_kernel<bf16, 8>), grid, dim3(256), 0, (hipStream_t)stream, (bf16*)x, (long)ld, nch, z);
    else
        hipLaunchKernelGGL((box_zero_kernel<bf16, 1>), grid, dim3(256), 0, (hipStream_t)stream, (bf16*)x, (long)ld, nch, z);
    return dlcs_launch_status();
}

}  // extern "C"
