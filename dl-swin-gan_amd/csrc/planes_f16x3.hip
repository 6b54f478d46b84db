// The plane utilities of the 2-plane f16 split (f16x3_common.h): max |x| words, the split,
// column-sum partials, the 160 x 160 conv weights' packing, and the bound of a tensor yet to be produced.
// Planes written by the producing kernel (out_planes of the conv / K = 160 GEMM):
// the scale must be known before the output exists, so it comes from an upper
// bound B >= max|out| written into the trailer beforehand (dlcs_planes_bound:
// B = c0 m0 n0 + c1 m1 n1 + cv max|vec|, with m the inputs' max |.| and n an
// operator norm, the max absolute row sum of the weights: |W x + b + r| <=
// ||W||_inf max|x| + max|b| + max|r|).  Any B >= max|out| gives the split's
// guarantee (u = s x < 2^14, no overflow); a loose B only lowers the level below
// which the low plane goes subnormal -- |x| >= 2^-17 B keep 22 bits and smaller
// values an absolute error <= 2^-38 B.
#include "f16x3_common.h"

namespace {
// max over rows r < R of sum_{o < no} sum_{i < ni} |w[r rs + o os + i]| -> *out (float
// bits, zeroed before), fixed-order sums (run-to-run deterministic): rows of up to
// 2048 elements one wave each (grid-stride), longer rows (a conv weight: 4320) a
// workgroup each; one atomicMax per workgroup (10240 per-row atomics on one word
// serialised to ~120 us)
template <bool ROWBLK>
__global__ void __launch_bounds__(256) absrow_max_kernel(const float* w, int R, long rs, int no, long os, int ni,
                                                         unsigned* out) {
    const int n = no * ni;
    float best = 0.0f;
    if (ROWBLK) {
        const float* row = w + (long)blockIdx.x * rs;
        float acc = 0.0f;
        for (int k = threadIdx.x; k < n; k += 256) acc += fabsf(row[(long)(k / ni) * os + k % ni]);
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);
        __shared__ float red[4];
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
        __syncthreads();
        best = (red[0] + red[1]) + (red[2] + red[3]);
    } else {
        const int lane = threadIdx.x & 63;
        for (int r = blockIdx.x * 4 + (int)(threadIdx.x >> 6); r < R; r += gridDim.x * 4) {
            const float* row = w + (long)r * rs;
            float acc = 0.0f;
            for (int k = lane; k < n; k += 64) acc += fabsf(row[(long)(k / ni) * os + k % ni]);
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);
            best = fmaxf(best, acc);
        }
        __shared__ float redm[4];
        if (lane == 0) redm[threadIdx.x >> 6] = best;
        __syncthreads();
        best = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
    }
    if (threadIdx.x == 0 && best > 0.0f) atomicMax(out, __float_as_uint(best));
}

// the trailer word of a split2 image <- bits of B (see above), rounded up by 2^-10
// for the fp32 rounding of the sums; the zero row after the trailer as split2 writes it
__global__ void __launch_bounds__(256) planes_bound_kernel(unsigned* trailer, const unsigned* m0, const unsigned* n0,
                                                           float c0, const unsigned* m1, const unsigned* n1, float c1,
                                                           const float* vec, int nvec, float cv) {
    float vm = 0.0f;
    for (int i = threadIdx.x; i < nvec; i += 256) vm = fmaxf(vm, fabsf(vec[i]));
    __shared__ float red[256];
    red[threadIdx.x] = vm;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x < 40)
        *reinterpret_cast<u32x4_h3*>(reinterpret_cast<char*>(trailer) + 256 + threadIdx.x * 16) = (u32x4_h3)0u;
    if (threadIdx.x == 0) {
        auto f = [](const unsigned* p) { return p ? __uint_as_float(*p) : 1.0f; };
        float b = cv * red[0];
        if (m0) b += c0 * f(m0) * f(n0);
        if (m1) b += c1 * f(m1) * f(n1);
        b *= 1.0f + 0.0009765625f;
        *trailer = b > 0.0f ? __float_as_uint(b) : 0u;
    }
}

// max |x| over rows x 160 channels of a row-major [rows][ld] fp32 tensor, as
// float bits (non-negative floats order as unsigned ints); *out zeroed before
__global__ void __launch_bounds__(256) absmax_kernel(const float* x, long rows, int ld, unsigned* out) {
    float m = 0.0f;
    const long stride = (long)gridDim.x * blockDim.x;
    if (ld == 160) {                                    // contiguous: a flat float4 stream, 4 loads in flight
        const f32x4_t* v = reinterpret_cast<const f32x4_t*>(x);
        const long n = rows * 40;
        long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
        for (; i + 3 * stride < n; i += 4 * stride) {
            const f32x4_t a0 = v[i], a1 = v[i + stride], a2 = v[i + 2 * stride], a3 = v[i + 3 * stride];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                m = fmaxf(m, fmaxf(fmaxf(fabsf(a0[e]), fabsf(a1[e])), fmaxf(fabsf(a2[e]), fabsf(a3[e]))));
        }
        for (; i < n; i += stride) {
            const f32x4_t a = v[i];
            m = fmaxf(m, fmaxf(fmaxf(fabsf(a[0]), fabsf(a[1])), fmaxf(fabsf(a[2]), fabsf(a[3]))));
        }
    } else {
        for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < rows * 40; i += stride) {
            const unsigned r = (unsigned)(i / 40), c = (unsigned)(i % 40);
            const f32x4_t a = *reinterpret_cast<const f32x4_t*>(x + (long)r * ld + c * 4);
            m = fmaxf(m, fmaxf(fmaxf(fabsf(a[0]), fabsf(a[1])), fmaxf(fabsf(a[2]), fabsf(a[3]))));
        }
    }
    __shared__ float red[4];
    block_max_to(out, m, red);
}

// x [rows][ld] fp32 (160 channels) -> XP [rows][320] f16 (per 32-channel chunk:
// xh then xl); a thread handles 8 channels of a row per item, its channel group
// fixed (the grid stride is a multiple of 20), four items in flight per
// iteration (round 4's one-item loop ran at 3.5-4.8 TB/s on the 550 MB tensors).
// CS: the column sums of x (a conv bias gradient) from the same read, per block
// in a fixed thread order into cpart[block][160] -- summed by
// colsum_parts_kernel in a fixed order (run-to-run deterministic; round 4's
// per-block float atomics on 160 addresses from 8192 blocks cost ~80 us).
// Block 0 also writes the zero row after the trailer (dlcs_split2_f16_bytes).
constexpr int kSplit2Blocks = 2045;                 // 5 x 409: stride 523,520 = 20 x 26,176 threads
template <bool CS>
__global__ void __launch_bounds__(256) split2_f16_kernel(const float* x, long rows, int ld, const unsigned* maxbits,
                                                         f16* xp, float* cpart) {
    const float s = f16x3_scale(*maxbits);
    if (blockIdx.x == 0 && threadIdx.x < 40)            // the zero row after the trailer
        *reinterpret_cast<u32x4_h3*>(reinterpret_cast<char*>(xp) + rows * 640 + 256 + threadIdx.x * 16) = (u32x4_h3)0u;
    float cs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const long stride = (long)gridDim.x * blockDim.x;
    const long gt = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const int c8 = (int)(gt % 20) * 8;
    auto put = [&](long r, const f32x4_t& v0, const f32x4_t& v1) {
        f16x8_t h, l;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xv = e < 4 ? v0[e] : v1[e - 4];
            if (CS) cs[e] += xv;
            const float u = xv * s;
            const f16 hv = (f16)u;
            h[e] = hv;
            l[e] = (f16)(u - (float)hv);
        }
        f16* dst = xp + r * 320 + (c8 >> 5) * 64 + (c8 & 31);
        *reinterpret_cast<f16x8_t*>(dst) = h;
        *reinterpret_cast<f16x8_t*>(dst + 32) = l;
    };
    // the stride is 20 x rs threads: this thread's rows are r0, r0 + rs, ... (no division per item)
    const long rs = stride / 20;
    long r = gt / 20;
    for (; r + 3 * rs < rows; r += 4 * rs) {
        f32x4_t v[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float* src = x + (r + u * rs) * ld + c8;
            v[u][0] = *reinterpret_cast<const f32x4_t*>(src);
            v[u][1] = *reinterpret_cast<const f32x4_t*>(src + 4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) put(r + u * rs, v[u][0], v[u][1]);
    }
    for (; r < rows; r += rs)
        put(r, *reinterpret_cast<const f32x4_t*>(x + r * ld + c8), *reinterpret_cast<const f32x4_t*>(x + r * ld + c8 + 4));
    if (CS) {
        __shared__ float part[256 * 8];
#pragma unroll
        for (int e = 0; e < 8; ++e) part[threadIdx.x * 8 + e] = cs[e];
        __syncthreads();
        if (threadIdx.x < 160) {
            const int c = threadIdx.x, g = c >> 3;
            const int t0 = (int)((g - (long)blockIdx.x * 256 % 20 + 20) % 20);   // first thread of group g
            float sum = 0.0f;
            for (int t = t0; t < 256; t += 20) sum += part[t * 8 + (c & 7)];
            cpart[blockIdx.x * 160 + c] = sum;
        }
    }
}

// colsum[c] += sum over blocks of cpart[block][c], one workgroup per channel, fixed order
__global__ void __launch_bounds__(256) colsum_parts_kernel(const float* cpart, int nblk, float* colsum) {
    const int c = blockIdx.x;
    float v = 0.0f;
    for (int b = threadIdx.x; b < nblk; b += 256) v += cpart[b * 160 + c];
    __shared__ float red[256];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) colsum[c] += red[0];
}

// workgroups of the split (one row of 160 column-sum partials each): the grid stride
// is a multiple of 20 (each thread keeps one 8-channel group)
static unsigned split2_blocks(long rows) {
    return (unsigned)std::min<long>(kSplit2Blocks, std::max<long>(5, (rows * 20 + 255) / 256 / 5 * 5));
}

// weights [160][160][27] fp32 -> WP [5][27][160][64]; mode 0 (forward): rows co,
// contracted ci, tap t; mode 1 (dgrad): rows ci, contracted co, tap 26 - t
__global__ void pack_weights_f16x3_kernel(const float* w, const unsigned* maxbits, f16* wp, int mode) {
    const float s = f16x3_scale(*maxbits);
    const long n = 27L * 160 * 160;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % 160);
        const int r = (int)((i / 160) % 160);
        const int tap = (int)(i / (160L * 160));
        const float u = s * (mode == 0 ? w[((long)r * 160 + c) * 27 + tap] : w[((long)c * 160 + r) * 27 + (26 - tap)]);
        const f16 hv = (f16)u;
        const long base = (((long)(c >> 5) * 27 + tap) * 160 + r) * 64 + (c & 31);
        wp[base] = hv;
        wp[base + 32] = (f16)(u - (float)hv);
    }
}

// max |x| over n floats into *out (float bits; atomicMax, *out zeroed before)
__global__ void __launch_bounds__(256) absmax_flat_kernel(const float* x, long n, unsigned* out) {
    float m = 0.0f;
    const long stride = (long)gridDim.x * blockDim.x;
    const long n4 = n >> 2;
    const f32x4_t* v = reinterpret_cast<const f32x4_t*>(x);
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += stride) {
        const f32x4_t a = v[i];
        m = fmaxf(m, fmaxf(fmaxf(fabsf(a[0]), fabsf(a[1])), fmaxf(fabsf(a[2]), fabsf(a[3]))));
    }
    for (long i = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride) m = fmaxf(m, fabsf(x[i]));
    __shared__ float red[4];
    block_max_to(out, m, red);
}

}  // namespace

namespace dlcs_internal {
int launch_colsum_parts(const float* cpart, int nblk, float* colsum, hipStream_t st) {
    hipLaunchKernelGGL(colsum_parts_kernel, dim3(160), dim3(256), 0, st, cpart, nblk, colsum);
    return dlcs_launch_status();
}
int launch_absmax_flat(const float* x, long n, unsigned* out, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL(absmax_flat_kernel, dim3(grid), dim3(256), 0, st, x, n, out);
    return dlcs_launch_status();
}
}  // namespace dlcs_internal

extern "C" {

// planes [rows][320] f16, the 256-B trailer (max |x| bits in its first word) and one
// 640-B zero row (the weight gradient's source for halo voxels off the grid)
size_t dlcs_split2_f16_bytes(int64_t rows) { return (size_t)rows * 640 + 256 + 640; }

size_t dlcs_split2_f16_workspace_bytes(int64_t rows, int has_colsum) {
    return has_colsum ? (size_t)split2_blocks(rows) * 160 * sizeof(float) : 0;
}

int dlcs_split2_f16(const float* x, int64_t rows, int64_t ld, void* planes, int have_max, float* colsum,
                    void* workspace, size_t workspace_bytes, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(x && planes && rows > 0 && ld >= 160);
    if (ld % 4 || ((uintptr_t)x & 15) || ((uintptr_t)planes & 15)) return DLCS_ERR_UNSUPPORTED_SIZE;
    if (!ws_ok(workspace, workspace_bytes, dlcs_split2_f16_workspace_bytes(rows, colsum != nullptr)))
        return DLCS_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    unsigned* mx = planes_trailer(planes, rows);
    if (!have_max) {
        if (hipMemsetAsync(mx, 0, 4, st) != hipSuccess) return dlcs_launch_status();
        hipLaunchKernelGGL(absmax_kernel, dim3(std::min(h3_grid(rows * 10), 2048u)), dim3(256), 0, st, x, (long)rows,
                           (int)ld, mx);
    }
    const unsigned g = split2_blocks(rows);
    if (colsum) {
        float* cpart = static_cast<float*>(workspace);          // one row of 160 per block
        hipLaunchKernelGGL(split2_f16_kernel<true>, dim3(g), dim3(256), 0, st, x, (long)rows, (int)ld,
                           (const unsigned*)mx, (f16*)planes, cpart);
        hipLaunchKernelGGL(colsum_parts_kernel, dim3(160), dim3(256), 0, st, (const float*)cpart, (int)g, colsum);
    } else {
        hipLaunchKernelGGL(split2_f16_kernel<false>, dim3(g), dim3(256), 0, st, x, (long)rows, (int)ld,
                           (const unsigned*)mx, (f16*)planes, nullptr);
    }
    return dlcs_launch_status();
}

size_t dlcs_conv3d_pack_weights_f16x3_bytes(void) { return kW3Bytes + 256; }

int dlcs_conv3d_pack_weights_f16x3(const float* w, int mode, void* packed, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(w && packed && (mode == 0 || mode == 1));
    if (((uintptr_t)w & 15) || ((uintptr_t)packed & 15)) return DLCS_ERR_UNSUPPORTED_SIZE;
    hipStream_t st = (hipStream_t)stream;
    unsigned* mx = (unsigned*)((char*)packed + kW3Bytes);
    if (hipMemsetAsync(mx, 0, 4, st) != hipSuccess) return dlcs_launch_status();
    hipLaunchKernelGGL(absmax_kernel, dim3(h3_grid(4320L * 10)), dim3(256), 0, st, w, 4320L, 160, mx);
    hipLaunchKernelGGL(pack_weights_f16x3_kernel, dim3(h3_grid(27L * 160 * 160)), dim3(256), 0, st, w,
                       (const unsigned*)mx, (f16*)packed, mode);
    return dlcs_launch_status();
}

int dlcs_abs_row_sum_max(const float* w, int64_t rows, int64_t row_stride, int64_t n_outer, int64_t outer_stride,
                         int64_t inner, unsigned* out, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(w && out && rows > 0 && rows < (1L << 31) && n_outer > 0 && inner > 0 && n_outer * inner < (1L << 31));
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, 4, st) != hipSuccess) return dlcs_launch_status();
    if (n_outer * inner > 2048)
        hipLaunchKernelGGL(absrow_max_kernel<true>, dim3((unsigned)rows), dim3(256), 0, st, w, (int)rows,
                           (long)row_stride, (int)n_outer, (long)outer_stride, (int)inner, out);
    else
        hipLaunchKernelGGL(absrow_max_kernel<false>, dim3((unsigned)std::min<int64_t>((rows + 3) / 4, 256)), dim3(256), 0, st,
                           w, (int)rows, (long)row_stride, (int)n_outer, (long)outer_stride, (int)inner, out);
    return dlcs_launch_status();
}

int dlcs_planes_bound(void* planes, int64_t rows, const unsigned* m0, const unsigned* n0, float c0,
                      const unsigned* m1, const unsigned* n1, float c1, const float* vec, int64_t nvec, float cvec,
                      dlcs_stream_t stream) {
    DLCS_CHECK_ARG(planes && rows > 0 && nvec >= 0 && nvec < (1L << 31) && (vec || nvec == 0));
    if ((uintptr_t)planes & 15) return DLCS_ERR_UNSUPPORTED_SIZE;
    hipLaunchKernelGGL(planes_bound_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream,
                       planes_trailer(planes, rows), m0, n0, c0, m1, n1, c1, vec, (int)nvec, cvec);
    return dlcs_launch_status();
}

int dlcs_absmax_f32(const float* x, int64_t n, unsigned* out, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(x && out && n >= 0);
    if ((uintptr_t)x & 15) return DLCS_ERR_UNSUPPORTED_SIZE;
    if (n == 0) return 0;
    hipLaunchKernelGGL(absmax_flat_kernel, dim3(std::min(h3_grid(n / 4 + 1), 1024u)), dim3(256), 0,
                       (hipStream_t)stream, x, (long)n, out);
    return dlcs_launch_status();
}

}  // extern "C"
