// ---------------------------------------------------------------- fp32 conv on fp16 MFMAs (2-plane split)
// The fp32 Conv3d 160 -> 160 (forward / dgrad) computed with fp16 matrix cores
// to fp32 accuracy.  Every fp32 operand tensor gets ONE power-of-two scale s
// (max|s x| in (2^13, 2^14]) and is split into two fp16 planes,
//   u = s x,  xh = f16(u),  xl = f16(u - xh)        (u - xh exact in fp32)
// so xh + xl carries 22 significant bits; the product is the three plane
// products hh + hl + lh (the dropped xl wl is 2^-22 relative), each exact in
// the fp32 MFMA accumulator, and the tile is rescaled by 1 / (s_x s_w) (exact)
// before the epilogue.  tools/f16x3_numerics.py: NRMSE vs float64 3.5e-7 on
// activations AND on 1e-7-sized gradients with a 1e6 dynamic range -- PyTorch's
// own fp32 conv gives 3.6e-7; without the scale the gradient case is 3e-4.
// Three fp16 MFMAs per fp32 product: half the matrix-core work of the 3-plane
// bf16 split (conv3d_x6.inc, six products for the same accuracy).
//
// Operands: activations XP [rows][320] f16 (per 32-channel chunk cc: xh of the
// 32 channels, then xl: one 128-B row segment), max|x| bits in a trailer
// (dlcs_split2_f16); weights WP [5 cc][27 tap][160 rows][64] (wh 32 | wl 32),
// trailer max|w| (dlcs_conv3d_pack_weights_f16x3, mode 0 forward, 1 dgrad).
//
// Kernel: workgroup tile, waves and epilogue of the fp32 / x6 kernels (256
// voxels x 160 channels, 8 waves x 4 x 5 tiles of 16x16, v_mfma_f32_16x16x32_f16,
// K = 32 channels of one plane per MFMA).  Steps: 5 chunks x 14 tap pairs (the
// 14th a single tap) = 70 barriers.  LDS: the chunk's halo image X [600][64]
// (76.8 KB, single-buffered: the next chunk waits in registers and is stored
// behind an extra barrier at the seam) and two weight slots of two tap slices
// [160][64] (2 x 40 KB, DMA'd one step ahead): 156.8 KB.  Both images are
// 128-B rows of eight 16-B chunks XOR-swizzled so every ds_read_b128 fragment
// read is conflict-free (tools/f16x3_swizzle.py, exact search):
//   halo row (hy, hx): chunk ^ (2 (hy & 3) + ((hx >> 1) & 1))
//   weight row co:     chunk ^ ((co >> 1) & 7)
// Workgroups are numbered XCD-major (block b runs on XCD b % 8; each XCD gets
// one contiguous run of tiles), so neighbouring tiles share their halo rows in
// the same L2.
typedef _Float16 f16;
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned u32x4_h3 __attribute__((ext_vector_type(4)));

DLCS_DEV void mfma16h(f32x4_t& acc, const f16x8_t& a, const f16x8_t& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
}

// the power-of-two scale of a tensor from the bits of max|x| (see the header)
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
// (split2_f16_kernel's layout: per 32-channel chunk the high plane, then the low)
typedef _Float16 f16x4_h3 __attribute__((ext_vector_type(4)));
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
    f16x4_h3 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float u = v[e] * s;
        h[e] = (f16)u;
        l[e] = plane_lo(u, h[e]);
    }
    f16* d = xp + r * 320 + (c >> 5) * 64 + (c & 31);
    *reinterpret_cast<f16x4_h3*>(d) = h;
    *reinterpret_cast<f16x4_h3*>(d + 32) = l;
}

// (hi + lo) / s of 4 channels c.. of row r of a split2 image (rinv = 1 / s): the
// value to 2^-22 relative (+ 2^-38 of the image's bound), hi + lo exact in fp32
DLCS_DEV f32x4_t get_planes4(const f16* xp, long r, int c, float rinv) {
    const f16* d = xp + r * 320 + (c >> 5) * 64 + (c & 31);
    const f16x4_h3 h = *reinterpret_cast<const f16x4_h3*>(d), l = *reinterpret_cast<const f16x4_h3*>(d + 32);
    f32x4_t v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ((float)h[e] + (float)l[e]) * rinv;
    return v;
}

// Planes written by the producing kernel (out_planes of the conv / K = 160 GEMM):
// the scale must be known before the output exists, so it comes from an upper
// bound B >= max|out| written into the trailer beforehand (dlcs_planes_bound:
// B = c0 m0 n0 + c1 m1 n1 + cv max|vec|, with m the inputs' max |.| and n an
// operator norm, the max absolute row sum of the weights: |W x + b + r| <=
// ||W||_inf max|x| + max|b| + max|r|).  Any B >= max|out| gives the split's
// guarantee (u = s x < 2^14, no overflow); a loose B only lowers the level below
// which the low plane goes subnormal -- |x| >= 2^-17 B keep 22 bits and smaller
// values an absolute error <= 2^-38 B.
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

constexpr int kH3Halo = kHalo * 64;            // f16 in the halo image (76.8 KB)
constexpr int kH3Tap = 160 * 64;               // f16 in one tap slice (20 KB)
constexpr int kH3Slot = 2 * kH3Tap;            // two tap slices per step
constexpr int kH3Steps = 5 * 14;

struct ConvH3Args {
    const f16* xp; const f16* wp; const unsigned* xmax; const unsigned* wmax;
    const float* bias; float* out; const float* mask; const float* res;
    int B, D, H, W;
    int cout_ld, mask_ld, res_ld, accumulate, relu_out;
    float res_scale;
    unsigned* omax;                                 // optional max |out| (float bits) for the next split
    // tail split (conv_f16x3_launch): workgroup w computes tile tail_base + w / 5
    // over input chunk w % 5 only and stores the raw partial tile to part + w 256 x 160
    float* part; int tail_base;
    f16* oplanes; const unsigned* opmax;            // optional split2 image of out (scale from the trailer's bound)
    float* cpart;                                   // optional per-tile column sums of out [tiles][160] (colsum)
    const void* mplanes;                            // kEpiMask: the mask as split2 planes of a non-negative tensor
    int stamp;                                      // DIAG build: record s_memtime stamps (g_h3_stamps)
    int exp;                                        // DIAG build: timing experiments (DLCS_H3_EXP bits, results invalid)
};

#ifdef DLCS_DIAG_BUILD
// DIAG build: per workgroup (first 4096) the cycle counter at kernel entry, after the
// prologue barrier, after each of the 70 steps and after the epilogue (wave 0 lane 0)
__device__ unsigned long long g_h3_stamps[4096 * 73];
#define H3_STAMP(k) do { if (!TAIL && a.stamp && threadIdx.x == 0 && blockIdx.x < 4096) \
    g_h3_stamps[blockIdx.x * 73 + (k)] = __builtin_readcyclecounter(); } while (0)
#else
#define H3_STAMP(k) do { } while (0)
#endif

// Accumulation modes (FOLD; dlcs launch: DLCS_H3_FOLD, see conv_f16x3_launch).
// The matrix core's 16-bit-MFMA accumulate is not exactly rounded: it truncates
// toward -inf (tools/probe/mfma_chain.hip) -- about 0.007 ulp of the accumulator
// per MFMA into a large running sum, 0.1 x 2^-24 x rms per fresh six-product
// tile, the same sign for positive and negative results.  Invisible per element,
// that offset is coherent over the tensor and survives the network's column sums
// (bias and norm gradients over 3e5 voxels: 2e-5 there, tools/dgrad_diag.py).
//   0  plain running sum (the forward: its bias feeds no such sum);
//   3  (default for the masked, input-gradient launches) each wave's 16 output rows
//      take a pseudo-random sign (a hash of tile and wave): their A fragments are
//      XOR-negated for the whole sum and the epilogue restores the sign, so the
//      bias is +/- per voxel and cancels in any later sum over voxels -- column-sum
//      error 8.3e-7, PyTorch's fp32 conv 8.8e-7, at one XOR per fragment (+6 %
//      over plain).  Random, not by parity: a sign that repeats per 4x4x4 patch
//      becomes a coherent bias of the unembed's token gradient (norm gradients at
//      1.5e-5 NRMSE with it);
//   1  fold: each step's six plane products (both taps) run into fresh tiles that
//      the VALU adds to the running sum, odd steps on negated A fragments and
//      subtracted (the per-step biases alternate) -- the most accurate (element
//      NRMSE 1.9e-7, column sums 5e-7) but the temporaries spill (+23 %);
//   2  the running sum negated around odd steps, odd steps on negated A (+13 %:
//      the negations drain the matrix pipe).
// The tap count of a step is a compile-time constant (the 13 two-tap steps and the
// one-tap step of each chunk are separate instances).
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

template <int EPI, int FOLD, bool TAIL = false>
__global__ void __launch_bounds__(512) conv3d_k3_f16x3_kernel(ConvH3Args a) {
    __shared__ __attribute__((aligned(16))) f16 smem_h3[kH3Halo + 2 * kH3Slot];   // 156.8 KB
    f16* X = smem_h3;
    f16* Ws = X + kH3Halo;

    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int nYt = (nY + 1) >> 1, nXt = (nX + 1) >> 1;
    // XCD-major numbering: XCD x = b % 8 runs tiles [start(x), start(x) + count(x))
    const int nblk = a.B * nT * nYt * nXt;
    // virtual block vb: blockIdx.x, or a tail tile (one input chunk of it) of the split launch
    const int cc0 = TAIL ? (int)blockIdx.x % 5 : 0;
    const int cc1 = TAIL ? cc0 + 1 : 5;
    const int q8 = nblk >> 3, r8 = nblk & 7;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int vb = 0, b = 0, pt = 0, tyy = 0, txx = 0, t0 = 0, y0 = 0, x0 = 0;
    unsigned rsgn = 0;                                   // FOLD == 3: this tile's 16-bit row signs
    auto set_tile = [&](int v) {
        vb = v;
        const int xcd = vb & 7;
        int bid = xcd * q8 + min(xcd, r8) + (vb >> 3);
        txx = bid % nXt; bid /= nXt;
        tyy = bid % nYt; bid /= nYt;
        pt = bid % nT;
        b = bid / nT;
        t0 = pt * 4; y0 = tyy * 8; x0 = txx * 8;
        rsgn = ((unsigned)(vb * 8 + wave) * 0x9E3779B1u) >> 16;
    };
    set_tile(TAIL ? a.tail_base + (int)blockIdx.x / 5 : (int)blockIdx.x);
    const int pw = wave & 3, nh = wave >> 2;
    const int send = cc1 * 14;                          // one past the last step of this workgroup
    H3_STAMP(0);

    // halo pieces of this thread: 600 rows x 8 16-B chunks = 4800 (10 per thread,
    // piece k = threadIdx + 512 k).  Pieces k < 3 lie in the first two time slices
    // (rows < 200), which no tap reads after step 8 (taps 18..26 have kd = 2): the
    // next chunk's copies of them are DMA'd straight into the live image during
    // step 9; pieces 3..9 wait in registers from step 10 until the chunk seam.
    constexpr int HP = 10, HD = 3, HR = HP - HD;
    f16x8_t hr[HR];
    // source offset of halo piece k (-1 outside the volume), recomputed per chunk
    // (5 times per workgroup) rather than held in registers across the whole loop
    auto halo_off = [&](int k) {
        const int i = threadIdx.x + k * 512;
        int off = -1;
        if (i < kHalo * 8) {
            const int hv = i >> 3, c = i & 7;
            const int ht = hv / (kHaloY * kHaloX), hy = (hv / kHaloX) % kHaloY, hx = hv % kHaloX;
            const int t = t0 - 1 + ht, y = y0 - 1 + hy, x = x0 - 1 + hx;
            if (t >= 0 && t < a.D && y >= 0 && y < a.H && x >= 0 && x < a.W)
                off = (int)(brow(b, t, y, x, nT, nY, nX) * 320 + (c ^ f16x3_halo_swz(hy, hx)) * 8);
        }
        return off;
    };
    const unsigned xbase = lds_offset(X);
    auto dma_halo = [&](int cc) {                       // pieces 0 .. HD-1 (all below row 200)
        const f16* zrow = reinterpret_cast<const f16*>(g_wg_zero_row);
#pragma unroll
        for (int k = 0; k < HD; ++k) {
            const int off = halo_off(k);
            glds16(off >= 0 ? a.xp + cc * 64 + off : zrow, xbase + (unsigned)((k * 512 + wave * 64) * 16));
        }
    };
    auto load_halo = [&](int cc) {                      // pieces HD .. HP-1 into registers
#pragma unroll
        for (int k = 0; k < HR; ++k) {
            const int off = halo_off(HD + k);
            hr[k] = (f16x8_t)(f16)0.0f;
            if (off >= 0) hr[k] = *reinterpret_cast<const f16x8_t*>(a.xp + cc * 64 + off);
        }
    };
    // piece i -> LDS row i / 8, physical chunk i % 8 (the logical chunk was swizzled on the load side)
    auto store_halo = [&]() {
#pragma unroll
        for (int k = 0; k < HR; ++k) {
            const int i = threadIdx.x + (HD + k) * 512;
            if (i < kHalo * 8) *reinterpret_cast<f16x8_t*>(X + i * 8) = hr[k];
        }
    };
    // weight DMA of step s into slot s & 1: tap slices of 20 x 1 KB pieces;
    // piece wi (of 40) by wave wi % 8; LDS row r = 8 pp + lane / 8, physical
    // chunk lane % 8 <- logical chunk (lane % 8) ^ ((r >> 1) & 7)
    const unsigned wbase = lds_offset(Ws);
    unsigned woff[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int wi = k * 8 + wave, pp = wi % 20;
        const int r = pp * 8 + (lane >> 3), pc = lane & 7;
        woff[k] = (unsigned)((r * 64 + ((pc ^ ((r >> 1) & 7)) << 3)) * 2);
    }
    auto issue_w = [&](int s) {
        const int cc = s / 14, tp = s % 14;
        const int nt = tp == 13 ? 1 : 2;
        const unsigned dst = wbase + (unsigned)((s & 1) * kH3Slot * 2);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int wi = k * 8 + wave, ts = wi / 20, pp = wi % 20;
            if (ts < nt) {
                const f16* src = a.wp + ((long)cc * 27 + 2 * tp + ts) * kH3Tap;
                glds16_s(src, woff[k], dst + (unsigned)(ts * kH3Tap * 2 + pp * 1024));
            }
        }
    };

    f32x4_t acc[4][5];

    const int pyy = pw >> 1, pxx = pw & 1;
    const int vq = lane & 15, cq = lane >> 4;
    const int ly = pyy * 4 + (vq >> 2), lx = pxx * 4 + (vq & 3);
    const int hb0 = ly * kHaloX + lx;
    const int corow = nh * 80 + vq;
    // FOLD == 3: the 16-bit sign pattern of this wave's 16 rows (a hash of tile and wave)
    // (rsgn: set per tile by set_tile)
    const int wsw = (vq >> 1) & 7;                      // weight row swizzle (co & 15 = vq)
    const int bofh = (cq ^ wsw) << 3, bofl = ((4 + cq) ^ wsw) << 3;

    auto mma = [&](const f16x8_t (&af)[4], const f16x8_t (&bfr)[5]) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) mfma16h(acc[i][j], af[i], bfr[j]);
    };
    // one tap's xh wh + xh wl + xl wh into fresh tiles, then acc += tile (fp32 VALU);
    // the A fragments (xh, xl of voxel row block i) are read per row block
    auto mma_fold = [&](const f16* pah, const f16* pal, const f16x8_t (&bh)[5], const f16x8_t (&bl)[5]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f16x8_t ahi = *reinterpret_cast<const f16x8_t*>(pah + i * (kHaloY * kHaloX * 64));
            const f16x8_t ali = *reinterpret_cast<const f16x8_t*>(pal + i * (kHaloY * kHaloX * 64));
            // column tiles in groups of 3 and 2 (12 temporary registers)
#pragma unroll
            for (int j0 = 0; j0 < 5; j0 += 5) {
                constexpr int G = 5;
                f32x4_t t[G];
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    if (j0 + j < 5) {
                        t[j] = (f32x4_t)0.0f;
                        mfma16h(t[j], ahi, bl[j0 + j]);
                    }
                }
#pragma unroll
                for (int j = 0; j < G; ++j)
                    if (j0 + j < 5) mfma16h(t[j], ali, bh[j0 + j]);
#pragma unroll
                for (int j = 0; j < G; ++j)
                    if (j0 + j < 5) mfma16h(t[j], ahi, bh[j0 + j]);
#pragma unroll
                for (int j = 0; j < G; ++j)
                    if (j0 + j < 5) acc[i][j0 + j] += t[j];
            }

        }
    };

#ifdef DLCS_DIAG_BUILD
    // DLCS_H3_EXP (DIAG timing experiments; the results are wrong): 1 no end-of-step
    // barrier, 2 no end-of-step vmcnt wait, 4 no MFMAs, 8 no weight DMA after the prologue
    const int xexp = a.exp;
#else
    constexpr int xexp = 0;
#endif
    if (wave >= 4) __builtin_amdgcn_s_setprio(1);
    // step s of chunk cc = s / 14 covers taps 2 tp, 2 tp + 1 (tp = s % 14; tap 26 alone at tp = 13)
    auto step = [&](int s, int cc, int tp, auto NTc) {
        constexpr int nt = decltype(NTc)::value;
        const bool seam = (nt == 1) && (s + 1 < send);
        if (tp == 9 && cc + 1 < cc1) dma_halo(cc + 1);     // rows < 200 are dead after step 8
        if (tp == 10 && cc + 1 < cc1) load_halo(cc + 1);
        if (FOLD == 1 && s + 1 < send && !(xexp & 8)) issue_w(s + 1);
        const f16* wsl = Ws + (s & 1) * kH3Slot;
        auto tap_a = [&](int ti, int plane) {
            const int tap = 2 * tp + ti;
            const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
            const int hsw = f16x3_halo_swz(ly + kh, lx + kw);
            return X + (hb0 + (kd * kHaloY + kh) * kHaloX + kw) * 64 + (((4 * plane + cq) ^ hsw) << 3);
        };
        auto read_a = [&](const f16* p, f16x8_t (&af)[4]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const f16x8_t*>(p + i * (kHaloY * kHaloX * 64));
        };
        auto read_b = [&](int ti, int bof, f16x8_t (&bfr)[5]) {
            const f16* wb = wsl + ti * kH3Tap + corow * 64 + bof;
#pragma unroll
            for (int j = 0; j < 5; ++j) bfr[j] = *reinterpret_cast<const f16x8_t*>(wb + j * 16 * 64);
        };
        f16x8_t ah[4], al[4], bh[5], bl[5];
        if constexpr (FOLD == 1) {
            // both taps of the step into one fresh tile per row block (6 products per
            // tile between VALU adds): the B fragments of both taps stay in registers
            f16x8_t bh2[5], bl2[5];
            read_b(0, bofh, bh);
            read_b(0, bofl, bl);
            if constexpr (nt == 2) {
                read_b(1, bofh, bh2);
                read_b(1, bofl, bl2);
            }
            // odd steps: negated A planes, tile subtracted (the -inf bias flips sign)
            const unsigned nm = (tp & 1) ? 0x80008000u : 0u;
            const float sg = (tp & 1) ? -1.0f : 1.0f;
            auto negx = [&](f16x8_t v) {
                return __builtin_bit_cast(f16x8_t, __builtin_bit_cast(u32x4_h3, v) ^ nm);
            };
            const f16* pa0h = tap_a(0, 0);
            const f16* pa0l = tap_a(0, 1);
            const f16* pa1h = nt == 2 ? tap_a(1, 0) : pa0h;
            const f16* pa1l = nt == 2 ? tap_a(1, 1) : pa0l;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                constexpr int RS = kHaloY * kHaloX * 64;
                const f16x8_t ah0 = negx(*reinterpret_cast<const f16x8_t*>(pa0h + i * RS));
                const f16x8_t al0 = negx(*reinterpret_cast<const f16x8_t*>(pa0l + i * RS));
                f32x4_t t[5];
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    t[j] = (f32x4_t)0.0f;
                    mfma16h(t[j], ah0, bl[j]);
                }
#pragma unroll
                for (int j = 0; j < 5; ++j) mfma16h(t[j], al0, bh[j]);
#pragma unroll
                for (int j = 0; j < 5; ++j) mfma16h(t[j], ah0, bh[j]);
                if constexpr (nt == 2) {
                    const f16x8_t ah1 = negx(*reinterpret_cast<const f16x8_t*>(pa1h + i * RS));
                    const f16x8_t al1 = negx(*reinterpret_cast<const f16x8_t*>(pa1l + i * RS));
#pragma unroll
                    for (int j = 0; j < 5; ++j) mfma16h(t[j], ah1, bl2[j]);
#pragma unroll
                    for (int j = 0; j < 5; ++j) mfma16h(t[j], al1, bh2[j]);
#pragma unroll
                    for (int j = 0; j < 5; ++j) mfma16h(t[j], ah1, bh2[j]);
                }
#pragma unroll
                for (int j = 0; j < 5; ++j) acc[i][j] += t[j] * sg;
            }
        } else {
            // FOLD == 2: odd steps add their (negated-A) products into the negated running
            // sum -- the truncation bias alternates with no temporaries (acc negated twice
            // per odd step, 80 VALU ops)
            const bool flip = FOLD == 2 && (tp & 1);
            // FOLD == 3: output rows (voxels) on pseudo-randomly negated A rows for the
            // whole sum (rsgn), the sign restored in the epilogue: the bias takes a random
            // sign per voxel and cancels in every later sum over voxels, at one XOR per
            // fragment.  Random, not by parity: a pattern that repeats per 4x4x4 patch
            // turns into a coherent bias of the unembed's token gradient.
            const unsigned rowm = (FOLD == 3 && ((rsgn >> vq) & 1)) ? 0x80008000u : 0u;
            auto negate_acc = [&]() {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 5; ++j) acc[i][j] = -acc[i][j];
            };
            const unsigned nm = flip ? 0x80008000u : 0u;
            auto nega = [&](f16x8_t (&af)[4]) {
                if constexpr (FOLD == 2 || FOLD == 3) {
                    const unsigned m = FOLD == 2 ? nm : rowm;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        af[i] = __builtin_bit_cast(f16x8_t, __builtin_bit_cast(u32x4_h3, af[i]) ^ m);
                }
            };
            if (flip) negate_acc();
#pragma unroll
            for (int ti = 0; ti < nt; ++ti) {
                read_a(tap_a(ti, 0), ah);
                nega(ah);
                read_b(ti, bofh, bh);
                read_b(ti, bofl, bl);
                if (xexp & 4) {                             // DIAG: operands consumed, no matrix work
                    read_a(tap_a(ti, 1), al);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        acc[i][0][0] += (float)ah[i][0] + (float)al[i][1] + (float)bh[i][2] + (float)bl[i][3] + (float)bh[4][i] + (float)bl[4][i];
                    continue;
                }
                mma(ah, bh);                                // xh wh
                // the next step's weight DMA issued among the first MFMA group (-0.7 / -2 %
                // fwd / dgrad against issuing it before the step's first LDS reads)
                if (ti == 0 && s + 1 < send && !(xexp & 8)) issue_w(s + 1);
                read_a(tap_a(ti, 1), al);
                nega(al);
                mma(ah, bl);                                // xh wl
                mma(al, bh);                                // xl wh
            }
            if (flip) negate_acc();
        }
        if (seam) {
            __syncthreads();                                // every wave is done with this chunk's halo
            store_halo();
        }
        if (!(xexp & 2)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // step s+1's weight slices have landed
        if (seam || !(xexp & 1)) __syncthreads();
        H3_STAMP(2 + s);
    };
    dma_halo(cc0);
    load_halo(cc0);
    issue_w(cc0 * 14);
    store_halo();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    H3_STAMP(1);

#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) acc[i][j] = (f32x4_t)0.0f;
    for (int cc = cc0; cc < cc1; ++cc) {
        for (int tp = 0; tp < 13; ++tp) step(cc * 14 + tp, cc, tp, std::integral_constant<int, 2>{});
        step(cc * 14 + 13, cc, 13, std::integral_constant<int, 1>{});
    }
    const float inv = 1.0f / (f16x3_scale(*a.xmax) * f16x3_scale(*a.wmax));   // exact: a power of two
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)                 // output row 4 (lane / 16) + r
                acc[i][j][r] *= (FOLD == 3 && ((rsgn >> (4 * (lane >> 4) + r)) & 1)) ? -inv : inv;
    if constexpr (TAIL) {                               // tail split: the raw partial tile [256][160]
        float* pp = a.part + (long)blockIdx.x * 256 * 160;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    pp[(pw * 64 + i * 16 + (lane >> 4) * 4 + r) * 160 + nh * 80 + j * 16 + (lane & 15)] = acc[i][j][r];
        return;
    }
    ConvF32Args ea{};
    ea.bias = a.bias; ea.out = a.out; ea.mask = a.mask; ea.res = a.res;
    ea.cout_ld = a.cout_ld; ea.mask_ld = a.mask_ld; ea.res_ld = a.res_ld; ea.accumulate = a.accumulate;
    ea.relu_out = a.relu_out; ea.res_scale = a.res_scale; ea.omax = a.omax; ea.mplanes = a.mplanes;
    if constexpr (EPI == kEpiRes || EPI == kEpiMask)
        conv_epilogue_h3<EPI, 2>(ea, acc, reinterpret_cast<float*>(smem_h3), pw, nh * 80, lane, b, pt, tyy * 2, txx * 2,
                                 nT, nY, nX, a.oplanes, a.opmax, a.cpart ? a.cpart + (long)vb * 160 : nullptr);
    else
        conv_epilogue_f32<EPI>(ea, acc, reinterpret_cast<float*>(smem_h3), pw, nh * 80, lane, b, pt, tyy * 2, txx * 2,
                               nT, nY, nX);
    H3_STAMP(72);
}

// Tail of the split launch: out tile = the five chunk partials summed in a fixed
// order (run-to-run deterministic), then the epilogue of conv_epilogue_f32.
__global__ void __launch_bounds__(256) conv_f16x3_tail_reduce_kernel(ConvH3Args a, int ntail) {
    __shared__ float red[4];
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int nYt = (nY + 1) >> 1, nXt = (nX + 1) >> 1;
    const int nblk = a.B * nT * nYt * nXt;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    float vmax = 0.0f;
    if (i < (long)ntail * 256 * 40) {
        const int t = (int)(i / (256 * 40)), rem = (int)(i % (256 * 40));
        const int vl = rem / 40, c = (rem % 40) * 4;
        f32x4_t v = (f32x4_t)0.0f;
#pragma unroll
        for (int w = 0; w < 5; ++w) v += *reinterpret_cast<const f32x4_t*>(a.part + ((long)(t * 5 + w) * 256 + vl) * 160 + c);
        const int vb = a.tail_base + t;
        const int q8 = nblk >> 3, r8 = nblk & 7, xcd = vb & 7;
        int bid = xcd * q8 + min(xcd, r8) + (vb >> 3);
        const int txx = bid % nXt; bid /= nXt;
        const int tyy = bid % nYt; bid /= nYt;
        const int pt = bid % nT;
        const int b = bid / nT;
        const int pwv = vl >> 6;
        const int py = tyy * 2 + (pwv >> 1), px = txx * 2 + (pwv & 1);
        if (py < nY && px < nX) {
            const long orow = ((((long)b * nT + pt) * nY + py) * nX + px) * 64 + (vl & 63);
            if (a.bias) v += *reinterpret_cast<const f32x4_t*>(a.bias + c);
            if (a.mask) {
                const f32x4_t m = *reinterpret_cast<const f32x4_t*>(a.mask + orow * a.mask_ld + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.0f ? v[e] : 0.0f;
            } else if (a.mplanes) {
                const f16* q = reinterpret_cast<const f16*>(a.mplanes) + orow * 320 + (c >> 5) * 64 + (c & 31);
                const f16x4_h3 h = *reinterpret_cast<const f16x4_h3*>(q), l = *reinterpret_cast<const f16x4_h3*>(q + 32);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (h[e] != (f16)0.0f || l[e] != (f16)0.0f) ? v[e] : 0.0f;
            }
            if (a.res) v += a.res_scale * *reinterpret_cast<const f32x4_t*>(a.res + orow * a.res_ld + c);
            if (a.relu_out) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
            }
            if (a.out) {
                float* o = a.out + orow * a.cout_ld + c;
                if (a.accumulate) v += *reinterpret_cast<const f32x4_t*>(o);
                *reinterpret_cast<f32x4_t*>(o) = v;
            }
            if (a.oplanes) put_planes4(a.oplanes, orow, c, v, f16x3_scale(*a.opmax));
            vmax = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
        } else {
            v = (f32x4_t)0.0f;                              // rows off the grid
        }
        // column sums (a.cpart): the final value replaces this item's first partial
        // (read above by this thread only); tail_colsum_kernel sums the tile's rows
        if (a.cpart) *reinterpret_cast<f32x4_t*>(a.part + ((long)(t * 5) * 256 + vl) * 160 + c) = v;
    }
    if (a.omax) block_max_to(a.omax, vmax, red);
}

// column sums of the split tiles' final values (left in each tile's first partial
// slot by conv_f16x3_tail_reduce_kernel) -> a.cpart rows tail_base + t, fixed order
__global__ void __launch_bounds__(160) tail_colsum_kernel(ConvH3Args a, int nparts) {
    const int t = blockIdx.x, c = threadIdx.x;
    const float* p = a.part + (long)(t * nparts) * 256 * 160 + c;
    float cs = 0.0f;
    for (int r = 0; r < 256; ++r) cs += p[(long)r * 160];
    a.cpart[(long)(a.tail_base + t) * 160 + c] = cs;
}

// tail_ws: conv_tail_bytes(tiles) bytes for the tail split's partial tiles
static int conv_f16x3_launch(const ConvH3Args& v0, float* tail_ws, hipStream_t st) {
    ConvH3Args v = v0;
    const int nT = v.D / 4, nY = v.H / 4, nX = v.W / 4;
    unsigned nblk = (unsigned)((long)v.B * nT * ((nY + 1) / 2) * ((nX + 1) / 2));
    // the last partial round of 256-CU waves (3360 tiles = 13 x 256 + 32 at BASELINE
    // size: 32 busy CUs for a whole tile time) runs as 5 x ntail single-chunk
    // workgroups plus a fixed-order reduce
    const char* te = dlcs_test_hook("DLCS_H3_TAIL");                 // read per launch (tests toggle it)
    const bool tail_split = !(te && te[0] == '0');
    const unsigned ntail = tail_split ? conv_tail_tiles(nblk) : 0u, nmain = nblk - ntail;
    const bool split = ntail > 0;
    if (split) nblk = nmain;
    int epi;
    if (!v.res && !v.mask && !v.mplanes && !v.accumulate) epi = 0;
    else if (v.res && !v.mask && !v.mplanes && !v.accumulate) epi = kEpiRes;
    else if (!v.res && (v.mask || v.mplanes) && !v.accumulate) epi = kEpiMask;
    else epi = kEpiGeneric;
    if ((v.oplanes || v.cpart || v.mplanes) && epi != kEpiRes && epi != kEpiMask)
        return DLCS_ERR_UNSUPPORTED_SIZE;                                                   // fused forms only
    // DLCS_H3_FOLD (DIAG build; the modes above the kernel): r (default) random row
    // signs on the masked launches (the input gradients), R on every launch; m fold on
    // the masked launches, 1 fold on every launch and the weight gradient; a
    // sign-alternating running sum on the masked launches; 0 plain everywhere.  The
    // product library has the default only (plain forward, random-sign input gradient).
    static const int fold_mode = [] {
        const char* e = dlcs_knob("DLCS_H3_FOLD");
        return !e ? 4 : e[0] == '0' ? 0 : e[0] == 'm' ? 2 : e[0] == 'a' ? 3 : e[0] == 'r' ? 4 : e[0] == 'R' ? 5 : 1;
    }();
    // kernel FOLD: 1 folded tiles, 2 sign-alternating running sum, 3 sign-alternating rows, 0 plain
    const bool masked = v.mask || v.mplanes;             // an input gradient
    const int pf = fold_mode == 1 || (fold_mode == 2 && masked) ? 1 : (fold_mode == 3 && masked) ? 2
                 : (fold_mode == 5 || (fold_mode == 4 && masked)) ? 3 : 0;
    auto launch = [&](auto F) {
        constexpr int f = decltype(F)::value;
        const dim3 g(nblk);
        if (epi == 0) hipLaunchKernelGGL((conv3d_k3_f16x3_kernel<0, f>), g, dim3(512), 0, st, v);
        else if (epi == kEpiRes) hipLaunchKernelGGL((conv3d_k3_f16x3_kernel<kEpiRes, f>), g, dim3(512), 0, st, v);
        else if (epi == kEpiMask) hipLaunchKernelGGL((conv3d_k3_f16x3_kernel<kEpiMask, f>), g, dim3(512), 0, st, v);
        else hipLaunchKernelGGL((conv3d_k3_f16x3_kernel<kEpiGeneric, f>), g, dim3(512), 0, st, v);
    };
#ifdef DLCS_DIAG_BUILD
    if (pf == 1) launch(std::integral_constant<int, 1>{});
    else if (pf == 2) launch(std::integral_constant<int, 2>{});
    else
#endif
    if (pf == 3) launch(std::integral_constant<int, 3>{});
    else launch(std::integral_constant<int, 0>{});
    if (split) {
        ConvH3Args t = v;
        t.part = tail_ws;
        t.tail_base = (int)nmain;
#ifdef DLCS_DIAG_BUILD
        if (pf == 1) hipLaunchKernelGGL((conv3d_k3_f16x3_kernel<0, 1, true>), dim3(ntail * 5), dim3(512), 0, st, t);
        else if (pf == 2) hipLaunchKernelGGL((conv3d_k3_f16x3_kernel<0, 2, true>), dim3(ntail * 5), dim3(512), 0, st, t);
        else
#endif
        if (pf == 3) hipLaunchKernelGGL((conv3d_k3_f16x3_kernel<0, 3, true>), dim3(ntail * 5), dim3(512), 0, st, t);
        else hipLaunchKernelGGL((conv3d_k3_f16x3_kernel<0, 0, true>), dim3(ntail * 5), dim3(512), 0, st, t);
        hipLaunchKernelGGL(conv_f16x3_tail_reduce_kernel, dim3((unsigned)cdiv((long)ntail * 256 * 40, 256)), dim3(256),
                           0, st, t, (int)ntail);
        if (v.cpart) hipLaunchKernelGGL(tail_colsum_kernel, dim3(ntail), dim3(160), 0, st, t, 5);
    }
    return dlcs_launch_status();
}

// ---------------------------------------------------------------- wgrad on fp16 matrix cores (2-plane split)
// dW[tap][co][ci] = sum_v g[v][co] x[v + off(tap)][ci] with g and x as f16
// plane pairs (dlcs_split2_f16) and the three plane products gh xh + gh xl +
// gl xh; K = voxels, one v_mfma_f32_16x16x32_f16 covers 32 voxels of ONE plane
// pair (lane group gq supplies voxels 8 gq .. 8 gq + 7).  Workgroup = tap row
// (kd, kh) x voxel range, 12 waves = 3 kw taps x 2 co halves x 2 ci halves (80
// x 80 of dW[tap] each, 5 x 5 tiles); unit = half patch (32 voxels): per plane
// its g rows [32][160] and the tap row's x halo [2 t][4 y][6 x][160], 51.2 KB
// for the two planes, DMA'd global -> LDS two units ahead into a 3-buffer ring;
// 16-channel tiles XOR-swizzled by the parity of the 8-voxel group.  Per unit
// and wave: 25 transposed fragment reads (gh, gl, xh twice, xl) for 75 MFMAs.
//
// Issue budget (round 5).  With three waves per SIMD the matrix pipe leaves
// each wave ~8 of every 16 cycles of an MFMA for everything else; the round-4
// kernel spent ~280 VALU instructions per unit and wave on DMA address math
// (divisions by 20 and 6 of the piece index, neighbour-patch arithmetic, bounds
// tests), so the SIMD was VALU-issue-bound (SQ: 1.94x the forward's issued
// instructions at equal MFMA work, MFMA busy 0.54).  Now every lane's source
// offset of each of its DMA pieces is computed ONCE, for both half-patch
// positions (th = 0 / 1: the loop body is unrolled over the two halves of a
// patch, so th is a compile-time constant), relative to a per-unit scalar base;
// per unit and piece: one shift / mask for the offset, one AND + compare
// against the unit's scalar "missing neighbour" mask (halo rows outside the
// volume), one select of the zero row (a 640-B zero row after the plane
// buffer's trailer, dlcs_split2_f16_bytes).  Output: each workgroup stores its
// raw 3 x 160 x 160 partial (no float atomics) into a per-range slab; a
// fixed-order reduce adds the ranges into dW -- run-to-run deterministic.
constexpr int kWhRows = 32 + 48;                     // 32 g rows + the 48-row x halo of a patch
constexpr int kWhPlane = kWhRows * 160;              // f16 per plane image (25.6 KB)
constexpr int kWhBuf = 2 * kWhPlane;                 // 51.2 KB

struct WgradH3Args {
    const f16* gp; const f16* xp;                    // plane pairs [rows][320]
    const unsigned* gmax; const unsigned* xmax;
    float* dw;
    float* part;                                     // [nrange][27][160][160] raw partials
    int B, D, H, W;
};

DLCS_DEV f16x8_t tr_read16h(const f16* p0, const f16* p1) {
    return __builtin_bit_cast(f16x8_t, tr_read16(reinterpret_cast<const bf16*>(p0), reinterpret_cast<const bf16*>(p1)));
}

// byte offset of the zero row of a split2 buffer of `rows` rows (dlcs_split2_f16_bytes)
DLCS_DEV long h3_zero_row_byte(long rows) { return rows * 640 + 256; }

__global__ void __launch_bounds__(768) conv3d_wgrad_f16x3_kernel(WgradH3Args a, int nrange, int ppr) {
    __shared__ __attribute__((aligned(16))) f16 smem_wh[3 * kWhBuf];     // 153.6 KB: a 3-unit ring
    const int b = blockIdx.x;
    int range, grp;
    {                                                // the 9 tap rows of a range on one XCD (b % 8)
        const int xcd = b & 7, slot = b >> 3;
        const int q = nrange >> 3;
        if ((nrange & 7) == 0) { range = (slot / 9) * 8 + xcd; grp = slot % 9; }
        else if ((nrange & 7) == 4) {                // 8 q + 4: the last 4 ranges split 5 + 4 tap rows over XCD pairs
            if (slot < 9 * q) { range = (slot / 9) * 8 + xcd; grp = slot % 9; }
            else { range = 8 * q + (xcd & 3); grp = (slot - 9 * q) + (xcd < 4 ? 0 : 5); }
        } else { range = b / 9; grp = b % 9; }
    }
    if (range >= nrange || grp >= 9) return;
    const int kd = grp / 3 - 1, kh = grp % 3 - 1;
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int nYX = nY * nX;
    const int npatch = a.B * nT * nYX;
    const int p0 = range * ppr, p1 = min(npatch, p0 + ppr);
    if (p0 >= p1) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kwi = wave >> 2, coh = (wave >> 1) & 1, cih = wave & 1;
    // rows below the current patch a halo row may reach (t, y, x neighbours): the
    // per-unit scalar base sits that far back, so every lane offset is >= 0
    const int bias_rows = (nYX + nX + 1) * 64;
    const long rows = (long)npatch * 64;

    // per-lane DMA pieces: wave-instruction wi = 12 k + wave (< 50); plane wi / 25,
    // rows 0..31 (g, wl < 10) or 32..79 (halo).  One register per piece, for the first
    // half of a patch (th = 0): pk[k] = (byte offset / 16) << 7 | t1hi << 6 | req, req
    // = the 6-bit neighbour requirement (t-, t+, y-, y+, x-, x+) of the row.  The
    // second half (th = 1, two time slices later) is derived: g rows +32 rows; a halo
    // row +32 rows within the patch, or -- when tt = -1 or 2 (req bit 0 or t1hi) --
    // the next t patch (+nYX patches - 32 rows), whose t requirement is t1hi alone.
    unsigned pk[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int wi = k * 12 + wave;
        const int pl = wi >= 25 ? 1 : 0, wl = wi - pl * 25;
        const int c = wl * 64 + lane;
        const int row = c / 20, kp = c - row * 20;
        int vrow, swz;
        unsigned req = 0;
        if (wl < 10) {
            vrow = row;
            swz = (row >> 3) & 1;
        } else {
            const int hr = row - 32, ty = hr / 6, xh = hr - ty * 6;
            const int tl = ty >> 2, y = ty & 3;
            swz = (y >> 1) & 1;
            const int tt = tl + kd, yy = y + kh, xx = xh - 1;
            req = (tt < 0 ? 1u : 0u) | (tt >= 4 ? 2u : 0u) | (yy < 0 ? 4u : 0u) | (yy >= 4 ? 8u : 0u) |
                  (xx < 0 ? 16u : 0u) | (xx >= 4 ? 32u : 0u) | (tt + 2 >= 4 ? 64u : 0u);
            vrow = (((tt >> 2) * nYX + (yy >> 2) * nX + (xx >> 2)) << 6) + ((tt & 3) << 4) + ((yy & 3) << 2) +
                   (xx & 3);
        }
        const int kl = kp ^ (swz << 1);
        const unsigned off16 = (unsigned)((vrow + bias_rows) * 40 + (kl >> 2) * 8 + pl * 4 + (kl & 3));
        pk[k] = wi < 50 ? (off16 << 7) | req : 0u;
    }
    const unsigned dst0 = __builtin_amdgcn_readfirstlane(lds_offset(smem_wh));
    // the unit's patch: flat index ip and (t, y, x) coordinates, advanced with carries
    int ip = p0, ipt, ipy, ipx;
    {
        const int r = ip % (nT * nYX);
        ipt = r / nYX;
        ipy = (r / nX) % nY;
        ipx = r % nX;
    }
    auto missing = [&]() {                           // neighbours of patch ip outside the volume (scalar)
        return (ipt == 0 ? 1u : 0u) | (ipt == nT - 1 ? 2u : 0u) | (ipy == 0 ? 4u : 0u) | (ipy == nY - 1 ? 8u : 0u) |
               (ipx == 0 ? 16u : 0u) | (ipx == nX - 1 ? 32u : 0u);
    };
    auto next_patch = [&]() {
        ++ip;
        if (++ipx == nX) {
            ipx = 0;
            if (++ipy == nY) {
                ipy = 0;
                if (++ipt == nT) ipt = 0;
            }
        }
    };
    // DMA piece k of half th of patch `ip` into ring buffer buf
    const unsigned d32 = 32 * 640, dcross = (unsigned)(nYX * 64 - 32) * 640;
    auto issue_piece = [&](int k, int th, int buf, unsigned miss, const char* gbase, const char* xbase,
                           unsigned xzero) {
        const int wi = k * 12 + wave;
        if (wi >= 50) return;
        const int pl = wi >= 25 ? 1 : 0, wl = wi - pl * 25;
        const unsigned v = pk[k];
        unsigned off = (v >> 3) & ~15u;
        if (wl < 10) {
            if (th) off += d32;
        } else {
            unsigned req = v & 63u;
            if (th) {
                const bool cross = (v & 65u) != 0u;
                off += cross ? dcross : d32;
                req = (v & 60u) | ((v >> 5) & 2u);
            }
            off = (req & miss) ? xzero : off;
        }
        glds16_s(wl < 10 ? gbase : xbase, off, dst0 + (unsigned)(buf * kWhBuf * 2 + pl * kWhPlane * 2 + wl * 1024));
    };
    // per-patch scalars: the bases sit bias_rows below the patch's first row
    auto bases = [&](const char*& gb, const char*& xb, unsigned& xz) {
        const long r0 = (long)ip * 64 - bias_rows;
        gb = reinterpret_cast<const char*>(a.gp) + r0 * 640;
        xb = reinterpret_cast<const char*>(a.xp) + r0 * 640;
        xz = (unsigned)(h3_zero_row_byte(rows) - r0 * 640);
    };

    f32x4_t acc[5][5];
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) acc[i][j] = (f32x4_t)0.0f;

    const int gq = lane >> 4, q = (lane >> 2) & 3, p4 = (lane & 3) * 4, swb = gq & 1;
    auto acol = [&](int i) { return (((coh * 5 + i) ^ swb) << 4) + p4; };
    auto bcol = [&](int j) { return (((cih * 5 + j) ^ swb) << 4) + p4; };
    // voxels 8 gq + {q, q + 4} of the unit: t = gq >> 1, y = 2 (gq & 1) + {0, 1}, x = q
    const int grow = (8 * gq + q) * 160;
    const int xrow = (32 + ((gq >> 1) * 4 + 2 * swb) * 6 + q + kwi) * 160;

    // prologue: both halves of the first patch (units u0, u0 + 1) into buffers 0, 1
    {
        const char *gb, *xb;
        unsigned xz;
        bases(gb, xb, xz);
        const unsigned miss = missing();
#pragma unroll
        for (int k = 0; k < 5; ++k) issue_piece(k, 0, 0, miss, gb, xb, xz);
#pragma unroll
        for (int k = 0; k < 5; ++k) issue_piece(k, 1, 1, miss, gb, xb, xz);
    }
    next_patch();                                    // ip = the patch of units u0 + 2, u0 + 3
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    // one unit: multiply buffer cur, DMA half th of patch ip (unit u + 2) into the buffer
    // the ring frees next, then wait for unit u + 1 and publish it
    auto unit = [&](int TH, bool ahead) {
        // opaque per unit: keeps the compiler from hoisting the decoded piece values
        // (2-3 registers per piece) out of the loop and spilling them
#pragma unroll
        for (int k = 0; k < 5; ++k) asm volatile("" : "+v"(pk[k]));
        const int nbuf = cur == 0 ? 2 : cur - 1;
        const char *gb, *xb;
        unsigned xz;
        bases(gb, xb, xz);
        const unsigned miss = missing();
        const f16* S = smem_wh + cur * kWhBuf;
        const f16* Gh = S + grow;
        const f16* Gl = S + kWhPlane + grow;
        const f16* Xh = S + xrow;
        const f16* Xl = S + kWhPlane + xrow;
        f16x8_t gh[5], gl[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) gh[i] = tr_read16h(Gh + acol(i), Gh + 4 * 160 + acol(i));
        f16x8_t xh = tr_read16h(Xh + bcol(0), Xh + 6 * 160 + bcol(0));
        f16x8_t xl = tr_read16h(Xl + bcol(0), Xl + 6 * 160 + bcol(0));
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            if (j == 0) {
#pragma unroll
                for (int i = 0; i < 5; ++i) gl[i] = tr_read16h(Gl + acol(i), Gl + 4 * 160 + acol(i));
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) mfma16h(acc[i][j], gh[i], xh);
#pragma unroll
            for (int i = 0; i < 5; ++i) mfma16h(acc[i][j], gh[i], xl);
#pragma unroll
            for (int i = 0; i < 5; ++i) mfma16h(acc[i][j], gl[i], xh);
            if (ahead) issue_piece(j, TH, nbuf, miss, gb, xb, xz);
            if (j + 1 < 5) {
                xh = tr_read16h(Xh + bcol(j + 1), Xh + 6 * 160 + bcol(j + 1));
                xl = tr_read16h(Xl + bcol(j + 1), Xl + 6 * 160 + bcol(j + 1));
            }
        }
        if (!ahead) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (wave < 2) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        __syncthreads();
        cur = cur == 2 ? 0 : cur + 1;
    };
    for (int u = 2 * p0; u < 2 * p1; ++u) {
        const int th = u & 1;
        unit(th, (u >> 1) + 1 < p1);
        if (th) next_patch();
    }
    // raw partial of this (range, tap row): part[range][tap][co][ci], 16-B row stores
    // after a transpose through LDS (each wave's 80 x 80 block; the ring is free now)
    const int tap = (kd + 1) * 9 + (kh + 1) * 3 + kwi;
    float* pp = a.part + ((long)range * 27 + tap) * 160 * 160;
    float* st = reinterpret_cast<float*>(smem_wh) + wave * (16 * 84);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) st[(gq * 4 + r) * 84 + j * 16 + (lane & 15)] = acc[i][j][r];
        // 16 rows x 80 columns: lane -> (row lane / 4 .. +4 rows apart, 16-B column chunk)
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const int e = s * 64 + lane, r = e / 20, c4 = (e % 20) * 4;
            const f32x4_t v = *reinterpret_cast<const f32x4_t*>(st + r * 84 + c4);
            *reinterpret_cast<f32x4_t*>(pp + (coh * 80 + 16 * i + r) * 160 + cih * 80 + c4) = v;
        }
    }
}

// dW[tap][co][ci] += inv * sum over ranges (fixed order) of the raw partials;
// inv = 1 / (s_g s_x) (exact, a power of two)
__global__ void __launch_bounds__(256) wgrad_f16x3_reduce_kernel(WgradH3Args a, int nrange) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;        // float4 index
    if (i >= 27L * 160 * 40) return;
    const float inv = 1.0f / (f16x3_scale(*a.gmax) * f16x3_scale(*a.xmax));
    const f32x4_t* src = reinterpret_cast<const f32x4_t*>(a.part);
    f32x4_t s = src[i];
    for (int r = 1; r < nrange; ++r) s += src[(long)r * 27 * 160 * 40 + i];
    f32x4_t* d = reinterpret_cast<f32x4_t*>(a.dw) + i;
    *d = *d + s * inv;
}

// voxel ranges of the weight gradient, one partial slab (2.76 MB) each: 28, or
// DLCS_WGH3_RANGES (DIAG build) up to 32; bound = the most any setting gives
constexpr int kWgH3MaxRanges = 32;

static PatchRanges wgh3_ranges(long npatch, bool bound) {
    static const int env_nr = [] { const char* e = dlcs_knob("DLCS_WGH3_RANGES"); return e ? atoi(e) : 0; }();
    return patch_ranges(npatch, bound ? kWgH3MaxRanges : env_nr > 0 ? std::min(env_nr, kWgH3MaxRanges) : 28);
}

// a.part: wgh3_ranges(npatch, true).nr slabs
static int wgrad_f16x3_launch(const WgradH3Args& a, hipStream_t st) {
    const long npatch = (long)a.B * (a.D / 4) * (a.H / 4) * (a.W / 4);
    // 32-bit lane offsets (16-B units << 7 in the kernel, relative to a base bias_rows below
    // the patch): 2 bias_rows + 2 patches within 2^25 x 16 B; the zero row's byte offset
    // from a unit base within 2^32
    const long bias_rows = ((long)(a.H / 4) * (a.W / 4) + a.W / 4 + 1) * 64;
    if ((2 * bias_rows + 128) * 40 >= (1L << 25) || (npatch * 64 + bias_rows) * 640 + 1024 >= (1L << 32))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    const PatchRanges r = wgh3_ranges(npatch, false);
    const int nr = r.nr;
    const long pp = r.pp;
    hipLaunchKernelGGL(conv3d_wgrad_f16x3_kernel, dim3((unsigned)(9 * nr)), dim3(768), 0, st, a, nr, (int)pp);
    hipLaunchKernelGGL(wgrad_f16x3_reduce_kernel, dim3((unsigned)cdiv(27L * 160 * 40, 256)), dim3(256), 0, st, a, nr);
    return dlcs_launch_status();
}

// ---------------------------------------------------------------- K = 160 GEMM on fp16 matrix cores (2-plane split)
// C[m, n] (+)= alpha act(sum_k A[m, k] B[n, k] + bias[n]) + rs res[m, n] + rs2 res2[m, n]
// for K = 160 with A and B as dlcs_split2_f16 plane pairs ([rows][320] +
// max trailer): the k4s4 patch unembed forward and the patch embed's input
// gradient (vst:455, :503 -- N = 64 x 160 = 10240 output columns per token,
// 44 GFLOP each, 550 MB written).  Tile 64 x 160 (see v2 below), 3 plane
// products per 16x16x32 f16 MFMA group, the conv kernels' conflict-free
// 128-B-row swizzle for both operand images; epilogue staged through LDS so
// every C / residual access is 16 B along a row.
struct GemmH3Args {
    const f16* ap; const f16* bp; const unsigned* amax; const unsigned* bmax;
    float* c; long ldc;
    const float* bias; int act; float alpha;
    const float* res; long ldr; float res_scale;
    const float* res2; long ldr2; float res2_scale;
    int accumulate;
    int M, N;
    unsigned* omax;                                 // optional max |C| (float bits) for the next split
    // token Linear epilogues (dlcs_linear_k160_f16x3): act 1 = GELU (pre-activation
    // to aux_out), act 2 = times GELU'(aux); output / residual row row_map[m] (< 0: skip)
    const float* aux; float* aux_out; long ldaux;
    const int* row_map;
    int xcd_nt;                                     // > 0: 1-D grid, xcd_nt consecutive N tiles per XCD
    f16* oplanes; const unsigned* opmax;            // optional split2 image of C as [M N / 160][160] (ldc == N)
    float* cpart;                                   // optional column-sum partials [M / 64 tiles][N / 160][160] (c % 160)
    const f16* rp; const f16* rp2;                  // residuals as split2 images of the [M N / 160][160] view (instead of res / res2)
    const unsigned* rpmax; const unsigned* rp2max;
};
// v3: 64-row tiles; the A tile's whole K (5 x 8 KB) DMA'd up front, B streamed
// per 32-channel chunk through a 2-slot ring (2 x 20 KB): 80 KB, so two
// workgroups share a CU and one's DMA waits / epilogue overlap the other's
// MFMAs (v1, 128-row tiles with a one-chunk lookahead on both operands: 546 us
// for the 44-GFLOP unembed; v2, whole K of both up front in 140 KB = one
// workgroup per CU: no overlap).  8 waves of 16 x 80.
constexpr int kG3A = 64 * 64, kG3B = 160 * 64;        // f16 per operand chunk (8 KB / 20 KB)

__global__ void __launch_bounds__(512, 2) gemm_k160_f16x3_kernel(GemmH3Args g) {
    __shared__ __attribute__((aligned(16))) f16 smem_g3[5 * kG3A + 2 * kG3B];   // 80 KB
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave & 3, wn = wave >> 2;
    int mt = blockIdx.x, nt = blockIdx.y;
    if (g.xcd_nt) {
        // XCD x owns N tiles [x xcd_nt, (x + 1) xcd_nt) and walks the M tiles in
        // order: its B planes (xcd_nt x 100 KB) stay in its L2 and each A tile is
        // read by xcd_nt neighbouring workgroups (the one-tile-per-block order
        // streamed all 6.5 MB of B through every XCD's L2 from the MALL)
        const int k = blockIdx.x >> 3;
        nt = (blockIdx.x & 7) * g.xcd_nt + k % g.xcd_nt;
        mt = k / g.xcd_nt;
    }
    const int m0 = mt * 64, n0 = nt * 160;
    const unsigned sbase = lds_offset(smem_g3);
    // A: instruction wi (0..39) = chunk wi / 8, rows 8 (wi % 8) ..
    auto issue_a = [&]() {
        for (int wi = wave; wi < 40; wi += 8) {
            const int cc = wi >> 3, rb = wi & 7;
            const int r = rb * 8 + (lane >> 3), pc = lane & 7;
            const int lc = pc ^ ((r >> 1) & 7);
            const f16* src = g.ap + (long)min(m0 + r, g.M - 1) * 320 + cc * 64 + lc * 8;
            glds16(src, sbase + (unsigned)(cc * kG3A * 2 + rb * 1024));
        }
    };
    // B chunk cc into slot: 20 instructions, rows 8 rb ..
    auto issue_b = [&](int cc, int slot) {
        for (int rb = wave; rb < 20; rb += 8) {
            const int r = rb * 8 + (lane >> 3), pc = lane & 7;
            const int lc = pc ^ ((r >> 1) & 7);
            const f16* src = g.bp + (long)min(n0 + r, g.N - 1) * 320 + cc * 64 + lc * 8;
            glds16(src, sbase + (unsigned)((5 * kG3A + slot * kG3B) * 2 + rb * 1024));
        }
    };
    issue_a();
    issue_b(0, 0);
    f32x4_t acc[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) acc[j] = (f32x4_t)0.0f;
    const int vq = lane & 15, cq = lane >> 4, sw = (vq >> 1) & 7;
    const int oh = (cq ^ sw) << 3, ol = ((4 + cq) ^ sw) << 3;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int cc = 0; cc < 5; ++cc) {
        if (cc + 1 < 5) issue_b(cc + 1, (cc + 1) & 1);
        const f16* As = smem_g3 + cc * kG3A + (wm * 16 + vq) * 64;
        const f16* Bs = smem_g3 + 5 * kG3A + (cc & 1) * kG3B + (wn * 80 + vq) * 64;
        const f16x8_t ah = *reinterpret_cast<const f16x8_t*>(As + oh);
        const f16x8_t al = *reinterpret_cast<const f16x8_t*>(As + ol);
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const f16x8_t bh = *reinterpret_cast<const f16x8_t*>(Bs + j * 16 * 64 + oh);
            const f16x8_t bl = *reinterpret_cast<const f16x8_t*>(Bs + j * 16 * 64 + ol);
            mfma16h(acc[j], ah, bh);
            mfma16h(acc[j], ah, bl);
            mfma16h(acc[j], al, bh);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    const float inv = 1.0f / (f16x3_scale(*g.amax) * f16x3_scale(*g.bmax));
    __syncthreads();                                     // operand images dead: reuse LDS for the epilogue
    float* Es = reinterpret_cast<float*>(smem_g3);       // [64][164]
    constexpr int EL = 164;
    const float ps = g.oplanes ? f16x3_scale(*g.opmax) : 1.0f;
    const float rinv = g.rp ? 1.0f / f16x3_scale(*g.rpmax) : 1.0f;        // exact: powers of two
    const float rinv2 = g.rp2 ? 1.0f / f16x3_scale(*g.rp2max) : 1.0f;
    float vmax = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            Es[(wm * 16 + 4 * cq + r) * EL + wn * 80 + j * 16 + vq] = acc[j][r] * inv;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int c = threadIdx.x + k * 512;             // 64 rows x 40 16-B chunks
        const int ml = c / 40, ch = (c % 40) * 4;
        const long m = m0 + ml, n = n0 + ch;
        if (m >= g.M || n >= g.N) {
            if (g.cpart) *reinterpret_cast<f32x4_t*>(Es + ml * EL + ch) = (f32x4_t)0.0f;
            continue;
        }
        long orow = m;
        if (g.row_map) {
            orow = g.row_map[m];
            if (orow < 0) continue;
        }
        f32x4_t v = *reinterpret_cast<const f32x4_t*>(Es + ml * EL + ch);
        if (g.bias) v += *reinterpret_cast<const f32x4_t*>(g.bias + n);
        if (g.act == 3) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
        } else if (g.act == 1) {
            if (g.aux_out) *reinterpret_cast<f32x4_t*>(g.aux_out + m * g.ldaux + n) = v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = gelu_erf(v[e]);
        } else if (g.act == 2) {
            const f32x4_t av = *reinterpret_cast<const f32x4_t*>(g.aux + m * g.ldaux + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= gelu_erf_grad(av[e]);
        }
        v *= g.alpha;
        if (g.res) v += g.res_scale * *reinterpret_cast<const f32x4_t*>(g.res + orow * g.ldr + n);
        if (g.res2) v += g.res2_scale * *reinterpret_cast<const f32x4_t*>(g.res2 + orow * g.ldr2 + n);
        if (g.rp) v += g.res_scale * get_planes4(g.rp, orow * (g.N / 160) + nt, ch, rinv);
        if (g.rp2) v += g.res2_scale * get_planes4(g.rp2, orow * (g.N / 160) + nt, ch, rinv2);
        if (g.c) {                                       // (planes-only output: no fp32 C)
            float* cp = g.c + orow * g.ldc + n;
            if (g.accumulate) v += *reinterpret_cast<const f32x4_t*>(cp);
            *reinterpret_cast<f32x4_t*>(cp) = v;
        }
        if (g.oplanes) put_planes4(g.oplanes, orow * (g.N / 160) + nt, ch, v, ps);
        if (g.cpart) *reinterpret_cast<f32x4_t*>(Es + ml * EL + ch) = v;   // this item's own slot
        vmax = fmaxf(vmax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
    if (g.cpart) {                                       // the tile's column sums, fixed order
        __syncthreads();
        if (threadIdx.x < 160) {
            float cs = 0.0f;
            for (int r = 0; r < 64; ++r) cs += Es[r * EL + threadIdx.x];
            g.cpart[((long)mt * (g.N / 160) + nt) * 160 + threadIdx.x] = cs;
        }
    }
    if (g.omax) block_max_to(g.omax, vmax, Es + 64 * EL);    // past the staged tile: LDS stays at 80 KB
}

// v4 of round 5 (B planes resident in registers, A streamed through a 2-slot
// ring, one workgroup of 4 waves per CU) moved 3.5x less global -> LDS data but ran
// slower (unembed 273 vs 258 us, embed input gradient 821 vs 433 us): with four
// waves a CU no longer overlaps one tile's epilogue traffic with another's MFMAs.
static int gemm_k160_launch(const GemmH3Args& g0, hipStream_t st) {
    GemmH3Args g = g0;
    const int ntiles = g.N / 160;
    if (g.xcd_nt >= 0 && ntiles % 8 == 0) {
        g.xcd_nt = ntiles / 8;
        hipLaunchKernelGGL(gemm_k160_f16x3_kernel, dim3(cdiv(g.M, 64) * (unsigned)ntiles), dim3(512), 0, st, g);
    } else {
        g.xcd_nt = 0;
        hipLaunchKernelGGL(gemm_k160_f16x3_kernel, dim3(cdiv(g.M, 64), (unsigned)ntiles), dim3(512), 0, st, g);
    }
    return dlcs_launch_status();
}
