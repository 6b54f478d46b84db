// fp32 (parity-build) Conv3d 160 -> 160 kernels on the f32-input MFMA
// (v_mfma_f32_16x16x4_f32: exact f32 FMA chains at the f32 peak, 157 TF on
// MI355X -- 1/16 of bf16, so these kernels are far easier to keep fed than the
// bf16 ones; the design goal is the MFMA issue rate with no exposed latency).
// Included by conv3d.hip (args structs and layout: conv3d_common.h; DMA helpers: lds_dma.h).
//
// Operand convention of v_mfma_f32_16x16x4_f32: lane l holds ONE f32 of A
// (A[m = l & 15][k = l >> 4]) and of B (B[k = l >> 4][n = l & 15]); C/D as the
// bf16 16x16 forms (col = lane & 15, row = 4 (lane >> 4) + r).

// ---------------------------------------------------------------- wgrad, 160 -> 160 (fp32)
// dW[tap][co][ci] = sum_v g[v][co] * x[v + off(tap)][ci]:  M = co, N = ci, K = voxels.
// With K = voxels the f32 MFMA operands are channel-contiguous in the natural
// row-major activation layout: lane (m, k) of A reads g[voxel k][channel m], 16
// consecutive channels per 16 lanes -- no transposition anywhere.
//
// One workgroup = tap row (kd, kh) x voxel range; 12 waves = 3 kw taps x 2 co
// halves x 2 ci halves, each an 80 x 80 block of dW[tap] (5 x 5 tiles, 100
// accumulators per lane).  The unit of work is a half patch (32 voxels: 2 t x 4
// y x 4 x): its g rows [32][160] and the tap row's x halo [2 t][4 y][6 x][160],
// shared by the 3 kw taps, are DMA'd global -> LDS (global_load_lds_dwordx4) two
// units ahead into a ring of three 51.2-KB buffers; one barrier per unit (19.2k
// MFMA cycles per SIMD).  ds_read_b32 operands, conflict-free: the 16-B
// chunks of LDS row R sit XOR-swizzled by 4 (R & 1), so the two rows a 32-lane
// half reads (voxels k, k + 1) fall on opposite 16-bank halves.
constexpr int kWfC = 160;
constexpr int kWfRows = 32 + 48;                      // g rows + halo rows per unit
constexpr int kWfBuf = kWfRows * kWfC;                // floats per LDS buffer (51200 B)

__device__ float4 g_wf_zero_row[kWfC / 4];            // zero source row (halo voxels off the grid)

DLCS_DEV void mfma4f(f32x4_t& acc, float a, float b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
}

__global__ void __launch_bounds__(768) conv3d_wgrad_f32_kernel(WgradArgs a, int nrange, long ppr, int xcd_map) {
    __shared__ __attribute__((aligned(16))) float smem[3 * kWfBuf];     // 153.6 KB
    const int b = blockIdx.x;
    int range, grp;
    if (xcd_map) {                                   // the 9 tap rows of a range on one XCD (b % 8)
        const int xcd = b & 7, slot = b >> 3;
        range = (slot / 9) * 8 + xcd;
        grp = slot % 9;
    } else {
        range = b / 9;
        grp = b % 9;
    }
    if (range >= nrange) return;
    const int kd = grp / 3 - 1, kh = grp % 3 - 1;
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const long npatch = (long)a.B * nT * nY * nX;
    const long p0 = (long)range * ppr, p1 = min(npatch, p0 + ppr);
    if (p0 >= p1) return;
    const float* in = reinterpret_cast<const float*>(a.in);
    const float* g = reinterpret_cast<const float*>(a.g);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kwi = wave >> 2, coh = (wave >> 1) & 1, cih = wave & 1;
    const float* zrow = reinterpret_cast<const float*>(g_wf_zero_row);

    // DMA of unit u (patch u >> 1, t half u & 1): chunk c = row c / 40, physical
    // slot c % 40 holding logical chunk slot ^ (4 (row & 1)); rows 0..31 g,
    // 32..79 halo (row 32 + (tl * 4 + y) * 6 + xh), off-grid halo rows read zeros.
    auto issue = [&](long u, int buf) {
        const long patch = u >> 1;
        const int th = (int)(u & 1);
        const int px = (int)(patch % nX);
        long r = patch / nX;
        const int py = (int)(r % nY); r /= nY;
        const int pt = (int)(r % nT);
        const int bb = (int)(r / nT);
        const unsigned dst = __builtin_amdgcn_readfirstlane(lds_offset(smem) + buf * kWfBuf * 4);
        int ln = lane;
        asm volatile("" : "+v"(ln));
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int wi = k * 12 + wave;
            if (wi >= 50) break;
            const int c = wi * 64 + ln;
            const int row = c / 40, kp = c - row * 40;
            const int kl = kp ^ ((row & 1) << 2);
            const float* src;
            if (wi < 20) {                                  // g rows: 32 x 40 chunks = 20 instructions
                src = g + (patch * 64 + th * 32 + row) * (long)a.g_ld + (kl << 2);
            } else {
                const int hr = row - 32, ty = hr / 6, xh = hr - ty * 6;
                const int tl = ty >> 2, y = ty & 3;
                const int T = pt * 4 + th * 2 + tl + kd, Y = py * 4 + y + kh, X = px * 4 + xh - 1;
                const bool ok = (unsigned)T < (unsigned)a.D && (unsigned)Y < (unsigned)a.H && (unsigned)X < (unsigned)a.W;
                const long vrow = ((((long)(bb * nT + (T >> 2)) * nY + (Y >> 2)) * nX + (X >> 2)) << 6) +
                                  ((T & 3) << 4) + ((Y & 3) << 2) + (X & 3);
                src = ok ? in + vrow * a.cin_ld + (kl << 2) : zrow + (kl << 2);
            }
            glds16(src, dst + wi * 1024);
        }
    };

    f32x4_t acc[5][5];
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) acc[i][j] = (f32x4_t)0.0f;

    // lane -> voxel q = lane >> 4 of a 4-voxel k-step, channel m = lane & 15.
    // k-step s (0..7) of a unit: voxels 4s + q = (tl = s >> 2, y = s & 3, x = q):
    // g LDS row 4s + q (parity q & 1), halo LDS row 32 + (4 tl + y) * 6 + q + kwi
    // (parity (q + kwi) & 1).  The physical float of channel 16 t + m in a row
    // of parity p is (16 t + m) ^ 16 p, so every operand address is a per-lane
    // constant plus an immediate (row and buffer offsets): no address math in
    // the loop.
    const int q = lane >> 4, m = lane & 15;
    const int gp = q & 1, hp = (q + kwi) & 1;
    int aoff[5], boff[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) aoff[i] = q * kWfC + (((coh * 5 + i) ^ gp) << 4) + m;
#pragma unroll
    for (int j = 0; j < 5; ++j) boff[j] = (32 + q + kwi) * kWfC + (((cih * 5 + j) ^ hp) << 4) + m;

    const long u0 = 2 * p0, u1 = 2 * p1;
    issue(u0, 0);
    if (u0 + 1 < u1) issue(u0 + 1, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    for (long u = u0; u < u1; ++u) {
        // 3-buffer ring: unit u + 2 goes into the buffer unit u - 1 used, which
        // every wave left at the barrier that ended unit u - 1
        if (u + 2 < u1) issue(u + 2, cur == 0 ? 2 : cur - 1);
        const float* S = smem + cur * kWfBuf;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int gro = 4 * s * kWfC, hro = ((s >> 2) * 4 + (s & 3)) * 6 * kWfC;
            float af[5], bfv[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) af[i] = S[aoff[i] + gro];
#pragma unroll
            for (int j = 0; j < 5; ++j) bfv[j] = S[boff[j] + hro];
#pragma unroll
            for (int j = 0; j < 5; ++j)
#pragma unroll
                for (int i = 0; i < 5; ++i) mfma4f(acc[i][j], af[i], bfv[j]);
        }
        // unit u + 1 must have landed; unit u + 2's DMA (5 instructions on waves
        // 0-1, 4 on the others) may stay in flight
        if (u + 2 < u1) {
            if (wave < 2) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        cur = cur == 2 ? 0 : cur + 1;
    }
    // flush: dW packed [27][160 co][160 ci]; C/D row -> co, col -> ci
    const int tap = (kd + 1) * 9 + (kh + 1) * 3 + kwi;
    float* dw = a.dw + (long)tap * kWfC * kWfC;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = coh * 80 + 16 * i + q * 4 + r, ci = cih * 80 + 16 * j + m;
                atomicAdd(dw + co * kWfC + ci, acc[i][j][r]);
            }
}

static int wgrad_f32_c160_launch(const WgradArgs& a, hipStream_t st) {
    const long npatch = (long)a.B * (a.D / 4) * (a.H / 4) * (a.W / 4);
    static const int env_nr = [] { const char* e = dlcs_knob("DLCS_WGF32_RANGES"); return e ? atoi(e) : 0; }();
    int nr = env_nr > 0 ? env_nr : 28;                // 28 ranges x 9 tap rows = 252 workgroups (one wave of the chip)
    nr = (int)std::min<long>(nr, npatch);
    const long pp = (npatch + nr - 1) / nr;
    nr = (int)((npatch + pp - 1) / pp);
    const int xcd_map = (nr % 8 == 0) ? 1 : 0;
    hipLaunchKernelGGL(conv3d_wgrad_f32_kernel, dim3((unsigned)(9 * nr)), dim3(768), 0, st, a, nr, pp, xcd_map);
    return dlcs_launch_status();
}

// ---------------------------------------------------------------- forward / dgrad, 160 -> 160 (fp32)
// The tile / wave / pipeline structure of the bf16 v5 kernel, re-derived for the
// f32 MFMA: workgroup = 1x2x2 patches (256 voxels) x 160 output channels, 8
// waves = patch pw x channel half nh, 4 x 5 tiles of 16x16 per wave.  K is
// walked per 16-channel chunk (10 chunks) x 9 tap rows of 3 kw taps.  LDS rows
// are 64 B in both dtypes (32 bf16 or 16 f32 channels), so the halo [600][16]
// and weight-slice [3][160][16] images, their XOR swizzles and DMA pieces are
// the v5 ones byte for byte.  A lane's ds_read_b128 returns 4 consecutive
// channels 4 cq .. 4 cq + 3 of its voxel (A) / output channel (B); component e
// feeds the e-th of four v_mfma_f32_16x16x4_f32, in which lane group cq
// contributes k = channel 4 cq + e -- A and B agree, so the 4 MFMAs sum all 16
// channels of the chunk.  Per step 240 MFMAs (7680 cycles) per wave, two waves
// per SIMD: 15.4k MFMA cycles per barrier.

constexpr int kF5Slot = 3 * 160 * 16;                 // floats per weight slice (3 taps x 160 co x 16 ci)

template <int EPI>
__global__ void __launch_bounds__(512) conv3d_k3_f32_kernel(ConvF32Args a) {
    constexpr int LD = 16;
    constexpr int CO = 160;
    constexpr int HSZ = kHalo * LD;                      // floats per halo buffer (38.4 KB)
    __shared__ __attribute__((aligned(16))) float smem_f5[2 * HSZ + 2 * kF5Slot];   // 138.2 KB
    float* Ws = smem_f5 + 2 * HSZ;

    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int nYt = (nY + 1) >> 1, nXt = (nX + 1) >> 1;
    int bid = blockIdx.x;
    const int txx = bid % nXt; bid /= nXt;
    const int tyy = bid % nYt; bid /= nYt;
    const int pt = bid % nT;
    const int b = bid / nT;
    const int t0 = pt * 4, y0 = tyy * 8, x0 = txx * 8;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pw = wave & 3, nh = wave >> 2;
    const int ncc = a.cin_pad / LD;
    const int nsteps = ncc * 9;                          // step s: chunk s / 9, tap row s % 9

    constexpr int HPER = (kHalo * 4 + 511) / 512;        // 5
    f32x4_t hr[HPER];
    int hoff[HPER];
#pragma unroll
    for (int k = 0; k < HPER; ++k) {
        const int i = threadIdx.x + k * 512;
        hoff[k] = -1;
        if (i < kHalo * 4) {
            const int hv = i >> 2, c4 = (i & 3) * 4;
            const int ht = hv / (kHaloY * kHaloX), hy = (hv / kHaloX) % kHaloY, hx = hv % kHaloX;
            const int t = t0 - 1 + ht, y = y0 - 1 + hy, x = x0 - 1 + hx;
            if (t >= 0 && t < a.D && y >= 0 && y < a.H && x >= 0 && x < a.W)
                hoff[k] = (int)(brow(b, t, y, x, nT, nY, nX) * a.cin_ld + c4);
        }
    }
    auto load_halo = [&](int cc) {
        const float* base = a.in + cc * LD;
#pragma unroll
        for (int k = 0; k < HPER; ++k) {
            hr[k] = (f32x4_t)0.0f;
            if (hoff[k] >= 0) hr[k] = *reinterpret_cast<const f32x4_t*>(base + hoff[k]);
        }
    };
    auto store_halo = [&](int buf) {
        float* Hs = smem_f5 + buf * HSZ;
#pragma unroll
        for (int k = 0; k < HPER; ++k) {
            const int i = threadIdx.x + k * 512;
            if (i < kHalo * 4) {
                const int hv = i >> 2, c = i & 3;
                const int hy = (hv / kHaloX) % kHaloY;
                *reinterpret_cast<f32x4_t*>(Hs + hv * LD + ((c ^ ((hy & 1) << 1)) << 2)) = hr[k];
            }
        }
    };
    const unsigned wbase = lds_offset(Ws);
    unsigned woff[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int wi = k * 8 + wave;
        const int c = wi * 64 + lane;
        const int row = c >> 2, pos = c & 3;
        const int tl = row >= 2 * CO ? 2 : (row >= CO ? 1 : 0);
        const int co = row - tl * CO;
        const int kl = pos ^ ((4 - ((co & 15) >> 2)) & 3);
        woff[k] = (unsigned)(((tl * CO + co) * a.cin_pad + (kl << 2)) * 4);
    }
    auto issue_w = [&](int s) {
        const int cc = s / 9, t3 = (s % 9) * 3;
        const unsigned dst = wbase + (unsigned)((s & 1) * kF5Slot * 4);
        const float* src = a.w + (long)t3 * CO * a.cin_pad + cc * LD;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int wi = k * 8 + wave;
            if (wi < 30) glds16_s(src, woff[k], dst + wi * 1024);
        }
    };

    f32x4_t acc[4][5];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) acc[i][j] = (f32x4_t)0.0f;

    const int pyy = pw >> 1, pxx = pw & 1;
    const int vq = lane & 15, cq = lane >> 4;
    const int ly = pyy * 4 + ((vq >> 2) & 3), lx = pxx * 4 + (vq & 3);
    const int hb0 = ly * kHaloX + lx;
    const int corow = nh * 80 + vq;
    const int bpos = (cq ^ ((4 - (vq >> 2)) & 3)) << 2;

    auto read_frags = [&](int s, int kw, f32x4_t (&af)[4], f32x4_t (&bfr)[5]) {
        const int st = s % 9, kd = st / 3, kh = st % 3;
        const int apos = (cq ^ (((ly + kh) & 1) << 1)) << 2;
        const int toff = (kd * kHaloY + kh) * kHaloX + kw;
        const float* Hs = smem_f5 + ((s / 9) & 1) * HSZ;
        const float* wb = Ws + (s & 1) * kF5Slot;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            af[i] = *reinterpret_cast<const f32x4_t*>(Hs + (hb0 + i * kHaloY * kHaloX + toff) * LD + apos);
#pragma unroll
        for (int j = 0; j < 5; ++j)
            bfr[j] = *reinterpret_cast<const f32x4_t*>(wb + (kw * CO + corow + j * 16) * LD + bpos);
    };
    auto mma = [&](const f32x4_t (&af)[4], const f32x4_t (&bfr)[5]) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 5; ++j) mfma4f(acc[i][j], af[i][e], bfr[j][e]);
    };

    load_halo(0);
    issue_w(0);
    store_halo(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    if (wave >= 4) __builtin_amdgcn_s_setprio(1);
    for (int s = 0; s < nsteps; ++s) {
        const int sc = s % 9;
        const bool seam = (sc == 8) && (s + 1 < nsteps);
        if (sc == 7 && s + 2 < nsteps) load_halo(s / 9 + 1);
        const bool dma = s + 1 < nsteps;
        f32x4_t afA[4], bfA[5], afB[4], bfB[5];
        if (dma && wave < 4) issue_w(s + 1);
        read_frags(s, 0, afA, bfA);
        read_frags(s, 1, afB, bfB);
        mma(afA, bfA);
        if (dma && wave >= 4) issue_w(s + 1);
        read_frags(s, 2, afA, bfA);
        mma(afB, bfB);
        mma(afA, bfA);
        if (seam) store_halo((s / 9 + 1) & 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    conv_epilogue_f32<EPI>(a, acc, smem_f5, pw, nh * 80, lane, b, pt, tyy * 2, txx * 2, nT, nY, nX);
}

static int conv_f32_c160_launch(const ConvArgs& a, hipStream_t st) {
    ConvF32Args v{};
    v.in = (const float*)a.in; v.w = (const float*)a.w; v.bias = a.bias; v.out = (float*)a.out;
    v.mask = (const float*)a.mask; v.res = (const float*)a.res;
    v.B = a.B; v.D = a.D; v.H = a.H; v.W = a.W; v.cin_ld = a.cin_ld; v.cin_pad = a.cin_pad;
    v.cout_ld = a.cout_ld; v.mask_ld = a.mask_ld; v.res_ld = a.res_ld; v.accumulate = a.accumulate;
    v.relu_out = a.relu_out; v.res_scale = a.res_scale;
    const unsigned nblk = (unsigned)conv_tiles(a.B, a.D, a.H, a.W);
    const int epi = conv_epi_code(v.res, v.mask, !v.accumulate, true);
    if (epi == 0) hipLaunchKernelGGL(conv3d_k3_f32_kernel<0>, dim3(nblk), dim3(512), 0, st, v);
    else if (epi == kEpiRes) hipLaunchKernelGGL(conv3d_k3_f32_kernel<kEpiRes>, dim3(nblk), dim3(512), 0, st, v);
    else if (epi == kEpiMask) hipLaunchKernelGGL(conv3d_k3_f32_kernel<kEpiMask>, dim3(nblk), dim3(512), 0, st, v);
    else hipLaunchKernelGGL(conv3d_k3_f32_kernel<kEpiGeneric>, dim3(nblk), dim3(512), 0, st, v);
    return dlcs_launch_status();
}

// ---------------------------------------------------------------- wgrad, 160 <-> thin (fp32)
// The ConvBlocks' thin ends: SFE 4 -> 160 (dW[tap][co][ci < 4]) and the final
// 160 -> 4 (dW[tap][co < 4][ci]).  As in the bf16 kernel the tap shift is put on
// the thin side (u = v + off:  sum_v g[v] x[v + off] = sum_u x[u] g[u - off]):
//   dW = Big^T . Thin_im2col,  Big[u][b] (160 channels, unshifted, K = voxels)
//   Thin_im2col[u][(tap, s)] = Thin[u + sgn off(tap)][s]   (27 taps x 4 = 108 -> 7 tiles)
// With the f32 MFMA the im2col never materialises: lane (k = voxel, n = (tap,
// s)) of the B operand reads its one float straight from the patch's 6x6x6
// thin halo in LDS (per-lane constant offset + per-k-step immediate).  One
// workgroup = a patch range, 8 waves = big half bh (80 channels, 5 tiles) x
// k-phase kq (k-steps s = kq mod 4 of a patch's 16): 35 accumulator tiles per
// wave; per 64-voxel patch the big rows (40 KB) and the thin halo (3.4 KB) are
// DMA'd into one of two buffers while the other is multiplied.
struct ThinWgF32Args {
    const float* big; const float* thin; float* dw;
    int big_ld, thin_ld, sgn, big_is_co, thin_ch, cout_pad, cin_pad;
    int B, D, H, W;
};
constexpr int kTwBigF = 64 * 160;                       // floats of big rows per buffer
constexpr int kTwBufF = kTwBigF + 216 * 4;              // + thin halo (16 B per row)

__global__ void __launch_bounds__(512) conv3d_wgrad_thin_f32_kernel(ThinWgF32Args a, int nrange, int ppr) {
    __shared__ __attribute__((aligned(16))) float smem[2 * kTwBufF];         // 88.8 KB
    const int range = blockIdx.x;
    if (range >= nrange) return;
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int npatch = a.B * nT * nY * nX;
    const int p0 = range * ppr, p1 = min(npatch, p0 + ppr);
    if (p0 >= p1) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bh = wave & 1, kq = wave >> 1;
    const float* zrow = reinterpret_cast<const float*>(g_wf_zero_row);
    const unsigned sbase = lds_offset(smem);

    auto issue = [&](int patch, int buf) {
        const int px = patch % nX;
        int r = patch / nX;
        const int py = r % nY; r /= nY;
        const int pt = r % nT;
        const int bb = r / nT;
        const unsigned dst = sbase + buf * kTwBufF * 4;
        int ln = lane;
        asm volatile("" : "+v"(ln));
#pragma unroll
        for (int k = 0; k < 5; ++k) {                  // big rows: 64 x 40 chunks = 40 wave-instructions
            const int wi = k * 8 + wave;
            const int c = wi * 64 + ln;
            const int row = c / 40, kp = c - row * 40;
            const int kl = kp ^ ((row & 1) << 2);
            glds16(a.big + (long)(patch * 64 + row) * a.big_ld + (kl << 2), dst + wi * 1024);
        }
        if (wave < 4) {                                // thin halo: 216 rows x 16 B
            const int c = wave * 64 + ln;
            if (c < 216) {
                const int hz = c / 36, hy = (c / 6) % 6, hx = c % 6;
                const int T = pt * 4 + hz - 1, Y = py * 4 + hy - 1, X = px * 4 + hx - 1;
                const bool ok = (unsigned)T < (unsigned)a.D && (unsigned)Y < (unsigned)a.H && (unsigned)X < (unsigned)a.W;
                const int vrow = ((((bb * nT + (T >> 2)) * nY + (Y >> 2)) * nX + (X >> 2)) << 6) + ((T & 3) << 4) +
                                 ((Y & 3) << 2) + (X & 3);
                glds16(ok ? a.thin + (long)vrow * a.thin_ld : zrow, dst + kTwBigF * 4 + wave * 1024);
            }
        }
    };

    f32x4_t acc[5][7];
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 7; ++j) acc[i][j] = (f32x4_t)0.0f;

    // A: big row = voxel 4 s + q, channel bh * 80 + 16 i + m (swizzled by row parity q & 1)
    // B: thin halo row of (voxel 4 s + q) shifted by sgn * off(tap), tap = 4 j + (m >> 2), channel m & 3
    const int q = lane >> 4, m = lane & 15;
    int aoff[5], boff[7];
#pragma unroll
    for (int i = 0; i < 5; ++i) aoff[i] = q * 160 + (((bh * 5 + i) ^ (q & 1)) << 4) + m;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        int tap = 4 * j + (m >> 2);
        tap = tap < 27 ? tap : 26;                     // padding columns: discarded at the flush
        const int kd = tap / 9 - 1, kh = (tap / 3) % 3 - 1, kw = tap % 3 - 1;
        // voxel (t, y, x = q) of k-step s: halo row ((t+1+sgn kd) 6 + (y+1+sgn kh)) 6 + (q+1+sgn kw)
        boff[j] = kTwBigF + (((1 + a.sgn * kd) * 6 + (1 + a.sgn * kh)) * 6 + (q + 1 + a.sgn * kw)) * 4 + (m & 3);
    }

    issue(p0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int patch = p0; patch < p1; ++patch) {
        const int cur = (patch - p0) & 1;
        if (patch + 1 < p1) issue(patch + 1, cur ^ 1);
        const float* S = smem + cur * kTwBufF;
#pragma unroll
        for (int ss = 0; ss < 4; ++ss) {
            const int s = 4 * ss + kq;                   // k-step: voxels 4 s .. 4 s + 3 = (t, y, x 0..3)
            const int t = s >> 2, y = s & 3;
            const int arow = 4 * s * 160, hrow = (t * 36 + y * 6) * 4;
            float af[5], bfv[7];
#pragma unroll
            for (int i = 0; i < 5; ++i) af[i] = S[aoff[i] + arow];
#pragma unroll
            for (int j = 0; j < 7; ++j) bfv[j] = S[boff[j] + hrow];
#pragma unroll
            for (int j = 0; j < 7; ++j)
#pragma unroll
                for (int i = 0; i < 5; ++i) mfma4f(acc[i][j], af[i], bfv[j]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 7; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int bch = bh * 80 + 16 * i + 4 * q + r, n = 16 * j + m;
                const int tap = n >> 2, sc = n & 3;
                if (tap < 27 && sc < a.thin_ch) {
                    const int co = a.big_is_co ? bch : sc, ci = a.big_is_co ? sc : bch;
                    atomicAdd(a.dw + ((long)tap * a.cout_pad + co) * a.cin_pad + ci, acc[i][j][r]);
                }
            }
}

// ---------------------------------------------------------------- forward / dgrad, thin input (fp32)
// Cin <= 4 -> 160: the SFE conv (s3d:384) and the dgrad of the final conv
// (s3d:391).  K = 27 taps x 4 channels and the f32 MFMA's K is 4, so a k-step
// is exactly one tap: lane (voxel m, channel k) reads its one float of the
// [600][4] halo, and the B operand its weight from a [27][4][176] (co-
// contiguous, padded) image that stays in LDS for the persistent workgroup.
// Tiles, waves and epilogue as the 160 kernel (256 voxels x 160, 8 waves of
// 4 x 5 tiles); the next tile's halo is register-prefetched during the MFMAs.
constexpr int kTiWld = 176;

template <int EPI>
__global__ void __launch_bounds__(512) conv3d_thin_in_f32_kernel(ConvF32Args a, int ntiles) {
    __shared__ __attribute__((aligned(16))) float smem_ti[27 * 4 * kTiWld + kHalo * 4 + 256 * 36];
    float* Wt = smem_ti;
    float* Hs = smem_ti + 27 * 4 * kTiWld;
    float* Es = Hs + kHalo * 4;
    for (int it = threadIdx.x; it < 27 * 4 * 160; it += 512) {
        const int co = it % 160, k = (it / 160) & 3, tap = it / 640;
        Wt[(tap * 4 + k) * kTiWld + co] = a.w[((long)tap * 160 + co) * a.cin_pad + k];
    }
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int nYt = (nY + 1) >> 1, nXt = (nX + 1) >> 1;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pw = wave & 3, nh = wave >> 2;
    const int m = lane & 15, k = lane >> 4;
    const int ly = (pw >> 1) * 4 + ((m >> 2) & 3), lx = (pw & 1) * 4 + (m & 3);
    const int abase = (ly * kHaloX + lx) * 4 + k;
    const int bbase = k * kTiWld + nh * 80 + m;
    auto decode = [&](int tile, int& b, int& pt, int& tyy, int& txx) {
        int bid = tile;
        txx = bid % nXt; bid /= nXt;
        tyy = bid % nYt; bid /= nYt;
        pt = bid % nT;
        b = bid / nT;
    };
    constexpr int HPER = (kHalo + 511) / 512;           // 2
    f32x4_t hreg[HPER];
    const float* zrow = reinterpret_cast<const float*>(g_wf_zero_row);
    auto load_halo = [&](int tile) {
        int b, pt, tyy, txx;
        decode(tile, b, pt, tyy, txx);
#pragma unroll
        for (int kk = 0; kk < HPER; ++kk) {
            const int hv = threadIdx.x + 512 * kk;
            const int ht = hv / (kHaloY * kHaloX), hy = (hv / kHaloX) % kHaloY, hx = hv % kHaloX;
            const int t = pt * 4 - 1 + ht, y = tyy * 8 - 1 + hy, x = txx * 8 - 1 + hx;
            const bool ok = hv < kHalo && t >= 0 && t < a.D && y >= 0 && y < a.H && x >= 0 && x < a.W;
            const float* src = ok ? a.in + brow(b, t, y, x, nT, nY, nX) * a.cin_ld : zrow;
            hreg[kk] = *reinterpret_cast<const f32x4_t*>(src);
        }
    };
    int tile = blockIdx.x;
    if (tile < ntiles) load_halo(tile);
    for (; tile < ntiles; tile += gridDim.x) {
        int b, pt, tyy, txx;
        decode(tile, b, pt, tyy, txx);
#pragma unroll
        for (int kk = 0; kk < HPER; ++kk) {
            const int hv = threadIdx.x + 512 * kk;
            if (hv < kHalo) *reinterpret_cast<f32x4_t*>(Hs + hv * 4) = hreg[kk];
        }
        __syncthreads();
        if (tile + (int)gridDim.x < ntiles) load_halo(tile + gridDim.x);
        f32x4_t acc[4][5];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) acc[i][j] = (f32x4_t)0.0f;
#pragma unroll 3
        for (int tap = 0; tap < 27; ++tap) {
            const int toff = ((tap / 9) * kHaloY + (tap / 3) % 3) * kHaloX + tap % 3;
            float af[4], bfv[5];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = Hs[abase + (i * kHaloY * kHaloX + toff) * 4];
#pragma unroll
            for (int j = 0; j < 5; ++j) bfv[j] = Wt[bbase + tap * 4 * kTiWld + 16 * j];
#pragma unroll
            for (int j = 0; j < 5; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) mfma4f(acc[i][j], af[i], bfv[j]);
        }
        conv_epilogue_f32<EPI, 5>(a, acc, Es, pw, nh * 80, lane, b, pt, tyy * 2, txx * 2, nT, nY, nX);
    }
}

// ---------------------------------------------------------------- forward / dgrad, thin output (fp32)
// 160 -> Cout <= 4: the final conv (s3d:391) and the dgrad of the SFE conv
// (s3d:384).  N = 4 output channels would waste 3/4 of a 16-wide MFMA tile, so
// the kw taps ride in N:  Q[(t, y, x')][(kw, co)] = sum_{kd, kh, ci}
// W[kd, kh, kw][co][ci] x[t + kd - 1, y + kh - 1, x' - 1][ci] over the tile's
// rows with the halo x extent (x' = 0..9), N = 3 x 4 = 12 of 16 used, K = 9 x
// 160; then out[t, y, x][co] = sum_kw Q[(t, y, x + kw)][(kw, co)] (one LDS
// round trip per tile).  Tile 256 voxels (4 t x 8 y x 8 x) = 320 Q rows = 20
// M tiles over 4 waves; K walked per 16-channel chunk of the [600][16] halo
// (register-prefetched, v5 swizzle) with the 4-MFMA b128 fragment trick.
template <int EPI>
__global__ void __launch_bounds__(256) conv3d_thin_out_f32_kernel(ConvF32Args a, int ntiles) {
    constexpr int LD = 16, NWLD = 20;                    // weight image [9][16 n][16 ci + 4]
    __shared__ __attribute__((aligned(16))) float smem_to[kHalo * LD + 9 * 16 * NWLD];
    float* Hs = smem_to;
    float* Wk = smem_to + kHalo * LD;
    float* Q = smem_to;                                  // [320][17] after the K loop (aliases the halo)
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int nYt = (nY + 1) >> 1, nXt = (nX + 1) >> 1;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, cq = lane >> 4;
    const int ncc = a.cin_pad / LD;
    // A rows of this lane: Q row r = 16 (5 wave + i) + m = (t 8 + y) 10 + x'
    int hb[5], hyp[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int r = 16 * (5 * wave + i) + m;
        const int xp = r % 10, y = (r / 10) % 8, t = r / 80;
        hb[i] = (t * kHaloY + y) * kHaloX + xp;
        hyp[i] = y & 1;
    }
    constexpr int HPER = (kHalo * 4 + 255) / 256;        // 10
    f32x4_t hr[HPER];
    auto load_halo = [&](int b, int pt, int tyy, int txx, int cc) {
#pragma unroll
        for (int k = 0; k < HPER; ++k) {
            const int i = threadIdx.x + k * 256;
            hr[k] = (f32x4_t)0.0f;
            if (i < kHalo * 4) {
                const int hv = i >> 2, c4 = (i & 3) * 4;
                const int ht = hv / (kHaloY * kHaloX), hy = (hv / kHaloX) % kHaloY, hx = hv % kHaloX;
                const int t = pt * 4 - 1 + ht, y = tyy * 8 - 1 + hy, x = txx * 8 - 1 + hx;
                if (t >= 0 && t < a.D && y >= 0 && y < a.H && x >= 0 && x < a.W)
                    hr[k] = *reinterpret_cast<const f32x4_t*>(a.in + brow(b, t, y, x, nT, nY, nX) * a.cin_ld + cc * LD + c4);
            }
        }
    };
    auto store_halo = [&]() {
#pragma unroll
        for (int k = 0; k < HPER; ++k) {
            const int i = threadIdx.x + k * 256;
            if (i < kHalo * 4) {
                const int hv = i >> 2, c = i & 3;
                const int hy = (hv / kHaloX) % kHaloY;
                *reinterpret_cast<f32x4_t*>(Hs + hv * LD + ((c ^ ((hy & 1) << 1)) << 2)) = hr[k];
            }
        }
    };
    // weights of chunk cc: Wk[(kd, kh)][n = kw * 4 + co][ci] (n >= 12 or co >= Cout: 0)
    auto store_w = [&](int cc) {
        for (int it = threadIdx.x; it < 9 * 16 * 4; it += 256) {
            const int c4 = (it & 3) * 4, n = (it >> 2) & 15, kk = it >> 6;
            const int kw = n >> 2, co = n & 3;
            f32x4_t v = (f32x4_t)0.0f;
            if (kw < 3 && co < a.cout) {
                const int tap = kk * 3 + kw;
                v = *reinterpret_cast<const f32x4_t*>(a.w + ((long)tap * a.cout_pad + co) * a.cin_pad + cc * LD + c4);
            }
            *reinterpret_cast<f32x4_t*>(Wk + (kk * 16 + n) * NWLD + c4) = v;
        }
    };
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int bid = tile;
        const int txx = bid % nXt; bid /= nXt;
        const int tyy = bid % nYt; bid /= nYt;
        const int pt = bid % nT;
        const int b = bid / nT;
        f32x4_t acc[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) acc[i] = (f32x4_t)0.0f;
        load_halo(b, pt, tyy, txx, 0);
        for (int cc = 0; cc < ncc; ++cc) {
            __syncthreads();                             // previous chunk's / tile's readers are done
            store_halo();
            store_w(cc);
            __syncthreads();
            if (cc + 1 < ncc) load_halo(b, pt, tyy, txx, cc + 1);
#pragma unroll 3
            for (int kk = 0; kk < 9; ++kk) {
                const int kd = kk / 3, kh = kk % 3;
                const f32x4_t bfr = *reinterpret_cast<const f32x4_t*>(Wk + (kk * 16 + m) * NWLD + 4 * cq);
                f32x4_t af[5];
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const int pos = (cq ^ (((hyp[i] + kh) & 1) << 1)) << 2;
                    af[i] = *reinterpret_cast<const f32x4_t*>(Hs + (hb[i] + kd * kHaloY * kHaloX + kh * kHaloX) * LD + pos);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < 5; ++i) mfma4f(acc[i], af[i][e], bfr[e]);
            }
        }
        __syncthreads();
        // Q rows -> LDS [320][17]; C/D row = 4 cq + r, col n = m
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) Q[(16 * (5 * wave + i) + 4 * cq + r) * 17 + m] = acc[i][r];
        __syncthreads();
        {   // one output voxel per thread: 4 t x 8 y x 8 x
            const int v = threadIdx.x;
            const int t = v >> 6, y = (v >> 3) & 7, x = v & 7;
            const int py = tyy * 2 + (y >> 2), px = txx * 2 + (x >> 2);
            if (py < nY && px < nX) {
                f32x4_t o = (f32x4_t)0.0f;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const float* qr = Q + ((t * 8 + y) * 10 + x + kw) * 17 + kw * 4;
#pragma unroll
                    for (int co = 0; co < 4; ++co) o[co] += qr[co];
                }
                const long row = brow(b, pt * 4 + t, py * 4 + (y & 3), px * 4 + (x & 3), nT, nY, nX);
                float* op = a.out + row * a.cout_ld;
                if (a.bias) for (int co = 0; co < a.cout; ++co) o[co] += a.bias[co];
                if (a.relu_out) for (int co = 0; co < 4; ++co) o[co] = fmaxf(o[co], 0.0f);
                if (a.accumulate) o += *reinterpret_cast<const f32x4_t*>(op);
                *reinterpret_cast<f32x4_t*>(op) = o;
            }
        }
    }
}

static int conv_f32_thin_launch(const ConvArgs& a, hipStream_t st, bool thin_in) {
    ConvF32Args v{};
    v.in = (const float*)a.in; v.w = (const float*)a.w; v.bias = a.bias; v.out = (float*)a.out;
    v.mask = (const float*)a.mask; v.res = (const float*)a.res;
    v.B = a.B; v.D = a.D; v.H = a.H; v.W = a.W; v.cin_ld = a.cin_ld; v.cin_pad = a.cin_pad;
    v.cout_ld = a.cout_ld; v.mask_ld = a.mask_ld; v.res_ld = a.res_ld; v.accumulate = a.accumulate;
    v.relu_out = a.relu_out; v.res_scale = a.res_scale; v.cout = a.Cout; v.cout_pad = a.cout_pad;
    const int ntiles = (int)conv_tiles(a.B, a.D, a.H, a.W);
    if (thin_in) {
        const dim3 g(std::min(ntiles, 256));
        const int epi = conv_epi_code(v.res, v.mask, !v.accumulate, false);
        if (epi == 0) hipLaunchKernelGGL(conv3d_thin_in_f32_kernel<0>, g, dim3(512), 0, st, v, ntiles);
        else if (epi == kEpiMask) hipLaunchKernelGGL(conv3d_thin_in_f32_kernel<kEpiMask>, g, dim3(512), 0, st, v, ntiles);
        else hipLaunchKernelGGL(conv3d_thin_in_f32_kernel<kEpiGeneric>, g, dim3(512), 0, st, v, ntiles);
    } else {
        const dim3 g(std::min(ntiles, 512));
        hipLaunchKernelGGL(conv3d_thin_out_f32_kernel<0>, g, dim3(256), 0, st, v, ntiles);
    }
    return dlcs_launch_status();
}
