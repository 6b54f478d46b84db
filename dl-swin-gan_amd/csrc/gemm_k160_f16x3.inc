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
