// ---------------------------------------------------------------- bf16 Conv3d 160 -> 160, v7
// Included by conv3d.hip.  The bf16 160-channel forward / input
// gradient (s3d:336, :356; config 2's dtype) with TWO workgroups per CU.  The v6
// kernel (one 157.5 KB workgroup of 8 waves per CU) pays every barrier, end-of-step
// drain and epilogue with the whole CU idle; here the unit of work is half of v6's
// tile so two independent workgroups share a CU and one's barrier / DMA wait /
// epilogue runs under the other's matrix work:
//   * unit = (tile of 256 voxels = 1 x 2 x 2 patches, output-channel half of 80):
//     4 waves, one patch each, 4 x 5 tiles of 16 x 16 per wave (the v6 wave's
//     work and fragments, v_mfma_f32_16x16x32_bf16, K walked in 32-channel chunks);
//   * a step is one tap row (kd, kh) = three taps (60 MFMAs per wave between
//     barriers), 9 steps per chunk;
//   * LDS: ONE halo image [600][32] (38.4 KB) + two weight slots of three tap slices
//     [3][80][32] (2 x 15 KB) = 68.4 KB per workgroup; the epilogue reuses it in two
//     40-channel passes (45 KB);
//   * the next chunk's halo: time slices 0-1 (rows < 192 of the image), which no tap
//     reads after the kd = 1 rows (steps 0-5), are DMA'd straight into the live image
//     during step 6; the rest waits in registers (7 x 16 B per lane) and is stored
//     behind an extra barrier at the chunk seam;
//   * units numbered XCD-major with the two halves of a tile adjacent (one L2 serves
//     the halo to both), the last partial round of 512 workgroups split into 5
//     single-chunk workgroups per unit + a fixed-order reduce (run-to-run
//     deterministic), as the v6 / f16x3 launches.
// Weights: dlcs_conv3d_pack_weights bf16 modes 0 / 1 (the v5 packing, cin_pad 160).
// Measured at parity with v6, not faster (same box: microbench fwd 1.095-1.106 vs
// 1.083-1.085 ms, dgrad 1.079-1.090 vs 1.072-1.074; in the bf16 step fwd 988-1026 vs
// 1001-1008 us, dgrad 959-963 vs 978-983 us), so v6 stays the default and v7 runs
// under the DLCS_CONV_V7=1 test hook.  DIAG bits (DLCS_V7_EXP) show why: with the
// wave's tile unchanged a SIMD still holds 2 waves, and the MFMA work and the rest
// (fragment reads, DMA, barriers, epilogue) add instead of overlapping.
constexpr int kV7Co = 80;                               // output channels per unit
constexpr int kV7Slot = 3 * kV7Co * 32;                 // bf16 per weight slot (3 taps x 80 co x 32 ci)
constexpr int kV7Steps = 9;                             // tap rows per chunk

// unit vb (XCD-major virtual numbering over nunit = 2 nblk units) -> tile (b, pt, tyy, txx), half nh
DLCS_DEV void v7_unit(int vb, int nunit, int nT, int nYt, int nXt, int& b, int& pt, int& tyy, int& txx, int& nh) {
    const int q8 = nunit >> 3, r8 = nunit & 7, xcd = vb & 7;
    const int u = xcd * q8 + min(xcd, r8) + (vb >> 3);
    nh = u & 1;
    int bid = u >> 1;
    txx = bid % nXt; bid /= nXt;
    tyy = bid % nYt; bid /= nYt;
    pt = bid % nT;
    b = bid / nT;
}

template <int EPI, bool TAIL>
__global__ void __launch_bounds__(256, 2) conv3d_k3_v7_kernel(ConvV6Args g) {
    const ConvV2Args& a = g.v;
    constexpr int LD = 32, CO = kV7Co;
    constexpr int HSZ = kHalo * LD;                     // bf16 in the halo image
    __shared__ __attribute__((aligned(16))) bf16 smem_v7[HSZ + 2 * kV7Slot];   // 68.4 KB
    bf16* Hs = smem_v7;
    bf16* Ws = smem_v7 + HSZ;

    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int nYt = (nY + 1) >> 1, nXt = (nX + 1) >> 1;
    const int nunit = 2 * a.B * nT * nYt * nXt;
    const int cc0 = TAIL ? (int)blockIdx.x % 5 : 0;
    const int cc1 = TAIL ? cc0 + 1 : 5;
    int b, pt, tyy, txx, nh;
    v7_unit(TAIL ? g.tail_base + (int)blockIdx.x / 5 : (int)blockIdx.x, nunit, nT, nYt, nXt, b, pt, tyy, txx, nh);
    const int t0 = pt * 4, y0 = tyy * 8, x0 = txx * 8;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // the wave's patch of the tile

    // halo pieces: 600 rows x 4 16-B chunks = 2400, piece i = threadIdx + 256 k (k < 10)
    constexpr int HP = 10, HD = 3, HR = HP - HD;
    bf16x8_t hr[HR];
    auto halo_off = [&](int k) {                        // element offset of piece k (channel chunk 0), -1 off the grid
        const int i = threadIdx.x + k * 256;
        int off = -1;
        if (i < kHalo * 4) {
            const int hv = i >> 2, c = i & 3;
            const int ht = hv / (kHaloY * kHaloX), hy = (hv / kHaloX) % kHaloY, hx = hv % kHaloX;
            const int t = t0 - 1 + ht, y = y0 - 1 + hy, x = x0 - 1 + hx;
            if (t >= 0 && t < a.D && y >= 0 && y < a.H && x >= 0 && x < a.W)
                off = (int)(brow(b, t, y, x, nT, nY, nX) * a.cin_ld + ((c ^ ((hy & 1) << 1)) << 3));
        }
        return off;
    };
    const unsigned hbase = lds_offset(Hs);
    auto dma_halo = [&](int cc) {                       // pieces k < HD (rows < 192): LDS position i
#pragma unroll
        for (int k = 0; k < HD; ++k) {
            const int off = halo_off(k);
            glds16(off >= 0 ? (const void*)(a.in + cc * CK + off) : (const void*)g_wg_zero_row,
                   hbase + (unsigned)((k * 256 + wave * 64) * 16));
        }
    };
    auto load_halo = [&](int cc) {
#pragma unroll
        for (int k = 0; k < HR; ++k) {
            const int off = halo_off(HD + k);
            hr[k] = (bf16x8_t)(bf16)0.0f;
            if (off >= 0) hr[k] = *reinterpret_cast<const bf16x8_t*>(a.in + cc * CK + off);
        }
    };
    auto store_halo = [&]() {
#pragma unroll
        for (int k = 0; k < HR; ++k) {
            const int i = threadIdx.x + (HD + k) * 256;
            if (i < kHalo * 4) *reinterpret_cast<bf16x8_t*>(Hs + i * 8) = hr[k];
        }
    };
    // weight DMA of step s (chunk s / 9, tap row s % 9) into slot s & 1: the row's three
    // taps x this unit's 80 output channels, 15 x 1 KB pieces, piece wi by wave wi % 4;
    // LDS chunk c of the slot: row (c >> 2) = tap-in-slot * 80 + co, position c & 3 <-
    // logical chunk (c & 3) ^ swz(co) (the v5 / v6 weight swizzle)
    const unsigned wbase = lds_offset(Ws);
    unsigned woff[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int wi = k * 4 + wave;
        const int c = wi * 64 + lane;
        const int row = c >> 2, pos = c & 3;
        const int tl = row / CO, co = row - tl * CO;
        const int kl = pos ^ ((4 - ((co & 15) >> 2)) & 3);
        woff[k] = (unsigned)(((tl * 160 + nh * CO + co) * a.cin_pad + (kl << 3)) * 2);
    }
    auto issue_w = [&](int s) {
        const int cc = s / kV7Steps, sp = s % kV7Steps;
        const unsigned dst = wbase + (unsigned)((s & 1) * kV7Slot * 2);
        const bf16* src = a.w + (long)(3 * sp) * 160 * a.cin_pad + cc * CK;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int wi = k * 4 + wave;
            if (wi < 15) glds16_s(src, woff[k], dst + wi * 1024);
        }
    };

    f32x4_t acc[4][5];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) acc[i][j] = (f32x4_t)0.0f;

    const int pyy = wave >> 1, pxx = wave & 1;
    const int vq = lane & 15, cq = lane >> 4;
    const int ly = pyy * 4 + ((vq >> 2) & 3), lx = pxx * 4 + (vq & 3);
    const int hb0 = ly * kHaloX + lx;
    const int bpos = (cq ^ ((4 - (vq >> 2)) & 3)) << 3;

    // fragments of tap kw = ti of step s (tap row s % 9)
    auto read_frags = [&](int s, int ti, bf16x8_t (&af)[4], bf16x8_t (&bfr)[5]) {
#ifdef DLCS_DIAG_BUILD
        if (g.exp & 64) {                                // DIAG: no LDS reads (register-made fragments)
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = (bf16x8_t)(bf16)(float)(lane + i + ti);
#pragma unroll
            for (int j = 0; j < 5; ++j) bfr[j] = (bf16x8_t)(bf16)(float)(lane - j + s);
            return;
        }
#endif
        const int sp = s % kV7Steps;
        const int kd = sp / 3, kh = sp % 3;
        const int apos = (cq ^ (((ly + kh) & 1) << 1)) << 3;
        const int toff = (kd * kHaloY + kh) * kHaloX + ti;
        const bf16* wb = Ws + (s & 1) * kV7Slot;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            af[i] = *reinterpret_cast<const bf16x8_t*>(Hs + (hb0 + i * kHaloY * kHaloX + toff) * LD + apos);
#pragma unroll
        for (int j = 0; j < 5; ++j)
            bfr[j] = *reinterpret_cast<const bf16x8_t*>(wb + (ti * CO + vq + j * 16) * LD + bpos);
    };
    auto mma = [&](const bf16x8_t (&af)[4], const bf16x8_t (&bfr)[5]) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) mfma16(acc[i][j], af[i], bfr[j]);
    };

#ifdef DLCS_DIAG_BUILD
    // DLCS_V7_EXP (DIAG timing experiments; 1, 2, 4, 8 make the results wrong): 1 no
    // end-of-step vmcnt wait, 2 no end-of-step barrier, 4 no MFMAs, 8 no weight DMA after
    // the prologue, 16 the next step's weight DMA issued before the step's first reads, 32 no
    // epilogue, 64 no fragment reads from LDS
    const int xexp = g.exp;
#else
    constexpr int xexp = 0;
#endif
    const int send = cc1 * kV7Steps;                    // one past the last step of this workgroup
    dma_halo(cc0);
    load_halo(cc0);
    issue_w(cc0 * kV7Steps);
    store_halo();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int cc = cc0; cc < cc1; ++cc) {
#pragma unroll 1
        for (int sp = 0; sp < kV7Steps; ++sp) {
            const int s = cc * kV7Steps + sp;
            if (sp == 6 && cc + 1 < cc1) {              // time slices 0-1 are dead from step 6 on
                dma_halo(cc + 1);
                load_halo(cc + 1);
            }
            bf16x8_t afA[4], bfA[5], afB[4], bfB[5];
            const bool wdma = s + 1 < send && !(xexp & 8);
            if ((xexp & 16) && wdma) issue_w(s + 1);
            read_frags(s, 0, afA, bfA);
            read_frags(s, 1, afB, bfB);
            if (xexp & 4) {                             // DIAG: operands consumed, no matrix work
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[i][0][0] += (float)afA[i][0] + (float)afB[i][1] + (float)bfA[i][2] + (float)bfB[i][3];
                read_frags(s, 2, afA, bfA);
                acc[0][1][0] += (float)afA[0][0] + (float)bfA[4][1];
            } else {
                // scheduling fences as in the v6 kernel (128: off)
                auto SB = [&]() { if (!(xexp & 128)) __builtin_amdgcn_sched_barrier(0); };
                SB();
                mma(afA, bfA);
                SB();
                if (!(xexp & 16) && wdma) issue_w(s + 1);
                read_frags(s, 2, afA, bfA);
                SB();
                mma(afB, bfB);
                SB();
                mma(afA, bfA);
            }
            const bool seam = sp == kV7Steps - 1 && s + 1 < send;
            if (seam) {
                __syncthreads();                        // every wave is done with this chunk's halo
                store_halo();
            }
            if (seam || !(xexp & 1)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // step s+1's weights (and the halo DMA) have landed
            if (seam || !(xexp & 2)) __syncthreads();
        }
    }
    if constexpr (TAIL) {                               // the raw partial unit [256][80]
        float* pp = g.part + (long)blockIdx.x * 256 * CO;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    pp[(wave * 64 + i * 16 + (lane >> 4) * 4 + r) * CO + j * 16 + (lane & 15)] = acc[i][j][r];
        return;
    }
    if (xexp & 32) {                                    // DIAG: no epilogue (one store per wave keeps the work live)
        if (acc[0][0][0] + acc[3][4][3] == 12345.0f) reinterpret_cast<float*>(a.out)[threadIdx.x] = 0.0f;
        return;
    }
    conv_epilogue_spec<EPI, 256, CO, 2>(a, acc, reinterpret_cast<float*>(smem_v7), wave, 0, nh * CO, lane, b, pt,
                                        tyy * 2, txx * 2, nT, nY, nX);
}

// Tail of the split launch: unit = the five chunk partials summed in a fixed order,
// then the epilogue per 8 channels of a voxel row (conv_v6_tail_reduce_kernel's)
__global__ void __launch_bounds__(256) conv_v7_tail_reduce_kernel(ConvV6Args g, int ntail) {
    const ConvV2Args& a = g.v;
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int nYt = (nY + 1) >> 1, nXt = (nX + 1) >> 1;
    const int nunit = 2 * a.B * nT * nYt * nXt;
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)ntail * 256 * 10) return;
    const int t = (int)(i / (256 * 10)), rem = (int)(i % (256 * 10));
    const int vl = rem / 10, cl = (rem % 10) * 8;
    int b, pt, tyy, txx, nh;
    v7_unit(g.tail_base + t, nunit, nT, nYt, nXt, b, pt, tyy, txx, nh);
    const int c = nh * kV7Co + cl;
    const int pwv = vl >> 6;
    const int py = tyy * 2 + (pwv >> 1), px = txx * 2 + (pwv & 1);
    if (py >= nY || px >= nX) return;
    const long orow = ((((long)b * nT + pt) * nY + py) * nX + px) * 64 + (vl & 63);
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < 5; ++w) {
        const float* p = g.part + ((long)(t * 5 + w) * 256 + vl) * kV7Co + cl;
        const f32x4_t p0 = *reinterpret_cast<const f32x4_t*>(p), p1 = *reinterpret_cast<const f32x4_t*>(p + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] += p0[e]; v[4 + e] += p1[e]; }
    }
    if (a.bias) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += a.bias[c + e];
    }
    if (a.mask) {
        const bf16x8_t m = *reinterpret_cast<const bf16x8_t*>(a.mask + orow * a.mask_ld + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = ((float)m[e] > 0.0f) ? v[e] : 0.0f;
    }
    if (a.res) {
        if (a.res_f32) {
            const float* rp = reinterpret_cast<const float*>(a.res) + orow * a.res_ld + c;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += a.res_scale * rp[e];
        } else {
            const bf16x8_t rr = *reinterpret_cast<const bf16x8_t*>(reinterpret_cast<const bf16*>(a.res) + orow * a.res_ld + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += a.res_scale * (float)rr[e];
        }
    }
    if (a.relu_out) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.0f);
    }
    const long oi = orow * a.cout_ld + c;
    if (a.out_f32) {
        float* o = reinterpret_cast<float*>(a.out) + oi;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = a.accumulate ? o[e] + v[e] : v[e];
    } else {
        bf16* o = reinterpret_cast<bf16*>(a.out) + oi;
        bf16x8_t ov;
        if (a.accumulate) {
            const bf16x8_t prev = *reinterpret_cast<const bf16x8_t*>(o);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += (float)prev[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) ov[e] = (bf16)v[e];
        *reinterpret_cast<bf16x8_t*>(o) = ov;
    }
}

// tail_ws: conv_tail_bytes(tiles) bytes, as v6 (twice the tail units of half the channels)
static int conv_v7_launch(const ConvV2Args& v, float* tail_ws, hipStream_t st) {
    if ((long)v.B * v.D * v.H * v.W * v.cin_ld >= (1L << 31)) return DLCS_ERR_UNSUPPORTED_SIZE;   // 32-bit halo offsets
    const unsigned nunit = 2u * (unsigned)conv_tiles(v.B, v.D, v.H, v.W);
    const char* te = dlcs_test_hook("DLCS_V7_TAIL");                 // read per launch (tests toggle it)
    const bool tail_split = !(te && te[0] == '0');
    // one round = 512 workgroups (two per CU): the units of v6's tail tiles
    const unsigned ntail = tail_split ? 2u * conv_tail_tiles(nunit / 2) : 0u, nmain = nunit - ntail;
    const bool split = ntail > 0;
    ConvV6Args g{v};
#ifdef DLCS_DIAG_BUILD
    if (const char* e = dlcs_knob("DLCS_V7_EXP")) g.exp = atoi(e);   // read per launch (timing experiments)
#endif
    if (split) g.part = tail_ws;                        // ntail units x 5 x 256 x 80 floats
    const int epi = conv_epi_code(v.res, v.mask, !v.accumulate && !v.out_f32, !v.res_f32);   // fused residual: bf16
    const dim3 gm(split ? nmain : nunit);
    if (epi == 0) hipLaunchKernelGGL((conv3d_k3_v7_kernel<0, false>), gm, dim3(256), 0, st, g);
    else if (epi == kEpiRes) hipLaunchKernelGGL((conv3d_k3_v7_kernel<kEpiRes, false>), gm, dim3(256), 0, st, g);
    else if (epi == kEpiMask) hipLaunchKernelGGL((conv3d_k3_v7_kernel<kEpiMask, false>), gm, dim3(256), 0, st, g);
    else hipLaunchKernelGGL((conv3d_k3_v7_kernel<kEpiGeneric, false>), gm, dim3(256), 0, st, g);
    if (split) {
        g.tail_base = (int)nmain;
        hipLaunchKernelGGL((conv3d_k3_v7_kernel<0, true>), dim3(ntail * 5), dim3(256), 0, st, g);
        hipLaunchKernelGGL(conv_v7_tail_reduce_kernel, dim3((unsigned)cdiv((long)ntail * 256 * 10, 256)), dim3(256), 0,
                           st, g, (int)ntail);
    }
    return dlcs_launch_status();
}
