// ---------------------------------------------------------------- bf16 Conv3d 160 -> 160, v6
// Included by conv3d.hip.  The bf16 160-channel forward /
// input gradient (s3d:336, :356; config 2's dtype) on the f16x3 kernel's
// structure, with one bf16 product per tap instead of three plane products:
//   * tile, waves, fragments and LDS images of conv3d_k3_v5_kernel: 256 voxels
//     (1 x 2 x 2 patches) x 160 output channels, 8 waves x 4 x 5 tiles of 16 x 16
//     (v_mfma_f32_16x16x32_bf16), K walked in 32-channel chunks; 64-B image rows
//     with the v5 XOR chunk swizzles (conflict-free ds_read_b128);
//   * a step is TWO tap rows (kd, kh) = six taps (the v5 kernel: one row, three
//     taps): 120 MFMAs per wave between barriers -- the f16x3 step's matrix work
//     (2 taps x 3 plane products) -- so the barrier, the end-of-step drain and the
//     weight DMA's issue cost are paid 25 times per tile instead of 45;
//   * LDS: ONE halo image [600][32] (38.4 KB) + two weight slots of six tap slices
//     [6][160][32] (2 x 60 KB) = 157.5 KB.  The next chunk's halo is staged as in
//     the f16x3 kernel: its first 128 rows (time slices 0-1, which no tap reads
//     after step 2 of a chunk: kd = 0, 1 are rows 0..5) are DMA'd straight into the
//     live image during step 3, the rest waits in registers and is stored behind an
//     extra barrier at the chunk seam;
//   * the next step's six weight slices (60 x 1 KB pieces, contiguous in the
//     packed [tap][co][ci] layout) DMA'd among the first tap's MFMAs;
//   * tiles numbered XCD-major (neighbouring halos in one L2) and the last partial
//     round of 256 CUs (3360 = 13 x 256 + 32 tiles at the BASELINE slice) split
//     into 5 single-chunk workgroups per tile + a fixed-order reduce with the same
//     epilogue (run-to-run deterministic), as conv_f16x3_launch.
// Weights: dlcs_conv3d_pack_weights bf16 modes 0 / 1 (the v5 packing, cin_pad 160).
constexpr int kV6Slot = 6 * 160 * 32;                   // bf16 per weight slot (6 taps x 160 co x 32 ci)
constexpr int kV6Steps = 5;                             // steps per chunk: rows {0,1} {2,3} {4,5} {6,7} {8}

// tile vb (XCD-major virtual numbering over nblk tiles) -> (b, pt, tyy, txx)
DLCS_DEV void v6_tile(int vb, int nblk, int nT, int nYt, int nXt, int& b, int& pt, int& tyy, int& txx) {
    const int q8 = nblk >> 3, r8 = nblk & 7, xcd = vb & 7;
    int bid = xcd * q8 + min(xcd, r8) + (vb >> 3);
    txx = bid % nXt; bid /= nXt;
    tyy = bid % nYt; bid /= nYt;
    pt = bid % nT;
    b = bid / nT;
}

template <int EPI, bool TAIL>
__global__ void __launch_bounds__(512) conv3d_k3_v6_kernel(ConvV6Args g) {
    const ConvV2Args& a = g.v;
    constexpr int LD = 32, CO = 160;
    constexpr int HSZ = kHalo * LD;                     // bf16 in the halo image
    __shared__ __attribute__((aligned(16))) bf16 smem_v6[HSZ + 2 * kV6Slot];   // 157.5 KB
    bf16* Hs = smem_v6;
    bf16* Ws = smem_v6 + HSZ;

    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int nYt = (nY + 1) >> 1, nXt = (nX + 1) >> 1;
    const int nblk = a.B * nT * nYt * nXt;
    const int cc0 = TAIL ? (int)blockIdx.x % 5 : 0;
    const int cc1 = TAIL ? cc0 + 1 : 5;
    int b, pt, tyy, txx;
    v6_tile(TAIL ? g.tail_base + (int)blockIdx.x / 5 : (int)blockIdx.x, nblk, nT, nYt, nXt, b, pt, tyy, txx);
    const int t0 = pt * 4, y0 = tyy * 8, x0 = txx * 8;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pw = wave & 3, nh = wave >> 2;

    // halo pieces: 600 rows x 4 16-B chunks = 2400, piece i = threadIdx + 512 k (k < 5).
    // k = 0 (rows < 128, time slices 0-1) is DMA'd into the live image during step 3;
    // k = 1..4 wait in registers until the chunk seam.
    constexpr int HP = 5, HR = HP - 1;
    bf16x8_t hr[HR];
    auto halo_off = [&](int k) {                        // element offset of piece k (channel chunk 0), -1 off the grid
        const int i = threadIdx.x + k * 512;
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
    auto dma_halo = [&](int cc) {                       // piece k = 0: LDS position i (swizzle on the load side)
        const int off = halo_off(0);
        glds16(off >= 0 ? (const void*)(a.in + cc * CK + off) : (const void*)g_wg_zero_row,
               hbase + (unsigned)(wave * 64 * 16));
    };
    auto load_halo = [&](int cc) {
#pragma unroll
        for (int k = 0; k < HR; ++k) {
            const int off = halo_off(1 + k);
            hr[k] = (bf16x8_t)(bf16)0.0f;
            if (off >= 0) hr[k] = *reinterpret_cast<const bf16x8_t*>(a.in + cc * CK + off);
        }
    };
    auto store_halo = [&]() {
#pragma unroll
        for (int k = 0; k < HR; ++k) {
            const int i = threadIdx.x + (1 + k) * 512;
            if (i < kHalo * 4) *reinterpret_cast<bf16x8_t*>(Hs + i * 8) = hr[k];
        }
    };
    // weight DMA of step s (chunk s / 5, rows 2 (s % 5), + 1) into slot s & 1: the
    // step's taps 6 (s % 5) .. are contiguous in the packed layout; piece wi (of 60, or
    // 30 for the one-row step) by wave wi % 8; LDS chunk c of piece wi: row (c >> 2) =
    // tap-in-slot * 160 + co, position c & 3 <- logical chunk (c & 3) ^ swz(co)
    const unsigned wbase = lds_offset(Ws);
    unsigned woff[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int wi = k * 8 + wave;
        const int c = wi * 64 + lane;
        const int row = c >> 2, pos = c & 3;
        const int tl = row / CO, co = row - tl * CO;
        const int kl = pos ^ ((4 - ((co & 15) >> 2)) & 3);
        woff[k] = (unsigned)(((tl * CO + co) * a.cin_pad + (kl << 3)) * 2);
    }
    auto issue_w = [&](int s) {
        const int cc = s / kV6Steps, sp = s % kV6Steps;
        const int npc = sp == 4 ? 30 : 60;
        const unsigned dst = wbase + (unsigned)((s & 1) * kV6Slot * 2);
        const bf16* src = a.w + (long)(6 * sp) * CO * a.cin_pad + cc * CK;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int wi = k * 8 + wave;
            if (wi < npc) glds16_s(src, woff[k], dst + wi * 1024);
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
    const int bpos = (cq ^ ((4 - (vq >> 2)) & 3)) << 3;

    // fragments of tap ti (0..5) of step s (rows 2 sp, 2 sp + 1)
    auto read_frags = [&](int s, int ti, bf16x8_t (&af)[4], bf16x8_t (&bfr)[5]) {
        const int tap = 6 * (s % kV6Steps) + ti;
        const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
        const int apos = (cq ^ (((ly + kh) & 1) << 1)) << 3;
        const int toff = (kd * kHaloY + kh) * kHaloX + kw;
        const bf16* wb = Ws + (s & 1) * kV6Slot;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            af[i] = *reinterpret_cast<const bf16x8_t*>(Hs + (hb0 + i * kHaloY * kHaloX + toff) * LD + apos);
#pragma unroll
        for (int j = 0; j < 5; ++j)
            bfr[j] = *reinterpret_cast<const bf16x8_t*>(wb + (ti * CO + corow + j * 16) * LD + bpos);
    };
    auto mma = [&](const bf16x8_t (&af)[4], const bf16x8_t (&bfr)[5]) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) mfma16(acc[i][j], af[i], bfr[j]);
    };

    const int send = cc1 * kV6Steps;                    // one past the last step of this workgroup
    dma_halo(cc0);
    load_halo(cc0);
    issue_w(cc0 * kV6Steps);
    store_halo();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    if (wave >= 4) __builtin_amdgcn_s_setprio(1);
    auto step = [&](int s, int cc, auto NTc) {
        constexpr int nt = decltype(NTc)::value;        // taps in this step: 6, or 3 (row 8)
        const int sp = s % kV6Steps;
        const bool seam = (nt == 3) && (s + 1 < send);
        if (sp == 3 && cc + 1 < cc1) {                  // time slices 0-1 are dead from step 3 on
            dma_halo(cc + 1);
            load_halo(cc + 1);
        }
        bf16x8_t afA[4], bfA[5], afB[4], bfB[5];
        // scheduling fences (SB): the next tap's fragment reads are issued before the
        // current tap's MFMAs and stay there -- left alone, the compiler sinks each
        // ds_read next to its first use and every MFMA group waits on LDS latency
#ifdef DLCS_DIAG_BUILD
        const bool sbar = !(g.exp & 128);
#else
        constexpr bool sbar = true;
#endif
        auto SB = [&]() { if (sbar) __builtin_amdgcn_sched_barrier(0); };
        read_frags(s, 0, afA, bfA);
#pragma unroll
        for (int ti = 0; ti < nt; ti += 2) {
            if (ti + 1 < nt) read_frags(s, ti + 1, afB, bfB);
            SB();
            mma(afA, bfA);
            SB();
            if (ti == 0 && s + 1 < send) issue_w(s + 1);
            if (ti + 2 < nt) read_frags(s, ti + 2, afA, bfA);
            SB();
            if (ti + 1 < nt) mma(afB, bfB);
            SB();
        }
        if (seam) {
            __syncthreads();                            // every wave is done with this chunk's halo
            store_halo();
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // step s+1's weights (and the halo DMA) have landed
        __syncthreads();
    };
    for (int cc = cc0; cc < cc1; ++cc) {
#pragma unroll 1
        for (int sp = 0; sp < 4; ++sp) step(cc * kV6Steps + sp, cc, std::integral_constant<int, 6>{});
        step(cc * kV6Steps + 4, cc, std::integral_constant<int, 3>{});
    }
    if constexpr (TAIL) {                               // the raw partial tile [256][160]
        float* pp = g.part + (long)blockIdx.x * 256 * 160;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    pp[(pw * 64 + i * 16 + (lane >> 4) * 4 + r) * 160 + nh * 80 + j * 16 + (lane & 15)] = acc[i][j][r];
        return;
    }
    conv_epilogue_spec<EPI, 512, 160, 2>(a, acc, reinterpret_cast<float*>(smem_v6), pw, nh * 80, 0, lane, b, pt,
                                         tyy * 2, txx * 2, nT, nY, nX);
}

// Tail of the split launch: tile = the five chunk partials summed in a fixed order,
// then conv_epilogue_spec's epilogue per 8 channels of a voxel row
__global__ void __launch_bounds__(256) conv_v6_tail_reduce_kernel(ConvV6Args g, int ntail) {
    const ConvV2Args& a = g.v;
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int nYt = (nY + 1) >> 1, nXt = (nX + 1) >> 1;
    const int nblk = a.B * nT * nYt * nXt;
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)ntail * 256 * 20) return;
    const int t = (int)(i / (256 * 20)), rem = (int)(i % (256 * 20));
    const int vl = rem / 20, c = (rem % 20) * 8;
    int b, pt, tyy, txx;
    v6_tile(g.tail_base + t, nblk, nT, nYt, nXt, b, pt, tyy, txx);
    const int pwv = vl >> 6;
    const int py = tyy * 2 + (pwv >> 1), px = txx * 2 + (pwv & 1);
    if (py >= nY || px >= nX) return;
    const long orow = ((((long)b * nT + pt) * nY + py) * nX + px) * 64 + (vl & 63);
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < 5; ++w) {
        const float* p = g.part + ((long)(t * 5 + w) * 256 + vl) * 160 + c;
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

// tail_ws: conv_tail_bytes(tiles) bytes for the tail split's partial tiles
static int conv_v6_launch(const ConvV2Args& v, float* tail_ws, hipStream_t st) {
    if ((long)v.B * v.D * v.H * v.W * v.cin_ld >= (1L << 31)) return DLCS_ERR_UNSUPPORTED_SIZE;   // 32-bit halo offsets
    const unsigned nblk = (unsigned)conv_tiles(v.B, v.D, v.H, v.W);
    const char* te = dlcs_test_hook("DLCS_V6_TAIL");                 // read per launch (tests toggle it)
    const bool tail_split = !(te && te[0] == '0');
    const unsigned ntail = tail_split ? conv_tail_tiles(nblk) : 0u, nmain = nblk - ntail;
    const bool split = ntail > 0;
    ConvV6Args g{v};
#ifdef DLCS_DIAG_BUILD
    if (const char* e = dlcs_knob("DLCS_V6_EXP")) g.exp = atoi(e);   // read per launch: 128 = no scheduling fences
#endif
    if (split) g.part = tail_ws;
    const int epi = conv_epi_code(v.res, v.mask, !v.accumulate && !v.out_f32, !v.res_f32);   // fused residual: bf16
    const dim3 gm(split ? nmain : nblk);
    if (epi == 0) hipLaunchKernelGGL((conv3d_k3_v6_kernel<0, false>), gm, dim3(512), 0, st, g);
    else if (epi == kEpiRes) hipLaunchKernelGGL((conv3d_k3_v6_kernel<kEpiRes, false>), gm, dim3(512), 0, st, g);
    else if (epi == kEpiMask) hipLaunchKernelGGL((conv3d_k3_v6_kernel<kEpiMask, false>), gm, dim3(512), 0, st, g);
    else hipLaunchKernelGGL((conv3d_k3_v6_kernel<kEpiGeneric, false>), gm, dim3(512), 0, st, g);
    if (split) {
        g.tail_base = (int)nmain;
        hipLaunchKernelGGL((conv3d_k3_v6_kernel<0, true>), dim3(ntail * 5), dim3(512), 0, st, g);
        hipLaunchKernelGGL(conv_v6_tail_reduce_kernel, dim3((unsigned)cdiv((long)ntail * 256 * 20, 256)), dim3(256), 0,
                           st, g, (int)ntail);
    }
    return dlcs_launch_status();
}
