// ---------------------------------------------------------------- fp32 thin-end convs on fp16 MFMAs
// The ConvBlocks' thin ends at fp32 accuracy on the fp16 matrix cores, with the
// 2-plane split of conv3d_f16x3.inc (one power-of-two scale per tensor,
// u = s x, xh = f16(u), xl = f16(u - xh); three plane products hh + hl + lh,
// each exact in the fp32 accumulator, rescaled by 1 / (s_x s_w)):
//   * thin input  (Cin <= 4 -> 160): the SFE conv (s3d:384) and the final
//     conv's dgrad (s3d:391);
//   * thin output (160 -> Cout <= 4): the final conv (s3d:391) and the SFE
//     conv's dgrad;
//   * weight gradient 160 <-> thin: both ends' dW (+ the SFE bias gradient).
// Unlike the 160 -> 160 kernels, no operand is pre-split in HBM: each kernel
// reads the fp32 activation once and splits it in registers on its way into
// LDS (the scale comes from a max |x| word written by the producing kernel's
// epilogue, or by dlcs_absmax_f32 for the 4-channel volumes), so the 160-channel
// side costs exactly its fp32 bytes -- these kernels are HBM / L2 bound (29.7
// GFLOP per launch at fp32 = 89 GFLOP of fp16 products, 36 us of matrix-core
// time at the dense peak, vs 550 MB = 69 us of HBM).
// Weights are packed per call by pack_thin_f16x3_kernel (one workgroup: max,
// scale, planes) from the fp32 packing of dlcs_conv3d_pack_weights.

DLCS_DEV void mfma32h(f32x16& acc, const f16x8_t& a, const f16x8_t& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
}

// persistent-grid tile walk, XCD-major: workgroup w runs on XCD w % 8 and walks
// that XCD's contiguous run of tiles, so neighbouring tiles (shared halo rows)
// are in flight on one L2 (gridDim.x a multiple of 8)
struct XcdWalk {
    int t, end, step;
    DLCS_DEV XcdWalk(int ntiles) {
        const int per = (ntiles + 7) >> 3, x = blockIdx.x & 7;
        t = x * per + (blockIdx.x >> 3);
        end = min(ntiles, (x + 1) * per);
        step = gridDim.x >> 3;
    }
};

// 16-B load through a pointer selected between the element and a zero row, so the
// load itself is unconditional: a load under a branch (or a select the compiler
// turns into one) gets its own vmcnt(0) wait, which serialised the halo staging
// of these kernels on memory latency (19 loads per thread and chunk in thin_out)
DLCS_DEV f32x4_t ldz4f(const float* p, bool ok) {
    return *reinterpret_cast<const f32x4_t*>(ok ? static_cast<const void*>(p) : static_cast<const void*>(g_wg_zero_row));
}

DLCS_DEV void split_f16(float x, float s, f16& h, f16& l) {
    const float u = x * s;
    h = (f16)u;
    l = (f16)(u - (float)h);
}

// Grid-wide version (dlcs_conv3d_thin_pack_f16x3): max |w| by absmax_flat_kernel into
// the word `mx` first, then the planes by a grid of workgroups (block 0 writes s) --
// the one-workgroup pack below walked ~35 K weights serially (~50 us, 40 per step).
__global__ void __launch_bounds__(256) pack_thin_f16x3_grid_kernel(const float* wp, int cout, int cout_pad, int cin,
                                                                   int cin_pad, int kind, const unsigned* mx, f16* out) {
    const float s = f16x3_scale(*mx);
    const int stride = gridDim.x * 256;
    if (kind == 0) {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < kThinInHalfs / 2; i += stride) {
            const int j = i & 7, co = (i >> 3) % 160, kg = (i / 1280) & 3, ks = i / 5120;
            const int tap = 8 * ks + 2 * kg + (j >> 2), ci = j & 3;
            const float v = (tap < 27 && ci < cin && co < cout) ? wp[((long)tap * cout_pad + co) * cin_pad + ci] : 0.0f;
            f16 h, l;
            split_f16(v, s, h, l);
            out[i] = h;
            out[kThinInHalfs / 2 + i] = l;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<float*>(out + kThinInHalfs) = s;
    } else {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < kThinOutHalfs / 2; i += stride) {
            const int j = i & 7, n = (i >> 3) & 15, kg = (i >> 7) & 3, kk = (i >> 9) % 9, cc = (i >> 9) / 9;
            const int kw = n >> 2, co = n & 3, tap = 3 * kk + kw, ci = 32 * cc + 8 * kg + j;
            const float v = (kw < 3 && co < cout && ci < cin) ? wp[((long)tap * cout_pad + co) * cin_pad + ci] : 0.0f;
            f16 h, l;
            split_f16(v, s, h, l);
            const int base = (cc * 9 + kk) * 1024 + (kg * 16 + n) * 8 + j;
            out[base] = h;
            out[base + 512] = l;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<float*>(out + kThinOutHalfs) = s;
    }
}

// wp: fp32 [27][cout_pad][cin_pad] (dlcs_conv3d_pack_weights, mode 0 or 1).
// kind 0 (thin input, Cout = 160): element j of (ks, kg, co) = W[tap = 8 ks + 2 kg + (j >> 2)][co][ci = j & 3]
// kind 1 (thin output, Cin = 160): element j of (cc, kk, kg, n) = W[tap = 3 kk + (n >> 2)][co = n & 3][ci = 32 cc + 8 kg + j]
// Out-of-range taps / channels are 0.
__global__ void __launch_bounds__(1024) pack_thin_f16x3_kernel(const float* wp, int cout, int cout_pad, int cin,
                                                               int cin_pad, int kind, f16* out) {
    __shared__ float red[16];
    __shared__ float s_sh;
    float m = 0.0f;
    const int total = 27 * cout_pad * cin_pad;
    for (int i = threadIdx.x; i < total; i += 1024) {
        const int ci = i % cin_pad, co = (i / cin_pad) % cout_pad;
        if (ci < cin && co < cout) m = fmaxf(m, fabsf(wp[i]));
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float mm = red[0];
        for (int i = 1; i < 16; ++i) mm = fmaxf(mm, red[i]);
        s_sh = f16x3_scale(__float_as_uint(mm));
    }
    __syncthreads();
    const float s = s_sh;
    if (kind == 0) {
        for (int i = threadIdx.x; i < kThinInHalfs / 2; i += 1024) {
            const int j = i & 7, co = (i >> 3) % 160, kg = (i / 1280) & 3, ks = i / 5120;
            const int tap = 8 * ks + 2 * kg + (j >> 2), ci = j & 3;
            const float v = (tap < 27 && ci < cin && co < cout) ? wp[((long)tap * cout_pad + co) * cin_pad + ci] : 0.0f;
            f16 h, l;
            split_f16(v, s, h, l);
            out[i] = h;
            out[kThinInHalfs / 2 + i] = l;
        }
        if (threadIdx.x == 0) *reinterpret_cast<float*>(out + kThinInHalfs) = s;
    } else {
        for (int i = threadIdx.x; i < kThinOutHalfs / 2; i += 1024) {
            const int j = i & 7, n = (i >> 3) & 15, kg = (i >> 7) & 3, kk = (i >> 9) % 9, cc = (i >> 9) / 9;
            const int kw = n >> 2, co = n & 3, tap = 3 * kk + kw, ci = 32 * cc + 8 * kg + j;
            const float v = (kw < 3 && co < cout && ci < cin) ? wp[((long)tap * cout_pad + co) * cin_pad + ci] : 0.0f;
            f16 h, l;
            split_f16(v, s, h, l);
            const int base = (cc * 9 + kk) * 1024 + (kg * 16 + n) * 8 + j;
            out[base] = h;
            out[base + 512] = l;
        }
        if (threadIdx.x == 0) *reinterpret_cast<float*>(out + kThinOutHalfs) = s;
    }
}

// ---------------------------------------------------------------- thin input (Cin <= 4 -> 160)
// Tile, waves and epilogue of conv3d_thin_in_f32_kernel (256 voxels x 160
// channels, 8 waves = voxel quarter pw x channel half nh, 4 x 5 tiles of 16 x 16,
// persistent workgroups).  K = 27 taps x 4 channels = 108 (4 k-steps of 32 with
// the MFMA v_mfma_f32_16x16x32_f16): lane (voxel m, k group kg) of k-step ks
// holds taps 8 ks + 2 kg and + 1, 4 channels each -- two 16-B halo rows of the
// [600][hi 4 | lo 4] f16 image, whose 8-B halves are the hi and lo fragments.
// The weights [plane][ks][kg][co][8] (80 KB) stay in LDS.
// Each wave's 16 output voxels of a tile take pseudo-random signs through the sum
// (A rows XOR-negated, restored in the epilogue) so the matrix core's truncation
// bias cancels in later voxel sums (conv3d_f16x3.inc, accumulation mode 3): this
// kernel is the final conv's input gradient, whose bias every later gradient
// inherited (tools/grad_trained_diag.py: median 6e-6 -> 1.2e-6 NRMSE of float64).
// The masked form (the final conv's input gradient) takes conv3d_f16x3.inc's fused
// epilogue (mask prefetched into registers), which can also write the output's
// planes (op: the scale from the bound in their trailer) instead of / beside the
// fp32 output and the per-tile column sums (cpart: the DFE bias gradient).
template <int EPI>
__global__ void __launch_bounds__(512) conv3d_thin_in_f16x3_kernel(ConvF32Args a, const f16* wimg, const unsigned* xmax,
                                                                   int cin, int ntiles, f16* op, const unsigned* opmax,
                                                                   float* cpart) {
    __shared__ __attribute__((aligned(16))) f16 smem_ti3[kThinInHalfs + kHalo * 8 + 256 * 36 * 2 + 512 * 2];
    f16* Wt = smem_ti3;
    f16* Hs = smem_ti3 + kThinInHalfs;
    float* Es = reinterpret_cast<float*>(Hs + kHalo * 8);
    for (int i = threadIdx.x; i < kThinInHalfs / 8; i += 512)
        reinterpret_cast<uint4*>(Wt)[i] = reinterpret_cast<const uint4*>(wimg)[i];
    const float sx = f16x3_scale(*xmax);
    const float inv = 1.0f / (sx * *reinterpret_cast<const float*>(wimg + kThinInHalfs));
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int nYt = (nY + 1) >> 1, nXt = (nX + 1) >> 1;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pw = wave & 3, nh = wave >> 2;
    const int m = lane & 15, kg = lane >> 4;
    const int ly = (pw >> 1) * 4 + ((m >> 2) & 3), lx = (pw & 1) * 4 + (m & 3);
    int aoff[4][2];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int tap = min(8 * ks + 2 * kg + e, 26);     // taps >= 27 meet zero weights
            aoff[ks][e] = (((tap / 9) * kHaloY + ly + (tap / 3) % 3) * kHaloX + lx + tap % 3) * 8;
        }
    const int boff = (kg * 160 + nh * 80 + m) * 8;
    auto decode = [&](int tile, int& b, int& pt, int& tyy, int& txx) {
        int bid = tile;
        txx = bid % nXt; bid /= nXt;
        tyy = bid % nYt; bid /= nYt;
        pt = bid % nT;
        b = bid / nT;
    };
    constexpr int HPER = (kHalo + 511) / 512;           // 2
    f32x4_t hreg[HPER];
    auto load_halo = [&](int tile) {
        int b, pt, tyy, txx;
        decode(tile, b, pt, tyy, txx);
#pragma unroll
        for (int kk = 0; kk < HPER; ++kk) {
            const int hv = threadIdx.x + 512 * kk;
            const int ht = hv / (kHaloY * kHaloX), hy = (hv / kHaloX) % kHaloY, hx = hv % kHaloX;
            const int t = pt * 4 - 1 + ht, y = tyy * 8 - 1 + hy, x = txx * 8 - 1 + hx;
            const bool ok = hv < kHalo && t >= 0 && t < a.D && y >= 0 && y < a.H && x >= 0 && x < a.W;
            hreg[kk] = ldz4f(a.in + brow(b, t, y, x, nT, nY, nX) * a.cin_ld, ok);
        }
    };
    const XcdWalk wk(ntiles);
    int tile = wk.t;
    if (tile < wk.end) load_halo(tile);
    for (; tile < wk.end; tile += wk.step) {
        int b, pt, tyy, txx;
        decode(tile, b, pt, tyy, txx);
#pragma unroll
        for (int kk = 0; kk < HPER; ++kk) {
            const int hv = threadIdx.x + 512 * kk;
            if (hv < kHalo) {
                f16x8_t hl;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    f16 h, l;
                    split_f16(e < cin ? hreg[kk][e] : 0.0f, sx, h, l);
                    hl[e] = h;
                    hl[4 + e] = l;
                }
                *reinterpret_cast<f16x8_t*>(Hs + hv * 8) = hl;
            }
        }
        __syncthreads();
        if (tile + wk.step < wk.end) load_halo(tile + wk.step);
        f32x4_t acc[4][5];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) acc[i][j] = (f32x4_t)0.0f;
        const unsigned rsgn = ((unsigned)(tile * 8 + wave) * 0x9E3779B1u) >> 16;
        const unsigned rowm = ((rsgn >> m) & 1) ? 0x80008000u : 0u;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            f16x8_t ah[4], al[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f16x8_t ra = *reinterpret_cast<const f16x8_t*>(Hs + aoff[ks][0] + i * kHaloY * kHaloX * 8);
                const f16x8_t rb = *reinterpret_cast<const f16x8_t*>(Hs + aoff[ks][1] + i * kHaloY * kHaloX * 8);
                ah[i] = __builtin_shufflevector(ra, rb, 0, 1, 2, 3, 8, 9, 10, 11);
                al[i] = __builtin_shufflevector(ra, rb, 4, 5, 6, 7, 12, 13, 14, 15);
                ah[i] = __builtin_bit_cast(f16x8_t, __builtin_bit_cast(u32x4_h3, ah[i]) ^ rowm);
                al[i] = __builtin_bit_cast(f16x8_t, __builtin_bit_cast(u32x4_h3, al[i]) ^ rowm);
            }
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const f16* wb = Wt + ks * 4 * 160 * 8 + boff + j * 16 * 8;
                const f16x8_t bh = *reinterpret_cast<const f16x8_t*>(wb);
                const f16x8_t bl = *reinterpret_cast<const f16x8_t*>(wb + kThinInHalfs / 2);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    mfma16h(acc[i][j], al[i], bh);
                    mfma16h(acc[i][j], ah[i], bl);
                    mfma16h(acc[i][j], ah[i], bh);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] *= ((rsgn >> (4 * (lane >> 4) + r)) & 1) ? -inv : inv;
        if constexpr (EPI == kEpiMask)
            conv_epilogue_h3<kEpiMask, 5, false>(a, acc, Es, pw, nh * 80, lane, b, pt, tyy * 2, txx * 2, nT, nY, nX, op, opmax,
                                          cpart ? cpart + (long)tile * 160 : nullptr);
        else
            conv_epilogue_f32<EPI, 5>(a, acc, Es, pw, nh * 80, lane, b, pt, tyy * 2, txx * 2, nT, nY, nX);
    }
}

// ---------------------------------------------------------------- thin output (160 -> Cout <= 4)
// The output-shift formulation of conv3d_thin_out_f32_kernel: Q[(t, y, x')][(kw,
// co)] = sum_{kd, kh, ci} W[kd, kh, kw][co][ci] x[t + kd - 1, y + kh - 1, x' - 1][ci]
// over the tile's 4 t x 8 y x 10 x' rows (N = 12 of 16 used), then out[t, y,
// x][co] = sum_kw Q[(t, y, x + kw)][(kw, co)].  K walked per 32-channel chunk:
// the chunk's halo [600][hi 32 | lo 32] f16 (76.8 KB, fp32 loads of the next
// chunk held in registers and split on the way into LDS) and the chunk's
// weights [kk][plane][kg][n][8] (18 KB).  Halo rows are 128 B of eight 16-B
// chunks XOR-swizzled by 2 ((R >> 1) & 3): within each ds_read_b128 lane group
// the 16 rows are consecutive, and (R & 1, chunk') is then distinct for both
// k groups the group mixes -- conflict-free.  4 waves x 5 M tiles (20 x 16 rows).
// GW: the chunk's weight fragments are read from global memory (L2-resident,
// 18 KB per chunk) instead of an LDS copy, so the workgroup needs only the 76.8 KB
// halo and two share a CU (8 waves instead of 4 to hide the halo loads)
template <bool GW>
__global__ void __launch_bounds__(256, GW ? 2 : 1) conv3d_thin_out_f16x3_kernel(ConvF32Args a, const f16* wimg,
                                                                                const unsigned* xmax, int ntiles) {
    constexpr int WCH = 9 * 2 * 4 * 16 * 8;              // f16 per weight chunk
    __shared__ __attribute__((aligned(16))) f16 smem_to3[kHalo * 64 + (GW ? 8 : WCH)];
    f16* Hs = smem_to3;
    f16* Wk = smem_to3 + kHalo * 64;
    float* Q = reinterpret_cast<float*>(smem_to3);        // [320][17] after the K loop (aliases the halo)
    const float sx = f16x3_scale(*xmax);
    const float inv = 1.0f / (sx * *reinterpret_cast<const float*>(wimg + kThinOutHalfs));
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int nYt = (nY + 1) >> 1, nXt = (nX + 1) >> 1;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, kg = lane >> 4;
    int hb[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int r = 16 * (5 * wave + i) + m;
        const int xp = r % 10, y = (r / 10) % 8, t = r / 80;
        hb[i] = (t * kHaloY + y) * kHaloX + xp;
    }
    constexpr int NQ = kHalo * 8;                        // 16-B fp32 quads per chunk
    constexpr int HPER = (NQ + 255) / 256;               // 19
    f32x4_t hr[HPER];
    auto load_halo = [&](int b, int pt, int tyy, int txx, int cc) {
#pragma unroll
        for (int k = 0; k < HPER; ++k) {
            const int i = threadIdx.x + k * 256;
            const int hv = i >> 3, q = i & 7;
            const int ht = hv / (kHaloY * kHaloX), hy = (hv / kHaloX) % kHaloY, hx = hv % kHaloX;
            const int t = pt * 4 - 1 + ht, y = tyy * 8 - 1 + hy, x = txx * 8 - 1 + hx;
            const bool ok = i < NQ && t >= 0 && t < a.D && y >= 0 && y < a.H && x >= 0 && x < a.W;
            hr[k] = ldz4f(a.in + brow(b, ok ? t : 0, ok ? y : 0, ok ? x : 0, nT, nY, nX) * a.cin_ld + cc * 32 + q * 4, ok);
        }
    };
    auto store_halo = [&]() {
#pragma unroll
        for (int k = 0; k < HPER; ++k) {
            const int i = threadIdx.x + k * 256;
            if (i < NQ) {
                const int hv = i >> 3, q = i & 7;
                const int swz = ((hv >> 1) & 3) << 1;
                f16x4_t h, l;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    f16 hh, ll;
                    split_f16(hr[k][e], sx, hh, ll);
                    h[e] = hh;
                    l[e] = ll;
                }
                f16* row = Hs + hv * 64 + (q & 1) * 4;
                *reinterpret_cast<f16x4_t*>(row + (((q >> 1) ^ swz) << 3)) = h;
                *reinterpret_cast<f16x4_t*>(row + (((4 + (q >> 1)) ^ swz) << 3)) = l;
            }
        }
    };
    auto store_w = [&](int cc) {
        const uint4* src = reinterpret_cast<const uint4*>(wimg + cc * WCH);
        for (int it = threadIdx.x; it < WCH / 8; it += 256) reinterpret_cast<uint4*>(Wk)[it] = src[it];
    };
    const XcdWalk wk(ntiles);
    for (int tile = wk.t; tile < wk.end; tile += wk.step) {
        int bid = tile;
        const int txx = bid % nXt; bid /= nXt;
        const int tyy = bid % nYt; bid /= nYt;
        const int pt = bid % nT;
        const int b = bid / nT;
        f32x4_t acc[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) acc[i] = (f32x4_t)0.0f;
        load_halo(b, pt, tyy, txx, 0);
        for (int cc = 0; cc < 5; ++cc) {
            __syncthreads();                             // previous chunk's / tile's readers are done
            store_halo();
            if (!GW) store_w(cc);
            __syncthreads();
            if (cc + 1 < 5) load_halo(b, pt, tyy, txx, cc + 1);
#pragma unroll 3
            for (int kk = 0; kk < 9; ++kk) {
                const int kd = kk / 3, kh = kk % 3;
                const f16* wb = (GW ? wimg + cc * WCH : Wk) + kk * 1024 + (kg * 16 + m) * 8;
                const f16x8_t bh = *reinterpret_cast<const f16x8_t*>(wb);
                const f16x8_t bl = *reinterpret_cast<const f16x8_t*>(wb + 512);
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const int R = hb[i] + kd * kHaloY * kHaloX + kh * kHaloX;
                    const int swz = ((R >> 1) & 3) << 1;
                    const f16x8_t ah = *reinterpret_cast<const f16x8_t*>(Hs + R * 64 + ((kg ^ swz) << 3));
                    const f16x8_t al = *reinterpret_cast<const f16x8_t*>(Hs + R * 64 + (((4 + kg) ^ swz) << 3));
                    f32x4_t t = (f32x4_t)0.0f;            // fresh tile, VALU-added (FOLD, conv3d_f16x3.inc)
                    mfma16h(t, al, bh);
                    mfma16h(t, ah, bl);
                    mfma16h(t, ah, bh);
                    acc[i] += t;
                }
            }
        }
        __syncthreads();
        // Q rows -> LDS [320][17]; C/D row = 4 kg + r, col n = m
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) Q[(16 * (5 * wave + i) + 4 * kg + r) * 17 + m] = acc[i][r] * inv;
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

#ifdef DLCS_DIAG_BUILD
// v2 of the thin-output kernel (DLCS_THIN_OUT_V2=1): the whole packed weight image (5 chunks x 9
// (kd, kh) x 2 planes x 4 k groups x the 12 used (kw, co) columns, 69 KB) is
// copied into LDS once per persistent workgroup, next to the chunk halo (76.8 KB),
// so the K loop has no weight traffic; the (tile, chunk) items a workgroup walks
// form one stream whose fp32 halo loads run two items ahead in two register
// sets (the next tile's first chunk is in flight during the last chunk's MFMAs
// and the epilogue).  Lanes of the unused columns 12..15 read column 11 (their
// Q columns are never read).
__global__ void __launch_bounds__(256, 1) conv3d_thin_out_f16x3_v2_kernel(ConvF32Args a, const f16* wimg,
                                                                          const unsigned* xmax, int ntiles) {
    __shared__ __attribute__((aligned(16))) f16 smem_to4[kHalo * 64 + kThinOutW2];
    f16* Hs = smem_to4;
    f16* Wl = smem_to4 + kHalo * 64;
    float* Q = reinterpret_cast<float*>(smem_to4);       // [320][17] after a tile's K loop (aliases the halo)
    // weights: global [cc][kk][plane][kg][n 16][8] -> LDS [cc][kk][plane][kg][n 12][8]
    for (int i = threadIdx.x; i < kThinOutW2 / 8; i += 256) {
        const int n = i % 12, rest = i / 12;             // rest = ((cc * 9 + kk) * 2 + plane) * 4 + kg
        const int kg = rest & 3, pl = (rest >> 2) & 1, ck = rest >> 3;
        reinterpret_cast<uint4*>(Wl)[i] =
            reinterpret_cast<const uint4*>(wimg)[(ck * 1024 + pl * 512 + (kg * 16 + n) * 8) / 8];
    }
    const float sx = f16x3_scale(*xmax);
    const float inv = 1.0f / (sx * *reinterpret_cast<const float*>(wimg + kThinOutHalfs));
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int nYt = (nY + 1) >> 1, nXt = (nX + 1) >> 1;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, kg = lane >> 4;
    const int wn = m < 12 ? m : 11;
    int hb[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int r = 16 * (5 * wave + i) + m;
        const int xp = r % 10, y = (r / 10) % 8, t = r / 80;
        hb[i] = (t * kHaloY + y) * kHaloX + xp;
    }
    constexpr int NQ = kHalo * 8;                        // 16-B fp32 quads per chunk
    constexpr int HPER = (NQ + 255) / 256;               // 19
    const XcdWalk wk(ntiles);
    const int mytiles = wk.t < wk.end ? (wk.end - wk.t + wk.step - 1) / wk.step : 0;
    const int nitems = mytiles * 5;
    auto decode = [&](int s, int& b, int& pt, int& tyy, int& txx) {
        int bid = wk.t + (s / 5) * wk.step;
        txx = bid % nXt; bid /= nXt;
        tyy = bid % nYt; bid /= nYt;
        pt = bid % nT;
        b = bid / nT;
    };
    auto issue = [&](f32x4_t (&hr)[HPER], int s) {
        if (s >= nitems) return;
        int b, pt, tyy, txx;
        decode(s, b, pt, tyy, txx);
        const int cc = s % 5;
#pragma unroll
        for (int k = 0; k < HPER; ++k) {
            const int i = threadIdx.x + k * 256;
            const int hv = i >> 3, q = i & 7;
            const int ht = hv / (kHaloY * kHaloX), hy = (hv / kHaloX) % kHaloY, hx = hv % kHaloX;
            const int t = pt * 4 - 1 + ht, y = tyy * 8 - 1 + hy, x = txx * 8 - 1 + hx;
            const bool ok = i < NQ && t >= 0 && t < a.D && y >= 0 && y < a.H && x >= 0 && x < a.W;
            hr[k] = ldz4f(a.in + brow(b, ok ? t : 0, ok ? y : 0, ok ? x : 0, nT, nY, nX) * a.cin_ld + cc * 32 + q * 4, ok);
        }
    };
    f32x4_t acc[5];
    auto body = [&](f32x4_t (&hr)[HPER], int s) {
        const int cc = s % 5;
        if (cc == 0) {
#pragma unroll
            for (int i = 0; i < 5; ++i) acc[i] = (f32x4_t)0.0f;
        }
        __syncthreads();                                 // previous chunk's readers / epilogue are done
#pragma unroll
        for (int k = 0; k < HPER; ++k) {
            const int i = threadIdx.x + k * 256;
            if (i < NQ) {
                const int hv = i >> 3, q = i & 7;
                const int swz = ((hv >> 1) & 3) << 1;
                f16x4_t h, l;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    f16 hh, ll;
                    split_f16(hr[k][e], sx, hh, ll);
                    h[e] = hh;
                    l[e] = ll;
                }
                f16* row = Hs + hv * 64 + (q & 1) * 4;
                *reinterpret_cast<f16x4_t*>(row + (((q >> 1) ^ swz) << 3)) = h;
                *reinterpret_cast<f16x4_t*>(row + (((4 + (q >> 1)) ^ swz) << 3)) = l;
            }
        }
        __syncthreads();
        issue(hr, s + 2);
        const f16* wc = Wl + cc * 9 * 768 + (kg * 12 + wn) * 8;
#pragma unroll 3
        for (int kk = 0; kk < 9; ++kk) {
            const int kd = kk / 3, kh = kk % 3;
            const f16* wb = wc + kk * 768;
            const f16x8_t bh = *reinterpret_cast<const f16x8_t*>(wb);
            const f16x8_t bl = *reinterpret_cast<const f16x8_t*>(wb + 384);
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int R = hb[i] + kd * kHaloY * kHaloX + kh * kHaloX;
                const int swz = ((R >> 1) & 3) << 1;
                const f16x8_t ah = *reinterpret_cast<const f16x8_t*>(Hs + R * 64 + ((kg ^ swz) << 3));
                const f16x8_t al = *reinterpret_cast<const f16x8_t*>(Hs + R * 64 + (((4 + kg) ^ swz) << 3));
                f32x4_t t = (f32x4_t)0.0f;                // fresh tile, VALU-added (FOLD, conv3d_f16x3.inc)
                mfma16h(t, al, bh);
                mfma16h(t, ah, bl);
                mfma16h(t, ah, bh);
                acc[i] += t;
            }
        }
        if (cc < 4) return;
        int b, pt, tyy, txx;
        decode(s, b, pt, tyy, txx);
        __syncthreads();
        // Q rows -> LDS [320][17]; C/D row = 4 kg + r, col n = m
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) Q[(16 * (5 * wave + i) + 4 * kg + r) * 17 + m] = acc[i][r] * inv;
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
    };
    f32x4_t hra[HPER], hrb[HPER];
    issue(hra, 0);
    issue(hrb, 1);
    for (int s = 0; s < nitems; s += 2) {
        body(hra, s);
        if (s + 1 < nitems) body(hrb, s + 1);
    }
}
#endif  // DLCS_DIAG_BUILD

// ---------------------------------------------------------------- wgrad, 160 <-> thin
// dW = Big^T . Thin_im2col with the tap shift on the thin side (u = v + off):
//   SFE   (Cin <= 4):  dW[tap][co][ci] = sum_u g[u][co] x[u + off(tap)][ci]   (Big = g, sgn +1)
//   final (Cout <= 4): dW[tap][co][ci] = sum_u x[u][ci] g[u - off(tap)][co]   (Big = x, sgn -1)
// M = 160 Big channels (5 tiles of 32), N = (tap, s) = 4 tap + s (108 of 128: 4
// tiles), K = the 64 voxels of a patch (4 k-steps of v_mfma_f32_32x32x16_f16).
// Per patch, both operands are built K-contiguous in LDS as [plane][row][64
// voxels] f16 (128-B rows, 16-B chunk c at c ^ ((row >> 1) & 7): the 16 rows of
// each ds_read_b128 lane group cover all 16 row residues -- conflict-free), in
// two buffers: while the 8 waves multiply patch p out of one, they split and
// transpose patch p + 1 from registers into the other and issue the loads of
// patch p + 2 (one barrier per patch).  Big: threads 0..319 each hold 8 voxels
// x 4 channels; thin im2col: threads 296..511 each hold one (tap, 8-voxel)
// column chunk, loaded straight from global (16-B rows, L2-resident).  Wave w:
// N tile w & 3, k-steps 2 (w >> 2) .. + 1, all 5 M tiles (80 accumulators);
// the two k halves meet in LDS before one atomicAdd per dW element.  One
// workgroup per CU (144 KB of LDS).  colsum (optional, Big = g): += sum_u
// g[u][co], the SFE bias gradient, from the fp32 registers of the same read.
struct ThinWgH3Args {
    const float* big; const float* thin; float* dw; float* colsum;
    const unsigned* big_max; const unsigned* thin_max;
    int big_ld, thin_ld, sgn, big_is_co, thin_ch, cout_pad, cin_pad;
    int B, D, H, W;
};
constexpr int kTwgBig = 2 * 160 * 64, kTwgThin = 2 * 128 * 64, kTwgBuf = kTwgBig + kTwgThin;   // f16

__global__ void __launch_bounds__(512, 1) conv3d_wgrad_thin_f16x3_kernel(ThinWgH3Args a, int nrange, int ppr) {
    __shared__ __attribute__((aligned(16))) f16 smem_tw[2 * kTwgBuf];    // 144 KB
    const int range = blockIdx.x;
    if (range >= nrange) return;
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int npatch = a.B * nT * nY * nX;
    const int p0 = range * ppr, p1 = min(npatch, p0 + ppr);
    if (p0 >= p1) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float sb = f16x3_scale(*a.big_max), st = f16x3_scale(*a.thin_max);
    const float inv = 1.0f / (sb * st);
    // thin rows n >= 108 stay zero (both buffers, both planes)
    for (int i = tid; i < 2 * 2 * 20 * 8; i += 512) {
        const int bf = i / 320, pl = (i / 160) & 1, rr = 108 + (i % 160) / 8, c = i % 8;
        *reinterpret_cast<uint4*>(smem_tw + bf * kTwgBuf + kTwgBig + pl * 8192 + rr * 64 + c * 8) = make_uint4(0, 0, 0, 0);
    }
    const bool big_task = tid < 320, thin_task = tid >= 296;
    const int vg = tid / 40, cq = tid % 40;                       // big: voxels 8 vg .., channels 4 cq ..
    const int tt = tid - 296, ttap = tt >> 3, tc = tt & 7;        // thin: tap, voxel chunk (t = tc >> 1, y pair tc & 1)
    const int tkd = a.sgn * (ttap / 9 - 1), tkh = a.sgn * ((ttap / 3) % 3 - 1), tkw = a.sgn * (ttap % 3 - 1);
    f32x4_t breg[8], treg[8];
    f32x4_t csum = (f32x4_t)0.0f;
    auto load = [&](int patch) {
        if (big_task) {
            const float* src = a.big + ((long)patch * 64 + 8 * vg) * a.big_ld + 4 * cq;
#pragma unroll
            for (int j = 0; j < 8; ++j) breg[j] = *reinterpret_cast<const f32x4_t*>(src + (long)j * a.big_ld);
        }
        if (thin_task) {
            const int px = patch % nX;
            int r = patch / nX;
            const int py = r % nY; r /= nY;
            const int pt = r % nT;
            const int bb = r / nT;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int T = pt * 4 + (tc >> 1) + tkd, Y = py * 4 + 2 * (tc & 1) + (j >> 2) + tkh,
                          X = px * 4 + (j & 3) + tkw;
                const bool ok = (unsigned)T < (unsigned)a.D && (unsigned)Y < (unsigned)a.H && (unsigned)X < (unsigned)a.W;
                treg[j] = ldz4f(a.thin + brow(bb, T, Y, X, nT, nY, nX) * a.thin_ld, ok);
            }
        }
    };
    auto store = [&](int buf) {
        f16* BigT = smem_tw + buf * kTwgBuf;
        f16* ThinC = BigT + kTwgBig;
        if (big_task) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int bch = 4 * cq + e;
                f16x8_t hv, lv;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    f16 h, l;
                    split_f16(breg[j][e], sb, h, l);
                    hv[j] = h;
                    lv[j] = l;
                }
                const int c = vg ^ ((bch >> 1) & 7);
                *reinterpret_cast<f16x8_t*>(BigT + bch * 64 + c * 8) = hv;
                *reinterpret_cast<f16x8_t*>(BigT + 10240 + bch * 64 + c * 8) = lv;
            }
            if (a.colsum) {
#pragma unroll
                for (int j = 0; j < 8; ++j) csum += breg[j];
            }
        }
        if (thin_task) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                f16x8_t hv, lv;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    f16 h, l;
                    split_f16(s < a.thin_ch ? treg[j][s] : 0.0f, st, h, l);
                    hv[j] = h;
                    lv[j] = l;
                }
                const int n = 4 * ttap + s;
                const int c = tc ^ ((n >> 1) & 7);
                *reinterpret_cast<f16x8_t*>(ThinC + n * 64 + c * 8) = hv;
                *reinterpret_cast<f16x8_t*>(ThinC + 8192 + n * 64 + c * 8) = lv;
            }
        }
    };

    f32x16 acc[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[i] = (f32x16)0.0f;
    const int r = lane & 31, h = lane >> 5;
    const int nt = wave & 3, kh2 = wave >> 2;
    const int nrow = 32 * nt + r;
    load(p0);
    store(0);
    if (p0 + 1 < p1) load(p0 + 1);
    __syncthreads();
    for (int patch = p0; patch < p1; ++patch) {
        const int cur = (patch - p0) & 1;
        const f16* BigT = smem_tw + cur * kTwgBuf;
        const f16* ThinC = BigT + kTwgBig;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int c = 2 * (2 * kh2 + kk) + h;
            const f16* bp = ThinC + nrow * 64 + ((c ^ ((nrow >> 1) & 7)) << 3);
            const f16x8_t bh = *reinterpret_cast<const f16x8_t*>(bp);
            const f16x8_t bl = *reinterpret_cast<const f16x8_t*>(bp + 8192);
#pragma unroll
            for (int mt = 0; mt < 5; ++mt) {
                const int brw = 32 * mt + r;
                const f16* ap = BigT + brw * 64 + ((c ^ ((brw >> 1) & 7)) << 3);
                const f16x8_t ah = *reinterpret_cast<const f16x8_t*>(ap);
                const f16x8_t al = *reinterpret_cast<const f16x8_t*>(ap + 10240);
                mfma32h(acc[mt], al, bh);
                mfma32h(acc[mt], ah, bl);
                mfma32h(acc[mt], ah, bh);
            }
        }
        if (patch + 1 < p1) {
            store(cur ^ 1);
            if (patch + 2 < p1) load(patch + 2);
        }
        __syncthreads();
    }
    // the k half 1 waves hand their accumulators to the k half 0 waves through LDS
    float* X = reinterpret_cast<float*>(smem_tw);                 // [4 nt][5 mt][16 q][64 lanes]
    if (kh2 == 1) {
#pragma unroll
        for (int mt = 0; mt < 5; ++mt)
#pragma unroll
            for (int q = 0; q < 16; ++q) X[((nt * 5 + mt) * 16 + q) * 64 + lane] = acc[mt][q];
    }
    __syncthreads();
    if (kh2 == 0) {
        // C[b][n]: b = 32 mt + (q & 3) + 8 (q >> 2) + 4 h, n = 32 nt + r
        const int n = 32 * nt + r, tap = n >> 2, sc = n & 3;
        if (tap < 27 && sc < a.thin_ch) {
#pragma unroll
            for (int mt = 0; mt < 5; ++mt)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int bch = 32 * mt + (q & 3) + 8 * (q >> 2) + 4 * h;
                    const int co = a.big_is_co ? bch : sc, ci = a.big_is_co ? sc : bch;
                    const float v = acc[mt][q] + X[((nt * 5 + mt) * 16 + q) * 64 + lane];
                    atomicAdd(a.dw + ((long)tap * a.cout_pad + co) * a.cin_pad + ci, v * inv);
                }
        }
    }
    if (a.colsum && big_task) {
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(a.colsum + 4 * cq + e, csum[e]);
    }
}

static int conv_thin_f16x3_launch(const ConvF32Args& v, const f16* wimg, const unsigned* xmax, int cin, bool thin_in,
                                  hipStream_t st, f16* op = nullptr, const unsigned* opmax = nullptr,
                                  float* cpart = nullptr) {
    const int ntiles = (int)conv_tiles(v.B, v.D, v.H, v.W);
    const dim3 g(256);
    if (thin_in) {
        const int epi = conv_epi_code(v.res, v.mask || v.mplanes, !v.accumulate, false);
        if ((op || cpart || v.mplanes) && epi != kEpiMask) return DLCS_ERR_UNSUPPORTED_SIZE;   // the masked form only
        auto launch = [&](auto E) {
            hipLaunchKernelGGL(conv3d_thin_in_f16x3_kernel<decltype(E)::value>, g, dim3(512), 0, st, v, wimg, xmax, cin,
                               ntiles, op, opmax, cpart);
        };
        if (epi == 0) launch(std::integral_constant<int, 0>{});
        else if (epi == kEpiMask) launch(std::integral_constant<int, kEpiMask>{});
        else launch(std::integral_constant<int, kEpiGeneric>{});
    } else {
#ifdef DLCS_DIAG_BUILD
        // DLCS_THIN_OUT_V2=1: the thin-output kernel with LDS-resident weights (A/B timing; 510 vs
        // 480 us); DLCS_THIN_OUT_GW=0: the chunk's weights from an LDS copy, one workgroup per CU
        static const bool v2 = [] { const char* e = dlcs_knob("DLCS_THIN_OUT_V2"); return e && e[0] == '1'; }();
        static const bool gw = [] { const char* e = dlcs_knob("DLCS_THIN_OUT_GW"); return !(e && e[0] == '0'); }();
        if (v2) hipLaunchKernelGGL(conv3d_thin_out_f16x3_v2_kernel, g, dim3(256), 0, st, v, wimg, xmax, ntiles);
        else if (!gw) hipLaunchKernelGGL(conv3d_thin_out_f16x3_kernel<false>, g, dim3(256), 0, st, v, wimg, xmax, ntiles);
        else
#endif
        hipLaunchKernelGGL(conv3d_thin_out_f16x3_kernel<true>, dim3(512), dim3(256), 0, st, v, wimg, xmax, ntiles);
    }
    return dlcs_launch_status();
}
