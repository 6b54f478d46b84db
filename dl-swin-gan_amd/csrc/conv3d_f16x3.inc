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
constexpr int kH3Halo = kHalo * 64;            // f16 in the halo image (76.8 KB)
constexpr int kH3Tap = 160 * 64;               // f16 in one tap slice (20 KB)
constexpr int kH3Slot = 2 * kH3Tap;            // two tap slices per step

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
                const f16x4_t h = *reinterpret_cast<const f16x4_t*>(q), l = *reinterpret_cast<const f16x4_t*>(q + 32);
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
    unsigned nblk = (unsigned)conv_tiles(v.B, v.D, v.H, v.W);
    // the last partial round of 256-CU waves (3360 tiles = 13 x 256 + 32 at BASELINE
    // size: 32 busy CUs for a whole tile time) runs as 5 x ntail single-chunk
    // workgroups plus a fixed-order reduce
    const char* te = dlcs_test_hook("DLCS_H3_TAIL");                 // read per launch (tests toggle it)
    const bool tail_split = !(te && te[0] == '0');
    const unsigned ntail = tail_split ? conv_tail_tiles(nblk) : 0u, nmain = nblk - ntail;
    const bool split = ntail > 0;
    if (split) nblk = nmain;
    const int epi = conv_epi_code(v.res, v.mask || v.mplanes, !v.accumulate, true);
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

// Live-frame window (WIN).  The caller promises that g is exactly zero outside
// frames [t_lo, t_hi) of every batch item (the crop of the network's circular time
// pad: its backward writes zero frames, and each k3 input gradient widens the band
// by one frame per side).  A half patch covers two frames, so the live units are
// the half-slabs hs = 2 t_blk + th in [hs_lo, hs_hi) = [t_lo / 2, ceil(t_hi / 2)) of
// each batch item, walked in the same patch-major order: the first live slab may
// have its second half alone, the last its first half alone, every slab between
// both.  The ranges are cut in live-unit space (sizes differ by at most one unit),
// dead units are neither DMA'd nor multiplied, and the DMA stream follows the live
// sequence one unit at a time (wgl_advance, wgrad_live.h) instead of "unit u + 2 =
// the same half of the next patch"; the half is then a wave-uniform scalar.  The
// prologue stays straight-line code: as a loop it cost five reloads of spilled LDS
// offsets per unit.  WIN = false is the kernel without a window.
struct WgradH3Live { int hs_lo, hs_hi, upr, urem; };   // ranges: upr units each, the first urem one more

template <bool WIN>
__global__ void __launch_bounds__(768) conv3d_wgrad_f16x3_kernel(WgradH3Args a, int nrange, int ppr, WgradH3Live lv) {
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
    if (!WIN && p0 >= p1) return;
    // WIN: this range's live units [lu0, lu1), never empty (the launch has nrange <= live units)
    const WgLiveGeom lg{nT, nY, nX, lv.hs_lo, lv.hs_hi};
    int lu0, lu1;
    wgl_range(lv.upr, lv.urem, range, &lu0, &lu1);
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
    // (WIN: of the unit the DMA stream stands at, with its half in it.th)
    WgLiveIter it{};
    int &ip = it.ip, &ipt = it.ipt, &ipy = it.ipy, &ipx = it.ipx;
    if (WIN) it = wgl_seek(lg, lu0);
    else {
        ip = p0;
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
    // (WIN: the first two live units, each with its own patch and half)
    if (WIN) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (lu0 + s < lu1) {
                const char *gb, *xb;
                unsigned xz;
                bases(gb, xb, xz);
                const unsigned miss = missing();
#pragma unroll
                for (int k = 0; k < 5; ++k) issue_piece(k, it.th, s, miss, gb, xb, xz);
                wgl_advance(lg, it);
            }
        }
    } else {
        const char *gb, *xb;
        unsigned xz;
        bases(gb, xb, xz);
        const unsigned miss = missing();
#pragma unroll
        for (int k = 0; k < 5; ++k) issue_piece(k, 0, 0, miss, gb, xb, xz);
#pragma unroll
        for (int k = 0; k < 5; ++k) issue_piece(k, 1, 1, miss, gb, xb, xz);
    }
    if (!WIN) next_patch();                          // ip = the patch of units u0 + 2, u0 + 3
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
    if (WIN) {
        // the stream stands at live unit u + 2, whose half is the scalar it.th
        for (int u = lu0; u < lu1; ++u) {
            unit(it.th, u + 2 < lu1);
            wgl_advance(lg, it);
        }
    } else {
        for (int u = 2 * p0; u < 2 * p1; ++u) {
            const int th = u & 1;
            unit(th, (u >> 1) + 1 < p1);
            if (th) next_patch();
        }
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

// a.part: wgh3_ranges(npatch, true).nr slabs.  [t_lo, t_hi): the frames of every batch item
// outside which g is exactly zero (the caller's promise); [0, D) or wider = no window.
static int wgrad_f16x3_launch(const WgradH3Args& a, int t_lo, int t_hi, hipStream_t st) {
    const long npatch = (long)a.B * (a.D / 4) * (a.H / 4) * (a.W / 4);
    int hs_lo, hs_hi;
    wgl_halfslabs(a.D, t_lo, t_hi, &hs_lo, &hs_hi);
    if (hs_lo >= hs_hi) return DLCS_OK;              // g = 0 everywhere: dW += 0
    // 32-bit lane offsets (16-B units << 7 in the kernel, relative to a base bias_rows below
    // the patch): 2 bias_rows + 2 patches within 2^25 x 16 B; the zero row's byte offset
    // from a unit base within 2^32
    const long bias_rows = ((long)(a.H / 4) * (a.W / 4) + a.W / 4 + 1) * 64;
    if ((2 * bias_rows + 128) * 40 >= (1L << 25) || (npatch * 64 + bias_rows) * 640 + 1024 >= (1L << 32))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    const PatchRanges r = wgh3_ranges(npatch, false);
    int nr = r.nr;
    const long pp = r.pp;
    if (hs_lo == 0 && hs_hi == a.D / 2)
        hipLaunchKernelGGL(conv3d_wgrad_f16x3_kernel<false>, dim3((unsigned)(9 * nr)), dim3(768), 0, st, a, nr, (int)pp,
                           WgradH3Live{});
    else {
        // as many ranges as without a window (never more than live units), cut over the live units
        const long nlive = (long)a.B * (hs_hi - hs_lo) * (a.H / 4) * (a.W / 4);
        nr = (int)std::min<long>(nr, nlive);
        hipLaunchKernelGGL(conv3d_wgrad_f16x3_kernel<true>, dim3((unsigned)(9 * nr)), dim3(768), 0, st, a, nr, (int)pp,
                           WgradH3Live{hs_lo, hs_hi, (int)(nlive / nr), (int)(nlive % nr)});
    }
    hipLaunchKernelGGL(wgrad_f16x3_reduce_kernel, dim3((unsigned)cdiv(27L * 160 * 40, 256)), dim3(256), 0, st, a, nr);
    return dlcs_launch_status();
}
