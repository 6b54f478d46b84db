// ---------------------------------------------------------------- thin ends from pre-split planes (round 5)
// Part of conv3d_f16x3.hip.  The 160-channel operand of
// the final conv's forward (relu(h), s3d:391) and weight gradient, and of the SFE
// conv's input and weight gradients (g_s, s3d:384), as dlcs_split2_f16 plane
// pairs [rows][320] (one split per tensor, shared by the two kernels that read
// it) DMA'd global -> LDS -- instead of conv3d_thin_f16x3.inc's in-register split
// of fp32 loads, which left those kernels VALU-issue-bound on a 2.3x-redundant
// halo (SQ: 45 % of wave cycles issuing VALU, 0.14-0.32 of HBM).  Every DMA
// source offset is computed once per lane relative to a per-tile scalar base
// (as in the f16x3 weight gradient), halo rows off the grid read the planes'
// zero row (dlcs_split2_f16_bytes).  Run-to-run deterministic: no float atomics.

// ---------------------------------------------------------------- thin output (160 -> Cout <= 4)
// The output-shift formulation of conv3d_thin_out_f16x3_kernel: Q[(t, y, x')][(kw,
// co)] = sum_{kd, kh, ci} W[kd, kh, kw][co][ci] x[t + kd - 1, y + kh - 1, x' - 1][ci]
// over the tile's 4 t x 8 y x 6 x' rows (192 = 12 M tiles, N = 12 of 16 used), then
// out[t, y, x][co] = sum_kw Q[(t, y, x + kw)][(kw, co)].  Tile = 4 t x 8 y x 4 x
// output voxels (1 x 2 x 1 patches); its halo [6][10][6] = 360 rows of one
// 32-channel chunk [xh 32 | xl 32] (128 B, eight 16-B pieces XOR-swizzled by
// ((R >> 1) & 3) << 1) is DMA'd one (tile, chunk) item ahead into a 2-buffer ring
// (2 x 45 KB); the weights of all 5 chunks (the 12 used (kw, co) columns, 67.5 KB)
// stay in LDS.  8 waves: M tiles 3 (w & 3) .. + 2, (kd, kh) pairs 0..4 (w < 4) or
// 5..8 (w >= 4) -- the two halves meet in LDS before the kw gather.
constexpr int kTpHY = 10, kTpHX = 6, kTpHalo = 6 * kTpHY * kTpHX;   // 360 halo rows
constexpr int kTpBuf = kTpHalo * 64;                                // f16 per halo buffer (45 KB)
constexpr int kTpPieces = kTpHalo * 8 / 64;                         // 45 DMA wave-instructions per item

#ifdef DLCS_DIAG_BUILD                                  // the two-buffer form: DLCS_THIN_OUT_P2=1
__global__ void __launch_bounds__(512, 1) conv3d_thin_out_p_kernel(ConvF32Args a, const f16* xp, const f16* wimg,
                                                                   long rows) {
    __shared__ __attribute__((aligned(16))) f16 smem_tp[2 * kTpBuf + kThinOutW2];
    f16* Wl = smem_tp + 2 * kTpBuf;
    // weights: global [cc][kk][plane][kg][n 16][8] -> LDS [cc][kk][plane][kg][n 12][8]
    for (int i = threadIdx.x; i < kThinOutW2 / 8; i += 512) {
        const int n = i % 12, rest = i / 12;
        const int kg = rest & 3, pl = (rest >> 2) & 1, ck = rest >> 3;
        reinterpret_cast<uint4*>(Wl)[i] = reinterpret_cast<const uint4*>(wimg)[(ck * 1024 + pl * 512 + (kg * 16 + n) * 8) / 8];
    }
    const float sx = f16x3_scale(*reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(xp) + rows * 640));
    const float inv = 1.0f / (sx * *reinterpret_cast<const float*>(wimg + kThinOutHalfs));
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int nYX = nY * nX, nYt = (nY + 1) >> 1;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, kg = lane >> 4;
    const int wn = m < 12 ? m : 11;
    const int bias_rows = (nYX + nX + 1) * 64;

    // DMA pieces of this wave: wi = 8 k + wave < 45; lane -> halo row 8 wi + lane / 8,
    // physical piece lane % 8 <- logical piece (lane % 8) ^ swz(row).
    // pk[k] = (byte offset / 16 from the tile base, + bias) << 8 | 7 neighbour bits
    // (t-, t+, y-, y+1, y+2, x-, x+)
    unsigned pk[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int wi = 8 * k + wave;
        const int hv = min(wi * 8 + (lane >> 3), kTpHalo - 1);
        const int ht = hv / (kTpHY * kTpHX), hy = (hv / kTpHX) % kTpHY, hx = hv % kTpHX;
        const int L = (lane & 7) ^ (((hv >> 1) & 3) << 1);
        const int t = ht - 1, y = hy - 1, x = hx - 1;
        const int dt = t >> 2, dy = y >> 2, dx = x >> 2;
        const unsigned req = (dt < 0 ? 1u : 0u) | (dt > 0 ? 2u : 0u) | (dy < 0 ? 4u : 0u) | (dy == 1 ? 8u : 0u) |
                             (dy == 2 ? 16u : 0u) | (dx < 0 ? 32u : 0u) | (dx > 0 ? 64u : 0u);
        const int rel = ((dt * nYX + dy * nX + dx) << 6) + ((t & 3) << 4) + ((y & 3) << 2) + (x & 3);
        const unsigned off16 = (unsigned)((rel + bias_rows) * 40 + L);
        pk[k] = wi < kTpPieces ? (off16 << 8) | req : 0u;
    }
    const unsigned dst0 = __builtin_amdgcn_readfirstlane(lds_offset(smem_tp));
    // tile walk: blocks of 4 (y tile pairs) x 8 (x patches) tiles; XCD x takes blocks x, x + 8, ...
    // and its 32 workgroups the 32 tiles of a block together, so the tiles in flight on one
    // L2 form a compact 32 x 32-voxel patch of the volume whose halo rows they share
    // (a contiguous run per workgroup missed L2 on 96 % of its halo reads)
    const int nBY = (nYt + 3) >> 2, nBX = (nX + 7) >> 3;
    const int nblocks = a.B * nT * nBY * nBX, xcd = blockIdx.x & 7, kw = blockIdx.x >> 3;
    const int nrounds = xcd < nblocks ? (nblocks - xcd + 7) >> 3 : 0;
    const int nitems = nrounds * 5;
    // tile of round r for this workgroup; false when it lies past the volume's edge
    auto decode = [&](int r, int& b, int& pt, int& py2, int& px) {
        int bid = r * 8 + xcd;
        const int bx = bid % nBX; bid /= nBX;
        const int by = bid % nBY; bid /= nBY;
        pt = bid % nT;
        b = bid / nT;
        py2 = by * 4 + (kw >> 3);
        px = bx * 8 + (kw & 7);
        return py2 < nYt && px < nX;
    };
    auto issue = [&](int s) {                                   // DMA of item s into buffer s & 1
        if (s >= nitems) return;
        int b, pt, py2, px;
        if (!decode(s / 5, b, pt, py2, px)) return;
        const int cc = s % 5;
        const long r0 = ((((long)b * nT + pt) * nY + 2 * py2) * nX + px) * 64 - bias_rows;
        const char* sb = reinterpret_cast<const char*>(xp) + r0 * 640 + cc * 128;
        const unsigned zoff = (unsigned)(rows * 640 + 256 - r0 * 640 - cc * 128);
        const unsigned miss = (pt == 0 ? 1u : 0u) | (pt == nT - 1 ? 2u : 0u) | (py2 == 0 ? 4u : 0u) |
                              (2 * py2 + 1 >= nY ? 8u : 0u) | (2 * py2 + 2 >= nY ? 16u : 0u) | (px == 0 ? 32u : 0u) |
                              (px == nX - 1 ? 64u : 0u);
        const unsigned dst = dst0 + (unsigned)((s & 1) * kTpBuf * 2);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int wi = 8 * k + wave;
            if (wi < kTpPieces) {
                const unsigned v = pk[k];
                const unsigned off = (v & miss) ? zoff : ((v >> 4) & ~15u);
                glds16_s(sb, off, dst + (unsigned)(wi * 1024));
            }
        }
    };
    // M rows of this wave: r = 16 (3 (w & 3) + i) + m = (t 8 + y) 6 + x'
    int hb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int r = 16 * (3 * (wave & 3) + i) + m;
        const int xq = r % 6, y = (r / 6) % 8, t = r / 48;
        hb[i] = (t * kTpHY + y) * kTpHX + xq;
    }
    const int kk0 = wave < 4 ? 0 : 5, kk1 = wave < 4 ? 5 : 9;
    f32x4_t acc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) acc[i] = (f32x4_t)0.0f;

    issue(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                           // weights and item 0 in LDS
    for (int s = 0; s < nitems; ++s) {
#pragma unroll
        for (int k = 0; k < 6; ++k) asm volatile("" : "+v"(pk[k]));   // no hoisting of the decoded pieces
        issue(s + 1);
        const int cc = s % 5;
        int b, pt, py2, px;
        const bool live = decode(s / 5, b, pt, py2, px);       // workgroup-uniform
        const f16* Hs = smem_tp + (s & 1) * kTpBuf;
        const f16* wc = Wl + cc * 9 * 768 + (kg * 12 + wn) * 8;
        for (int kk = live ? kk0 : kk1; kk < kk1; ++kk) {
            const int kd = kk / 3, kh = kk - 3 * kd;
            const f16* wb = wc + kk * 768;
            const f16x8_t bh = *reinterpret_cast<const f16x8_t*>(wb);
            const f16x8_t bl = *reinterpret_cast<const f16x8_t*>(wb + 384);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int R = hb[i] + (kd * kTpHY + kh) * kTpHX;
                const int swz = ((R >> 1) & 3) << 1;
                const f16x8_t ah = *reinterpret_cast<const f16x8_t*>(Hs + R * 64 + ((kg ^ swz) << 3));
                const f16x8_t al = *reinterpret_cast<const f16x8_t*>(Hs + R * 64 + (((4 + kg) ^ swz) << 3));
                f32x4_t t = (f32x4_t)0.0f;                     // fresh tile, VALU-added (FOLD, conv3d_f16x3.inc)
                mfma16h(t, al, bh);
                mfma16h(t, ah, bl);
                mfma16h(t, ah, bh);
                acc[i] += t;
            }
        }
        if (cc == 4 && live) {
            __syncthreads();                                   // every wave is done with buffer s & 1
            // Q halves -> LDS [2][192][17] in the free buffer; C/D row = 4 kg + r, col n = m
            float* Q = reinterpret_cast<float*>(smem_tp + (s & 1) * kTpBuf);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    Q[((wave >> 2) * 192 + 16 * (3 * (wave & 3) + i) + 4 * kg + r) * 17 + m] = acc[i][r] * inv;
#pragma unroll
            for (int i = 0; i < 3; ++i) acc[i] = (f32x4_t)0.0f;
            __syncthreads();
            if (threadIdx.x < 128) {                           // one output voxel per thread: 4 t x 8 y x 4 x
                const int v = threadIdx.x;
                const int t = v >> 5, y = (v >> 2) & 7, x = v & 3;
                const int py = 2 * py2 + (y >> 2);
                if (py < nY) {
                    f32x4_t o = (f32x4_t)0.0f;
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const int qr = (t * 8 + y) * 6 + x + kw;
#pragma unroll
                        for (int co = 0; co < 4; ++co) o[co] += Q[qr * 17 + kw * 4 + co] + Q[(192 + qr) * 17 + kw * 4 + co];
                    }
                    const long row = brow(b, pt * 4 + t, py * 4 + (y & 3), px * 4 + x, nT, nY, nX);
                    float* op = a.out + row * a.cout_ld;
                    if (a.bias) for (int co = 0; co < a.cout; ++co) o[co] += a.bias[co];
                    if (a.relu_out) for (int co = 0; co < 4; ++co) o[co] = fmaxf(o[co], 0.0f);
                    if (a.accumulate) o += *reinterpret_cast<const f32x4_t*>(op);
                    *reinterpret_cast<f32x4_t*>(op) = o;
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // item s + 1 has landed
        __syncthreads();
    }
}
#endif  // DLCS_DIAG_BUILD

// Three-buffer form (round 6): the kernel above holds ONE item in flight per CU (one
// 46 KB halo DMA, then a wait): a latency-bound 1.7 TB/s.  Here the weights leave LDS
// -- each wave loads its B fragments of an item (its 5 / 4 (kd, kh) pairs x 2 planes,
// 16 B per lane, L2-resident) into registers one item ahead -- and the freed 67.5 KB
// hold a third halo buffer, so items s + 1 and s + 2 are in flight while s computes
// (counted vmcnt waits: the B loads of s + 1 are issued before the DMA of s + 2).
// Same tile walk, products and epilogue.
template <int SET>
DLCS_DEV void thin_out_p3_b(const f16* wimg, int cc, int kk0, int kg, int m, f16x8_t (&bh)[2][5], f16x8_t (&bl)[2][5]) {
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const int kk = min(kk0 + q, 8);
        const f16* wb = wimg + (cc * 9 + kk) * 1024 + (kg * 16 + m) * 8;
        bh[SET][q] = *reinterpret_cast<const f16x8_t*>(wb);
        bl[SET][q] = *reinterpret_cast<const f16x8_t*>(wb + 512);
    }
}

// Slab window [tb0, tb1) of the tile walk: only the tiles of those 4-frame slabs are
// computed (their halos still reach into the slabs beside them), the output rows of the
// other slabs are left untouched -- for a caller that never reads them.  [0, nT) = all.
__global__ void __launch_bounds__(512, 1) conv3d_thin_out_p3_kernel(ConvF32Args a, const f16* xp, const f16* wimg,
                                                                    long rows, int tb0, int tb1) {
    __shared__ __attribute__((aligned(16))) f16 smem_tp3[3 * kTpBuf];           // 135 KB
    const float sx = f16x3_scale(*reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(xp) + rows * 640));
    const float inv = 1.0f / (sx * *reinterpret_cast<const float*>(wimg + kThinOutHalfs));
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int nYX = nY * nX, nYt = (nY + 1) >> 1;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, kg = lane >> 4;
    const int bias_rows = (nYX + nX + 1) * 64;
    unsigned pk[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int wi = 8 * k + wave;
        const int hv = min(wi * 8 + (lane >> 3), kTpHalo - 1);
        const int ht = hv / (kTpHY * kTpHX), hy = (hv / kTpHX) % kTpHY, hx = hv % kTpHX;
        const int L = (lane & 7) ^ (((hv >> 1) & 3) << 1);
        const int t = ht - 1, y = hy - 1, x = hx - 1;
        const int dt = t >> 2, dy = y >> 2, dx = x >> 2;
        const unsigned req = (dt < 0 ? 1u : 0u) | (dt > 0 ? 2u : 0u) | (dy < 0 ? 4u : 0u) | (dy == 1 ? 8u : 0u) |
                             (dy == 2 ? 16u : 0u) | (dx < 0 ? 32u : 0u) | (dx > 0 ? 64u : 0u);
        const int rel = ((dt * nYX + dy * nX + dx) << 6) + ((t & 3) << 4) + ((y & 3) << 2) + (x & 3);
        const unsigned off16 = (unsigned)((rel + bias_rows) * 40 + L);
        pk[k] = wi < kTpPieces ? (off16 << 8) | req : 0u;
    }
    const int npc = wave < kTpPieces - 40 ? 6 : 5;               // this wave's DMA instructions per item
    const unsigned dst0 = __builtin_amdgcn_readfirstlane(lds_offset(smem_tp3));
    const int nBY = (nYt + 3) >> 2, nBX = (nX + 7) >> 3;
    const int nTw = tb1 - tb0;
    const int nblocks = a.B * nTw * nBY * nBX, xcd = blockIdx.x & 7, kw = blockIdx.x >> 3;
    const int nrounds = xcd < nblocks ? (nblocks - xcd + 7) >> 3 : 0;
    const int nitems = nrounds * 5;
    auto decode = [&](int r, int& b, int& pt, int& py2, int& px) {
        int bid = r * 8 + xcd;
        const int bx = bid % nBX; bid /= nBX;
        const int by = bid % nBY; bid /= nBY;
        pt = tb0 + bid % nTw;
        b = bid / nTw;
        py2 = by * 4 + (kw >> 3);
        px = bx * 8 + (kw & 7);
        return py2 < nYt && px < nX;
    };
    auto issue = [&](int s) {                                   // DMA of item s into buffer s % 3; pieces issued
        if (s >= nitems) return 0;
        int b, pt, py2, px;
        if (!decode(s / 5, b, pt, py2, px)) return 0;
        const int cc = s % 5;
        const long r0 = ((((long)b * nT + pt) * nY + 2 * py2) * nX + px) * 64 - bias_rows;
        const char* sb = reinterpret_cast<const char*>(xp) + r0 * 640 + cc * 128;
        const unsigned zoff = (unsigned)(rows * 640 + 256 - r0 * 640 - cc * 128);
        const unsigned miss = (pt == 0 ? 1u : 0u) | (pt == nT - 1 ? 2u : 0u) | (py2 == 0 ? 4u : 0u) |
                              (2 * py2 + 1 >= nY ? 8u : 0u) | (2 * py2 + 2 >= nY ? 16u : 0u) | (px == 0 ? 32u : 0u) |
                              (px == nX - 1 ? 64u : 0u);
        const unsigned dst = dst0 + (unsigned)((s % 3) * kTpBuf * 2);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int wi = 8 * k + wave;
            if (wi < kTpPieces) {
                const unsigned v = pk[k];
                const unsigned off = (v & miss) ? zoff : ((v >> 4) & ~15u);
                glds16_s(sb, off, dst + (unsigned)(wi * 1024));
            }
        }
        return npc;
    };
    auto vmwait = [&](int n) {                                  // s_waitcnt vmcnt(n), n in {0, 5, 6}
        if (n >= 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else if (n == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    int hb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int r = 16 * (3 * (wave & 3) + i) + m;
        const int xq = r % 6, y = (r / 6) % 8, t = r / 48;
        hb[i] = (t * kTpHY + y) * kTpHX + xq;
    }
    const int kk0 = wave < 4 ? 0 : 5, nkk = wave < 4 ? 5 : 4;
    f32x4_t acc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) acc[i] = (f32x4_t)0.0f;
    f16x8_t bh[2][5], bl[2][5];

    thin_out_p3_b<0>(wimg, 0, kk0, kg, m, bh, bl);
    issue(0);
    const int n1 = issue(1);
    vmwait(n1);                                                // B(0) and item 0 have landed
    __syncthreads();
    auto body = [&](int s, auto SETc) {
        constexpr int SET = decltype(SETc)::value;
#pragma unroll
        for (int k = 0; k < 6; ++k) asm volatile("" : "+v"(pk[k]));   // no hoisting of the decoded pieces
        if (s + 1 < nitems) thin_out_p3_b<SET ^ 1>(wimg, (s + 1) % 5, kk0, kg, m, bh, bl);
        const int n2 = issue(s + 2);
        const int cc = s % 5;
        int b, pt, py2, px;
        const bool live = decode(s / 5, b, pt, py2, px);       // workgroup-uniform
        const f16* Hs = smem_tp3 + (s % 3) * kTpBuf;
        if (live) {
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                if (q < nkk) {
                    const int kk = kk0 + q;
                    const int kd = kk / 3, kh = kk - 3 * kd;
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const int R = hb[i] + (kd * kTpHY + kh) * kTpHX;
                        const int swz = ((R >> 1) & 3) << 1;
                        const f16x8_t ah = *reinterpret_cast<const f16x8_t*>(Hs + R * 64 + ((kg ^ swz) << 3));
                        const f16x8_t al = *reinterpret_cast<const f16x8_t*>(Hs + R * 64 + (((4 + kg) ^ swz) << 3));
                        f32x4_t t = (f32x4_t)0.0f;             // fresh tile, VALU-added (FOLD, conv3d_f16x3.inc)
                        mfma16h(t, al, bh[SET][q]);
                        mfma16h(t, ah, bl[SET][q]);
                        mfma16h(t, ah, bh[SET][q]);
                        acc[i] += t;
                    }
                }
            }
        }
        if (cc == 4 && live) {
            __syncthreads();                                   // every wave is done with buffer s % 3
            float* Q = reinterpret_cast<float*>(smem_tp3 + (s % 3) * kTpBuf);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    Q[((wave >> 2) * 192 + 16 * (3 * (wave & 3) + i) + 4 * kg + r) * 17 + m] = acc[i][r] * inv;
#pragma unroll
            for (int i = 0; i < 3; ++i) acc[i] = (f32x4_t)0.0f;
            __syncthreads();
            if (threadIdx.x < 128) {                           // one output voxel per thread: 4 t x 8 y x 4 x
                const int v = threadIdx.x;
                const int t = v >> 5, y = (v >> 2) & 7, x = v & 3;
                const int py = 2 * py2 + (y >> 2);
                if (py < nY) {
                    f32x4_t o = (f32x4_t)0.0f;
#pragma unroll
                    for (int kw3 = 0; kw3 < 3; ++kw3) {
                        const int qr = (t * 8 + y) * 6 + x + kw3;
#pragma unroll
                        for (int co = 0; co < 4; ++co) o[co] += Q[qr * 17 + kw3 * 4 + co] + Q[(192 + qr) * 17 + kw3 * 4 + co];
                    }
                    const long row = brow(b, pt * 4 + t, py * 4 + (y & 3), px * 4 + x, nT, nY, nX);
                    float* op = a.out + row * a.cout_ld;
                    if (a.bias) for (int co = 0; co < a.cout; ++co) o[co] += a.bias[co];
                    if (a.relu_out) for (int co = 0; co < 4; ++co) o[co] = fmaxf(o[co], 0.0f);
                    if (a.accumulate) o += *reinterpret_cast<const f32x4_t*>(op);
                    *reinterpret_cast<f32x4_t*>(op) = o;
                }
            }
        }
        vmwait(n2);                                            // B(s + 1) and item s + 1 have landed
        __syncthreads();
    };
    for (int s = 0; s < nitems; s += 2) {
        body(s, std::integral_constant<int, 0>{});
        if (s + 1 < nitems) body(s + 1, std::integral_constant<int, 1>{});
    }
}

static int conv_thin_out_p_launch(const ConvF32Args& v, const f16* xp, const f16* wimg, int tb0, int tb1,
                                  hipStream_t st) {
    const int nT = v.D / 4, nY = v.H / 4, nX = v.W / 4;
    tb0 = std::max(tb0, 0);
    tb1 = std::min(tb1, nT);
    if (tb0 >= tb1) return DLCS_OK;                  // no slab to compute
    const long rows = (long)v.B * v.D * v.H * v.W;
    const long bias_rows = ((long)nY * nX + nX + 1) * 64;
    // 16-B offsets relative to a base bias_rows below the tile (24 bits in the kernel);
    // the zero row's byte offset from a tile base within 2^32
    if ((2 * bias_rows + 4L * nX * 64 + 256) * 40 >= (1L << 24) || (rows + bias_rows) * 640 + 1024 >= (1L << 32))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    // 8 XCDs x 32 workgroups (one per CU): one 4 x 8-tile block per XCD and round;
    // DLCS_THIN_OUT_P2=1 (DIAG build): the two-buffer kernel with LDS weights, for A/B timing
#ifdef DLCS_DIAG_BUILD
    static const bool p2 = [] { const char* e = dlcs_knob("DLCS_THIN_OUT_P2"); return e && e[0] == '1'; }();
    if (p2 && tb0 == 0 && tb1 == nT)
        hipLaunchKernelGGL(conv3d_thin_out_p_kernel, dim3(256), dim3(512), 0, st, v, xp, wimg, rows);
    else
#endif
    hipLaunchKernelGGL(conv3d_thin_out_p3_kernel, dim3(256), dim3(512), 0, st, v, xp, wimg, rows, tb0, tb1);
    return dlcs_launch_status();
}

// ---------------------------------------------------------------- weight gradient, 160 <-> thin
// dW = Big^T . Thin_im2col with the tap shift on the thin side (u = v + off), as
// conv3d_wgrad_thin_f16x3_kernel:
//   SFE   (Cin <= 4):  dW[tap][co][ci] = sum_u g[u][co] x[u + off(tap)][ci]   (Big = g_s planes, sgn +1)
//   final (Cout <= 4): dW[tap][co][ci] = sum_u x[u][ci] g[u - off(tap)][co]   (Big = relu(h) planes, sgn -1)
// M = 160 Big channels (10 tiles of 16), N = (tap, s) = 4 tap + s (108 of 128: 8
// tiles), K = voxels, two 32-voxel units per patch on v_mfma_f32_16x16x32_f16 with
// the f16x3 weight gradient's transposed operand reads (ds_read_b64_tr_b16): the
// Big planes DMA'd into its [32 rows][160] images (same pieces and swizzle), the
// thin side's 6 x 6 x 6 halo rows (first 16 B: 4 fp32 channels) DMA'd raw, split
// and scattered into an im2col image [32 rows][128 columns] per plane and unit
// (16-column tiles swizzled as the Big image).  Patch p + 1's DMA runs during patch
// p's products; 8 waves = 2 M halves x 4 N pairs.  Each workgroup stores its raw
// [160][128] partial; wgrad_thin_p_reduce_kernel sums them in a fixed order.
//
// Live-frame window on the thin operand (final conv shape, lv.per > 0): the caller promises
// that the thin tensor is exactly zero outside frames [t_lo, t_hi) of every batch item.  A
// patch gathers it through a one-frame tap halo, so the patches of a 4-frame slab are dead iff
// the slab's frames widened by one per side miss the window (wgl_slabs); the workgroups cut
// their ranges over the live patches (sizes differ by at most one, empty ranges store zeros)
// and dead patches are neither DMA'd nor multiplied.
struct ThinWgPLive { int per, item, first, base, rem; };   // wgl_live_patch / wgl_range; per = 0: no window
struct ThinWgPArgs {
    const f16* bp; const float* thin; float* dw; float* part;
    const unsigned* thin_max;
    long rows;
    int thin_ld, sgn, big_is_co, thin_ch, cout_pad, cin_pad;
    int B, D, H, W;
};
constexpr int kTwImg = 32 * 160;                         // f16 per Big plane image (one unit)
constexpr int kTwBigB = 2 * 2 * kTwImg;                  // f16 per buffer: 2 units x 2 planes (40 KB)
constexpr int kTwTR = 256 * 8;                           // f16 of raw thin rows (16 B each, 216 used) per buffer
constexpr int kTwBuf = kTwBigB + kTwTR;
constexpr int kTwIm = 32 * 128;                          // f16 per im2col plane image (one unit)

__global__ void __launch_bounds__(512, 1) conv3d_wgrad_thin_p_kernel(ThinWgPArgs a, int ppr, ThinWgPLive lv) {
    __shared__ __attribute__((aligned(16))) f16 smem_twp[2 * kTwBuf + 4 * kTwIm];      // 121.6 KB
    f16* IM = smem_twp + 2 * kTwBuf;
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const int npatch = a.B * nT * nY * nX;
    // this workgroup's patches: numbers [p0, p1) of the live patches (no window: of all patches)
    int p0 = (int)blockIdx.x * ppr, p1 = min(npatch, p0 + ppr);
    if (lv.per) wgl_range(lv.base, lv.rem, (int)blockIdx.x, &p0, &p1);
    auto patch_of = [&](int u) { return lv.per ? wgl_live_patch(u, lv.per, lv.item, lv.first) : u; };
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float st = f16x3_scale(*a.thin_max);
    // im2col padding columns 108..127 (tile 7 minus 4 columns) stay zero: rows x 20 columns
    for (int i = tid; i < 4 * 32 * 20; i += 512) {
        const int img = i / 640, r = (i / 20) % 32, c = 108 + i % 20;
        IM[img * kTwIm + r * 128 + (c ^ (((r >> 3) & 1) << 4))] = (f16)0.0f;
    }
    // Big DMA pieces of this wave: wi = 8 k + wave (< 40): unit wi / 20, plane (wi / 10) & 1,
    // piece wl = wi % 10 of the f16x3 weight gradient's g pieces
    unsigned boff[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int wi = 8 * k + wave, wl = wi % 10, pl = (wi / 10) & 1, un = wi / 20;
        const int c = wl * 64 + lane;
        const int row = c / 20, kp = c - row * 20;
        const int kl = kp ^ (((row >> 3) & 1) << 1);
        boff[k] = (unsigned)(((un * 32 + row) * 320 + (kl >> 2) * 64 + pl * 32 + (kl & 3) * 8) * 2);
    }
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_offset(smem_twp));
    auto coords = [&](int patch, int& bb, int& pt, int& py, int& px) {
        px = patch % nX;
        int r = patch / nX;
        py = r % nY; r /= nY;
        pt = r % nT;
        bb = r / nT;
    };
    auto issue = [&](int u, int buf) {
        if (u >= p1) return;
        const int patch = patch_of(u);
        const char* sb = reinterpret_cast<const char*>(a.bp) + (long)patch * 64 * 640;
        const unsigned dst = lds0 + (unsigned)(buf * kTwBuf * 2);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int wi = 8 * k + wave, wl = wi % 10, pl = (wi / 10) & 1, un = wi / 20;
            glds16_s(sb, boff[k], dst + (unsigned)((un * 2 + pl) * kTwImg * 2 + wl * 1024));
        }
        if (wave < 4) {                                   // raw thin halo rows (clamped: masked when built)
            int bb, pt, py, px;
            coords(patch, bb, pt, py, px);
            const int hv = min(wave * 64 + lane, 215);
            const int ht = hv / 36, hy = (hv / 6) % 6, hx = hv % 6;
            const int T = min(max(pt * 4 - 1 + ht, 0), a.D - 1), Y = min(max(py * 4 - 1 + hy, 0), a.H - 1),
                      X = min(max(px * 4 - 1 + hx, 0), a.W - 1);
            glds16(a.thin + brow(bb, T, Y, X, nT, nY, nX) * a.thin_ld,
                   dst + (unsigned)(kTwBigB * 2 + wave * 1024));
        }
    };
    // im2col job of this thread (tid < 216): tap, 8-voxel chunk tc (t = tc >> 1, y pair tc & 1)
    const int jtap = tid >> 3, tc = tid & 7;
    const int skd = a.sgn * (jtap / 9 - 1), skh = a.sgn * ((jtap / 3) % 3 - 1), skw = a.sgn * (jtap % 3 - 1);
    auto build = [&](int u, int buf) {
        if (tid >= 216) return;
        const int patch = patch_of(u);
        int bb, pt, py, px;
        coords(patch, bb, pt, py, px);
        const float* TR = reinterpret_cast<const float*>(smem_twp + buf * kTwBuf + kTwBigB);
        const int t = tc >> 1;
        const bool tok = (unsigned)(pt * 4 + t + skd) < (unsigned)a.D;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int y = 2 * (tc & 1) + (j >> 2), x = j & 3;
            const bool ok = tok && (unsigned)(py * 4 + y + skh) < (unsigned)a.H && (unsigned)(px * 4 + x + skw) < (unsigned)a.W;
            const int hv = (t + 1 + skd) * 36 + (y + 1 + skh) * 6 + (x + 1 + skw);
            f32x4_t v = *reinterpret_cast<const f32x4_t*>(TR + hv * 4);
            f16x4_t h, l;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float u = (ok && e < a.thin_ch) ? v[e] * st : 0.0f;
                const f16 hh = (f16)u;
                h[e] = hh;
                l[e] = (f16)(u - (float)hh);
            }
            const int un = t >> 1, row = (t & 1) * 16 + y * 4 + x;
            const int col = (jtap * 4) ^ (((row >> 3) & 1) << 4);
            *reinterpret_cast<f16x4_t*>(IM + (un * 2 + 0) * kTwIm + row * 128 + col) = h;
            *reinterpret_cast<f16x4_t*>(IM + (un * 2 + 1) * kTwIm + row * 128 + col) = l;
        }
    };

    const int mh = wave & 1, nq = wave >> 1;
    f32x4_t acc[5][2];
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4_t)0.0f;
    const int gq = lane >> 4, q = (lane >> 2) & 3, p4 = (lane & 3) * 4, swb = gq & 1;
    auto acol = [&](int i) { return (((mh * 5 + i) ^ swb) << 4) + p4; };
    auto bcol = [&](int j) { return (((nq * 2 + j) ^ swb) << 4) + p4; };
    const int grow = (8 * gq + q) * 160, trow = (8 * gq + q) * 128;

    if (p0 < p1) issue(p0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int p = p0; p < p1; ++p) {
#pragma unroll
        for (int k = 0; k < 5; ++k) asm volatile("" : "+v"(boff[k]));
        const int buf = (p - p0) & 1;
        issue(p + 1, buf ^ 1);
        build(p, buf);
        __syncthreads();                                  // im2col of patch p published
#pragma unroll
        for (int un = 0; un < 2; ++un) {
            const f16* Gh = smem_twp + buf * kTwBuf + (un * 2) * kTwImg + grow;
            const f16* Gl = Gh + kTwImg;
            const f16* Th = IM + (un * 2) * kTwIm + trow;
            const f16* Tl = Th + kTwIm;
            f16x8_t bh[2], bl[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                bh[j] = tr_read16h(Th + bcol(j), Th + 4 * 128 + bcol(j));
                bl[j] = tr_read16h(Tl + bcol(j), Tl + 4 * 128 + bcol(j));
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const f16x8_t gh = tr_read16h(Gh + acol(i), Gh + 4 * 160 + acol(i));
                const f16x8_t gl = tr_read16h(Gl + acol(i), Gl + 4 * 160 + acol(i));
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    mfma16h(acc[i][j], gh, bh[j]);
                    mfma16h(acc[i][j], gh, bl[j]);
                    mfma16h(acc[i][j], gl, bh[j]);
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // patch p + 1 has landed
        __syncthreads();
    }
    // raw partial [160][128] of this workgroup: row m = 16 (mh 5 + i) + 4 gq + r, column 16 (nq 2 + j) + (lane & 15)
    float* pp = a.part + (long)blockIdx.x * 160 * 128;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                pp[(16 * (mh * 5 + i) + 4 * gq + r) * 128 + 16 * (nq * 2 + j) + (lane & 15)] = acc[i][j][r];
}

// dW += inv * sum over workgroups (fixed order) of the raw partials, into the
// dlcs_conv3d_pack_weights layout [27][cout_pad][cin_pad].  Block = 64 consecutive
// (m, n) of the [160][128] partial x 4 quarters of the workgroups (each quarter's
// 64 partials summed by 4 independent accumulators, then the quarters in order):
// one thread per output walking all 256 partials in a dependent chain was
// latency-bound (76 us).
__global__ void __launch_bounds__(256) wgrad_thin_p_reduce_kernel(ThinWgPArgs a, int nwg) {
    __shared__ float red[4][64];
    const int o = blockIdx.x * 64 + (threadIdx.x & 63), wq = threadIdx.x >> 6;
    float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int per = nwg / 4;                                       // nwg % 16 == 0
    const float* pp = a.part + (long)(wq * per) * 160 * 128 + o;
    for (int w = 0; w < per; w += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) s4[u] += pp[(long)(w + u) * 160 * 128];
    }
    red[wq][threadIdx.x & 63] = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    __syncthreads();
    if (wq != 0) return;
    const int mm = o / 128, n = o % 128, tap = n >> 2, s = n & 3;
    if (n >= 108 || s >= a.thin_ch) return;
    const int l = threadIdx.x;
    const float v = (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
    const unsigned bmax = *reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(a.bp) + a.rows * 640);
    const float inv = 1.0f / (f16x3_scale(bmax) * f16x3_scale(*a.thin_max));
    const int co = a.big_is_co ? mm : s, ci = a.big_is_co ? s : mm;
    float* d = a.dw + ((long)tap * a.cout_pad + co) * a.cin_pad + ci;
    *d += v * inv;
}

// a.part: partial slabs (256 workgroups x [160][128])
constexpr int kTwpWG = 256;

// [t_lo, t_hi): the frames of every batch item outside which the thin tensor is exactly zero
// (the caller's promise); [0, D) or wider = no window
static int wgrad_thin_p_launch(const ThinWgPArgs& a, int t_lo, int t_hi, hipStream_t st) {
    const int nT = a.D / 4, nYX = (a.H / 4) * (a.W / 4);
    const long npatch = (long)a.B * nT * nYX;
    if (npatch * 64 * 640 >= (1L << 32)) return DLCS_ERR_UNSUPPORTED_SIZE;       // 32-bit DMA offsets
    int s0, s1;
    wgl_slabs(a.D, t_lo, t_hi, 1, &s0, &s1);
    if (s0 >= s1) return DLCS_OK;                    // thin = 0 everywhere: dW += 0
    const int ppr = (int)((npatch + kTwpWG - 1) / kTwpWG);
    ThinWgPLive lv{};
    if (s0 > 0 || s1 < nT) {
        const int per = (s1 - s0) * nYX, n = a.B * per;
        lv = ThinWgPLive{per, nT * nYX, s0 * nYX, n / kTwpWG, n % kTwpWG};
    }
    hipLaunchKernelGGL(conv3d_wgrad_thin_p_kernel, dim3(kTwpWG), dim3(512), 0, st, a, ppr, lv);
    hipLaunchKernelGGL(wgrad_thin_p_reduce_kernel, dim3(160 * 128 / 64), dim3(256), 0, st, a, kTwpWG);
    return dlcs_launch_status();
}
